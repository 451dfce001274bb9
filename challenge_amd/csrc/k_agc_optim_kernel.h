// k_agc_optim_kernel.h -- the text of the AGC + clipvalue + sgd / rmsprop launches (see k_agc_optim.h, which includes this file FOUR
// times, as k_agc_adam.h includes k_agc_adam_kernel.h twice): IRIS_K_RMS 0 = torch.optim.SGD with momentum, 1 = torch.optim.RMSprop
// with momentum; IRIS_K_EMA 1 = the sibling that carries the updated parameter - still in its register - on into an exponential
// moving average of the weights.  IRIS_K_NAME is the kernel's name.  The rows are iris_agc_adam_row / iris_agc_adam_ema_row: the
// momentum buffer stands in the `exp_avg` slot, rmsprop's square average in the `exp_avg_sq` slot - a slot sgd never reads, neither
// the pointer nor what it points at.  No include guard on purpose.
#if IRIS_K_EMA
#define IRIS_K_ROW iris_agc_adam_ema_row
#else
#define IRIS_K_ROW iris_agc_adam_row
#endif
__global__ __launch_bounds__(256) void IRIS_K_NAME(const IRIS_K_ROW* rows, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                                   int use_agc, const float* lr_dev, float lr_host, float mu
#if IRIS_K_RMS
                                                   , double alphad, float eps
#endif
#if IRIS_K_EMA
                                                   , const float* step_dev, double decay
#endif
) {
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * 4;
    const float lr = lr_dev ? lr_dev[0] : lr_host;
    const bool clamp = clipvalue > 0.f;
#if IRIS_K_RMS
    // (alpha stays a double up to here, as the Adam launch keeps its betas: 1 - 0.9f is 2.4e-8 away from 1 - 0.9)
    const float alpha = (float)alphad, w2 = (float)(1.0 - alphad);
#endif
#if IRIS_K_EMA
    // the weight of k_agc_clip_adam_ema, from the counter the caller names: neither update has a bias correction, so only the
    // EMA siblings read one
    const double t = (double)step_dev[0];
    const double warm = (1.0 + t) / (10.0 + t);
    const float we = (float)(1.0 - (decay < warm ? decay : warm));
#endif
    for (size_t r = wave; r < n_rows; r += n_waves) {
        float* const p = rows[r].param;
        float* const g = rows[r].grad;
        float* const b = rows[r].exp_avg;       // momentum_buffer
        const long len = rows[r].len;
        uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(b);
#if IRIS_K_RMS
        float* const q = rows[r].exp_avg_sq;    // square_avg
        bits |= reinterpret_cast<uintptr_t>(q);
#endif
#if IRIS_K_EMA
        float* const e = rows[r].ema;
        bits |= reinterpret_cast<uintptr_t>(e);
#endif
        const bool vec = ((len & 3) == 0) && ((bits & 15) == 0);
        float scale = 1.0f;
        if (use_agc) {   // the unit's two norms (k_agc_clip's first pass, as k_agc_clip_adam has it)
            float sp = 0.f, sg = 0.f;
            if (vec) {
                for (long i = 4 * lane; i < len; i += 4 * kWave) {
                    const float4 a = *reinterpret_cast<const float4*>(p + i);
                    const float4 c = *reinterpret_cast<const float4*>(g + i);
                    sp += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
                    sg += c.x * c.x + c.y * c.y + c.z * c.z + c.w * c.w;
                }
            } else {
                for (long i = lane; i < len; i += kWave) {
                    sp += p[i] * p[i];
                    sg += g[i] * g[i];
                }
            }
            const float p_norm = sqrtf(wave_sum(sp)), g_norm = sqrtf(wave_sum(sg));
            // (a NaN norm stays NaN through both floors: see k_agc_adam_kernel.h)
            const float max_norm = (p_norm < eps_agc ? eps_agc : p_norm) * clip_factor;
            scale = g_norm < max_norm ? 1.0f : max_norm / (g_norm < 1e-6f ? 1e-6f : g_norm);
        }
#if IRIS_K_RMS
        auto one = [&](float& pp, float& gg, float& bb, float& ss) {
            float x = scale == 1.0f ? gg : gg * scale;
            if (clamp) x = clamp_keep_nan(x, clipvalue);
            gg = x;
            ss = alpha * ss + w2 * x * x;
            bb = mu * bb + x / (sqrtf(ss) + eps);
            pp -= lr * bb;
        };
#else
        auto one = [&](float& pp, float& gg, float& bb) {
            // (scale == 1 leaves the gradient's bits alone, as k_agc_clip does by skipping the unit)
            float x = scale == 1.0f ? gg : gg * scale;
            if (clamp) x = clamp_keep_nan(x, clipvalue);
            gg = x;
            bb = mu * bb + x;
            pp -= lr * bb;
        };
#endif
#if IRIS_K_EMA
        auto avg = [&](float& ee, float pp) { ee = ee + (pp - ee) * we; };
#endif
        if (vec) {
            for (long i = 4 * lane; i < len; i += 4 * kWave) {
                float4 a = *reinterpret_cast<float4*>(p + i), c = *reinterpret_cast<float4*>(g + i);
                float4 d = *reinterpret_cast<float4*>(b + i);
#if IRIS_K_RMS
                float4 s = *reinterpret_cast<float4*>(q + i);
                one(a.x, c.x, d.x, s.x);
                one(a.y, c.y, d.y, s.y);
                one(a.z, c.z, d.z, s.z);
                one(a.w, c.w, d.w, s.w);
                *reinterpret_cast<float4*>(q + i) = s;
#else
                one(a.x, c.x, d.x);
                one(a.y, c.y, d.y);
                one(a.z, c.z, d.z);
                one(a.w, c.w, d.w);
#endif
                *reinterpret_cast<float4*>(p + i) = a;
                *reinterpret_cast<float4*>(g + i) = c;
                *reinterpret_cast<float4*>(b + i) = d;
#if IRIS_K_EMA
                float4 f = *reinterpret_cast<float4*>(e + i);
                avg(f.x, a.x);
                avg(f.y, a.y);
                avg(f.z, a.z);
                avg(f.w, a.w);
                *reinterpret_cast<float4*>(e + i) = f;
#endif
            }
        } else {
            for (long i = lane; i < len; i += kWave) {
                float pp = p[i];
#if IRIS_K_RMS
                one(pp, g[i], b[i], q[i]);
#else
                one(pp, g[i], b[i]);
#endif
                p[i] = pp;
#if IRIS_K_EMA
                avg(e[i], pp);
#endif
            }
        }
    }
}
#undef IRIS_K_ROW
