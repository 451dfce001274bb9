// k_agc_adam_kernel.h -- the text of the AGC + clipvalue + Adam launch (see k_agc_adam.h, which includes this file TWICE, like
// k_fused_kernel.h): with IRIS_K_EMA 0 it is k_agc_clip_adam as it always was; 1 = its sibling k_agc_clip_adam_ema, which carries the
// updated parameter - still in its register - on into an exponential moving average of the weights (one more row pointer, one more
// read and one more write per element).  No include guard on purpose.
#if IRIS_K_EMA
__global__ __launch_bounds__(256) void k_agc_clip_adam_ema(const iris_agc_adam_ema_row* rows, size_t n_rows, float clip_factor, float eps_agc,
                                                           float clipvalue, int use_agc, const float* lr_dev, float lr_host, double beta1d,
                                                           double beta2d, float eps, const float* step_dev, double decay) {
#else
__global__ __launch_bounds__(256) void k_agc_clip_adam(const iris_agc_adam_row* rows, size_t n_rows, float clip_factor, float eps_agc,
                                                       float clipvalue, int use_agc, const float* lr_dev, float lr_host, double beta1d,
                                                       double beta2d, float eps, const float* step_dev) {
#endif
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * 4;
    const double t = (double)step_dev[0];
    // (the betas stay doubles up to here, as in ATen: 1 - 0.999f is 1.3e-5 away from 1 - 0.999)
    const float bc1 = (float)(1.0 - pow(beta1d, t)), bc2_sqrt = sqrtf((float)(1.0 - pow(beta2d, t)));
    const float lr = lr_dev ? lr_dev[0] : lr_host;
    const float step_size = lr / bc1, w1 = (float)(1.0 - beta1d), w2 = (float)(1.0 - beta2d), beta2 = (float)beta2d;
    const bool clamp = clipvalue > 0.f;
#if IRIS_K_EMA
    // TensorFlow's ExponentialMovingAverage(num_updates) warm-up from the counter the bias corrections read: a replayed graph sees
    // every step's weight with nothing to re-record
    const double warm = (1.0 + t) / (10.0 + t);
    const float we = (float)(1.0 - (decay < warm ? decay : warm));
#endif
    for (size_t r = wave; r < n_rows; r += n_waves) {
        float* const p = rows[r].param;
        float* const g = rows[r].grad;
        float* const m = rows[r].exp_avg;
        float* const v = rows[r].exp_avg_sq;
        const long len = rows[r].len;
#if IRIS_K_EMA
        float* const e = rows[r].ema;
        const bool vec = ((len & 3) == 0) && (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                                                reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(e)) & 15) == 0);
#else
        const bool vec = ((len & 3) == 0) && (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                                                reinterpret_cast<uintptr_t>(v)) & 15) == 0);
#endif
        float scale = 1.0f;
        if (use_agc) {   // the unit's two norms (k_agc_clip's first pass)
            float sp = 0.f, sg = 0.f;
            if (vec) {
                for (long i = 4 * lane; i < len; i += 4 * kWave) {
                    const float4 a = *reinterpret_cast<const float4*>(p + i);
                    const float4 b = *reinterpret_cast<const float4*>(g + i);
                    sp += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
                    sg += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
                }
            } else {
                for (long i = lane; i < len; i += kWave) {
                    sp += p[i] * p[i];
                    sg += g[i] * g[i];
                }
            }
            const float p_norm = sqrtf(wave_sum(sp)), g_norm = sqrtf(wave_sum(sg));
            // (a NaN norm stays NaN through both floors, as in torch.clamp / tf.maximum: fmaxf would drop it and hand a unit with one
            // NaN gradient a factor of max_norm / 1e-6 for its other elements)
            const float max_norm = (p_norm < eps_agc ? eps_agc : p_norm) * clip_factor;
            scale = g_norm < max_norm ? 1.0f : max_norm / (g_norm < 1e-6f ? 1e-6f : g_norm);
        }
        auto one = [&](float& pp, float& gg, float& mm, float& vv) {
            // (scale == 1 leaves the gradient's bits alone, as k_agc_clip does by skipping the unit)
            float x = scale == 1.0f ? gg : gg * scale;
            if (clamp) x = clamp_keep_nan(x, clipvalue);
            gg = x;
            mm = mm + (x - mm) * w1;
            vv = beta2 * vv + w2 * x * x;
            const float denom = sqrtf(vv) / bc2_sqrt + eps;
            pp -= step_size * mm / denom;
        };
#if IRIS_K_EMA
        // e' = e + (p' - e) w, the form of the first moment: a NaN parameter goes into its average (the parameter is lost anyway)
        auto avg = [&](float& ee, float pp) { ee = ee + (pp - ee) * we; };
#endif
        if (vec) {
            for (long i = 4 * lane; i < len; i += 4 * kWave) {
                float4 a = *reinterpret_cast<float4*>(p + i), b = *reinterpret_cast<float4*>(g + i);
                float4 c = *reinterpret_cast<float4*>(m + i), d = *reinterpret_cast<float4*>(v + i);
                one(a.x, b.x, c.x, d.x);
                one(a.y, b.y, c.y, d.y);
                one(a.z, b.z, c.z, d.z);
                one(a.w, b.w, c.w, d.w);
                *reinterpret_cast<float4*>(p + i) = a;
                *reinterpret_cast<float4*>(g + i) = b;
                *reinterpret_cast<float4*>(m + i) = c;
                *reinterpret_cast<float4*>(v + i) = d;
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
#if IRIS_K_EMA
            for (long i = lane; i < len; i += kWave) {
                float pp = p[i];
                one(pp, g[i], m[i], v[i]);
                p[i] = pp;
                avg(e[i], pp);
            }
#else
            for (long i = lane; i < len; i += kWave) one(p[i], g[i], m[i], v[i]);
#endif
        }
    }
}
