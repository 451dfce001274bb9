// k_metrics.h -- the reference's training metrics (metrics.py:217-299: er_score, cos_sim, f1_score) for one batch in ONE launch.
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// er_score is built from tf.where / argsort, whose shapes depend on the data; restated without event lists:
//   * one workgroup per clip, one wave per class (a loop over classes when K > 4 waves);
//   * __ballot turns 64 frames at a time into bit words of yt = y_true >= thr and yp = y_pred >= thr (NaN: 0), kept in LDS;
//   * run starts / ends are word operations (x & ~(x << 1 | carry)); each predicted run [s, e] sets bit (s + e) / 2 of an LDS
//     bitmap of T bits (ds_or_b64: the order of the ORs does not matter);
//   * a true run [ts, te] is correct iff the bitmap has a bit in [ts, te] - the reference's "same clip, same class,
//     ts <= middle <= te, reduce_max over the predictions";
//   * er = (n_true + n_pred - 2 correct) / max(n_true, 1) in fp32 from integer counts.
// smoothing=True: AveragePooling1D(pool, padding='same') with stride = pool (Keras' default) on the predictions first; the
// pooled middles are then compared, as indices, with full-rate label frames (the reference does so).
// cos_sim and the F1 counts ride along in the same pass over the labels when the predictions are at label rate.
// Cross-clip sums (cumulative F1 counts, epoch accumulator): per-clip slab in fp64 + last-arriving-block ticket with agent-scope
// release / acquire; the reducer adds in a fixed order, so every output is bitwise reproducible.  No float atomics.
// ---------------------------------------------------------------------------

constexpr int kMetWaves = 4;
constexpr int kMetMaxT = 8192;
constexpr int kMetWords = kMetMaxT / 64;
constexpr int kMetMaxK = 16;

struct MetLds {
    uint64_t yt[kMetWaves][kMetWords];
    uint64_t yp[kMetWaves][kMetWords];
    uint64_t mid[kMetWaves][kMetWords];
    double f1[kMetMaxK][3];
    float cs[kMetMaxK];
    float msk[kMetMaxK];
    int cnt[kMetMaxK][3];   // n_true, n_pred, correct
    int last;
};

// bit t: x[t] && !x[t-1]  /  x[t] && !x[t+1]   (0-padding on both sides of the sequence)
__device__ __forceinline__ uint64_t met_starts(const uint64_t* w, int j) {
    const uint64_t cur = w[j], prev = j > 0 ? w[j - 1] : 0ull;
    return cur & ~((cur << 1) | (prev >> 63));
}
__device__ __forceinline__ uint64_t met_ends(const uint64_t* w, int j, int nw) {
    const uint64_t cur = w[j], next = j + 1 < nw ? w[j + 1] : 0ull;
    return cur & ~((cur >> 1) | (next << 63));
}
// last frame of the run that starts at frame s
__device__ __forceinline__ int met_run_end(const uint64_t* w, int s, int nw) {
    int j = s >> 6;
    uint64_t e = met_ends(w, j, nw) & (~0ull << (s & 63));
    while (e == 0ull && j + 1 < nw) e = met_ends(w, ++j, nw);   // (a run always ends by the last word: bits past T are 0)
    return (j << 6) + __builtin_ctzll(e);
}
// any bit of m in [a, b]
__device__ __forceinline__ bool met_any(const uint64_t* m, int a, int b) {
    const int ja = a >> 6, jb = b >> 6;
    for (int j = ja; j <= jb; ++j) {
        uint64_t w = m[j];
        if (j == ja) w &= ~0ull << (a & 63);
        if (j == jb) w &= ~0ull >> (63 - (b & 63));
        if (w) return true;
    }
    return false;
}
__device__ __forceinline__ double met_wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_event_metrics(const float* __restrict__ y_true, const float* __restrict__ y_pred, int B, int T,
                                                       int Tp, int K, float thr, int pool, int Tpe, int pad0, float f1_thr,
                                                       float* __restrict__ er_out, float* __restrict__ cos_out,
                                                       double* __restrict__ f1_state, float* __restrict__ f1_out,
                                                       double* __restrict__ accum, double* __restrict__ slab, unsigned* ticket) {
    __shared__ MetLds L;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int nwT = (T + 63) >> 6, nwP = (Tpe + 63) >> 6;
    const bool rate = Tp == T;   // cos_sim / F1: predictions at label rate
    const float* yt = y_true + (size_t)b * T * K;
    const float* yp = y_pred + (size_t)b * Tp * K;
    uint64_t* const wt = L.yt[wv];
    uint64_t* const wp = L.yp[wv];
    uint64_t* const wm = L.mid[wv];
    for (int k0 = 0; k0 < K; k0 += nwv) {   // (uniform trip count: the barriers below are reached by every wave)
        const int k = k0 + wv;
        const bool act = k < K;
        if (act) {
            double tp = 0.0, fp = 0.0, fn = 0.0;
            float sy = 0.f, sp = 0.f, dot = 0.f, ysum = 0.f;
            for (int c = 0; c < nwT; ++c) {
                const int t = c * 64 + lane;
                float y = 0.f, p = 0.f;
                if (t < T) {
                    y = yt[(size_t)t * K + k];
                    if (rate) p = yp[(size_t)t * K + k];
                }
                const uint64_t bits = __ballot(t < T && y >= thr);
                if (lane == 0) {
                    wt[c] = bits;
                    wm[c] = 0ull;
                }
                if (rate && t < T) {
                    const double pb = p > f1_thr ? 1.0 : 0.0, yd = (double)y;   // tfa F1Score: strict >, raw labels
                    tp += pb * yd;
                    fp += pb * (1.0 - yd);
                    fn += (1.0 - pb) * yd;
                    sy += y * y;
                    sp += p * p;
                    dot += y * p;
                    ysum += y;
                }
            }
            for (int c = 0; c < nwP; ++c) {
                const int i = c * 64 + lane;
                bool on = false;
                if (i < Tpe) {
                    float v;
                    if (pool > 1) {   // the window's mean over its in-range frames, summed in frame order
                        const int lo = max(i * pool - pad0, 0), hi = min(i * pool - pad0 + pool, Tp);
                        float acc = 0.f;
                        for (int t = lo; t < hi; ++t) acc += yp[(size_t)t * K + k];
                        v = acc / (float)(hi - lo);
                    } else {
                        v = yp[(size_t)i * K + k];
                    }
                    on = v >= thr;
                }
                const uint64_t bits = __ballot(on);
                if (lane == 0) wp[c] = bits;
            }
            tp = met_wave_sum_f64(tp);
            fp = met_wave_sum_f64(fp);
            fn = met_wave_sum_f64(fn);
            sy = wave_sum(sy);
            sp = wave_sum(sp);
            dot = wave_sum(dot);
            ysum = wave_sum(ysum);
            if (lane == 0) {
                L.f1[k][0] = tp;
                L.f1[k][1] = fp;
                L.f1[k][2] = fn;
                // Keras cosine_similarity over time of l2_normalize'd operands (rsqrt(max(sum x^2, 1e-12))), negated
                L.cs[k] = -(dot * (1.0f / sqrtf(fmaxf(sy, 1e-12f))) * (1.0f / sqrtf(fmaxf(sp, 1e-12f))));
                L.msk[k] = ysum > 0.f ? 1.f : 0.f;
            }
        }
        __syncthreads();
        if (act) {   // predicted runs -> middles
            int n_pred = 0;
            for (int j = lane; j < nwP; j += 64) {
                uint64_t s = met_starts(wp, j);
                n_pred += __popcll(s);
                while (s) {
                    const int st = (j << 6) + __builtin_ctzll(s);
                    s &= s - 1;
                    const int m = (st + met_run_end(wp, st, nwP)) >> 1;
                    if (m < T) atomicOr(reinterpret_cast<unsigned long long*>(&wm[m >> 6]), 1ull << (m & 63));
                }
            }
            for (int o = 32; o > 0; o >>= 1) n_pred += __shfl_xor(n_pred, o, 64);
            if (lane == 0) L.cnt[k][1] = n_pred;
        }
        __syncthreads();
        if (act) {   // true runs: correct iff a middle lies inside
            int n_true = 0, correct = 0;
            for (int j = lane; j < nwT; j += 64) {
                uint64_t s = met_starts(wt, j);
                n_true += __popcll(s);
                while (s) {
                    const int st = (j << 6) + __builtin_ctzll(s);
                    s &= s - 1;
                    correct += met_any(wm, st, met_run_end(wt, st, nwT)) ? 1 : 0;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                n_true += __shfl_xor(n_true, o, 64);
                correct += __shfl_xor(correct, o, 64);
            }
            if (lane == 0) {
                L.cnt[k][0] = n_true;
                L.cnt[k][2] = correct;
            }
        }
        __syncthreads();
    }
    const bool reduce = f1_state != nullptr || accum != nullptr;
    if (threadIdx.x == 0) {   // the clip, classes in order
        int nt = 0, np = 0, cr = 0;
        float msum = 0.f;
        double c3[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) {
            nt += L.cnt[k][0];
            np += L.cnt[k][1];
            cr += L.cnt[k][2];
            msum += L.msk[k];
            for (int q = 0; q < 3; ++q) c3[q] += L.f1[k][q];
        }
        const float ntf = (float)nt;
        er_out[b] = (ntf + (float)np - 2.f * (float)cr) / fmaxf(ntf, 1.f);
        if (cos_out) {
            float cs = 0.f;
            for (int k = 0; k < K; ++k) cs += L.cs[k] * (L.msk[k] / fmaxf(msum, 1e-8f));   // utils.safe_div
            cos_out[b] = cs;
        }
        if (reduce) {
            for (int q = 0; q < 3; ++q) slab[(size_t)b * 3 + q] = c3[q];
            // publish (er, cos, slab) and draw the ticket: agent-scope release, then the counter (cdna_hip_programming §6 G16)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            L.last = prev == (unsigned)(B - 1);
            if (L.last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
    }
    if (!reduce) return;
    __syncthreads();
    if (!L.last || wv != 0) return;
    // last arriver, wave 0: every clip's slab in a fixed order (lane-strided, then a fixed butterfly)
    double tp = 0.0, fp = 0.0, fn = 0.0, ser = 0.0, scs = 0.0;
    for (int i = lane; i < B; i += 64) {
        tp += slab[(size_t)i * 3 + 0];
        fp += slab[(size_t)i * 3 + 1];
        fn += slab[(size_t)i * 3 + 2];
        ser += (double)er_out[i];
        if (cos_out) scs += (double)cos_out[i];
    }
    tp = met_wave_sum_f64(tp);
    fp = met_wave_sum_f64(fp);
    fn = met_wave_sum_f64(fn);
    ser = met_wave_sum_f64(ser);
    scs = met_wave_sum_f64(scs);
    if (lane == 0) {
        float f1 = 0.f;
        if (f1_state) {   // cumulative counts (the reference never resets its F1Score); micro F1 with div-no-nan
            const double ctp = f1_state[0] + tp, cfp = f1_state[1] + fp, cfn = f1_state[2] + fn;
            f1_state[0] = ctp;
            f1_state[1] = cfp;
            f1_state[2] = cfn;
            const double prec = (ctp + cfp) != 0.0 ? ctp / (ctp + cfp) : 0.0;
            const double rec = (ctp + cfn) != 0.0 ? ctp / (ctp + cfn) : 0.0;
            const double pr = prec * rec, ps = prec + rec;
            f1 = (float)((ps != 0.0 ? pr / ps : 0.0) * 2.0);
            f1_out[0] = f1;
        }
        if (accum) {
            accum[0] += ser;
            accum[1] += scs;
            accum[2] += (double)f1;
            accum[3] += (double)B;
            accum[4] += 1.0;
        }
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch / replay
    }
}

extern "C" int iris_event_metrics(const float* y_true, const float* y_pred, int batch, int n_time, int n_time_pred, int n_classes,
                                  float threshold, int pool, float f1_threshold, float* er_out, float* cos_out, double* f1_state,
                                  float* f1_out, double* accum, double* slab, unsigned* ticket, void* stream) {
    if (!y_true || !y_pred || !er_out) return fail(IRIS_E_INVALID, "iris_event_metrics: NULL y_true / y_pred / er_out");
    if ((f1_state == nullptr) != (f1_out == nullptr))
        return fail(IRIS_E_INVALID, "iris_event_metrics: f1_state and f1_out go together");
    if ((f1_state || accum) && (!slab || !ticket))
        return fail(IRIS_E_INVALID, "iris_event_metrics: the F1 state / accumulator need the slab and the ticket");
    if (batch < 1 || n_classes < 1 || n_time < 1 || n_time_pred < 1 || pool < 0)
        return fail(IRIS_E_INVALID, "iris_event_metrics: batch %d, T %d, T' %d, K %d, pool %d", batch, n_time, n_time_pred,
                    n_classes, pool);
    if (n_classes > kMetMaxK || n_time > kMetMaxT || n_time_pred > kMetMaxT || pool > kMetMaxT)
        return fail(IRIS_E_UNSUPPORTED, "iris_event_metrics: K %d (<= %d), T %d, T' %d (<= %d), pool %d", n_classes, kMetMaxK,
                    n_time, n_time_pred, kMetMaxT, pool);
    if ((cos_out || f1_state) && n_time_pred != n_time)
        return fail(IRIS_E_INVALID, "iris_event_metrics: cos_sim / F1 need the predictions at label rate (T' %d != T %d)",
                    n_time_pred, n_time);
    const int p = pool > 1 ? pool : 1;
    const int tpe = (n_time_pred + p - 1) / p;   // Keras 'same' pooling with stride = pool: ceil(T' / pool) windows,
    const int pad0 = (tpe * p - n_time_pred) / 2;  // the padding split floor / ceil before / after
    const int waves = std::min(n_classes, kMetWaves);
    k_event_metrics<<<batch, 64 * waves, 0, (hipStream_t)stream>>>(y_true, y_pred, batch, n_time, n_time_pred, n_classes, threshold,
                                                                  p, tpe, pad0, f1_threshold, er_out, cos_out, f1_state, f1_out,
                                                                  accum, slab, ticket);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
