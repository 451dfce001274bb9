// decode_core.h -- the event decoder's arithmetic, written once: k_detect.h (one setting) and k_tune.h (a grid of settings)
// call these pieces and restate none of them, so a setting the sweep scores is decoded exactly as detection decodes it.
// Part of the single translation unit iris_frontend.hip (before k_detect.h).
#pragma once
// ---------------------------------------------------------------------------
// The arithmetic (include/iris_frontend.h, iris_decode_events; challenge_amd/detect.py restates it on the CPU bit for bit).
// For file f, class k, frame t < T_f:
//   1. p[t] = (fp32 sum, from 0, over the windows w with w*hop <= t < w*hop + n_frame in ascending w of
//      preds[win_off[f] + w, (t - w*hop) / up, k]) / (float)count                      overlap-add average
//   2. a[t] = (fp32 sum, from 0, of p[u] for u in [t - al, t + ar] ∩ [0, T_f) ascending) / (float)n       AveragePooling1D 'same'
//   3. d[t] = some u in [t - ml, t + mr] ∩ [0, T_f) has a[u] >= thr, and none of them is NaN     MaxPooling1D 'same', >= thr
//   4. events = the maximal runs of d as (first, last) frames                          get_start_end_frame
// ---------------------------------------------------------------------------

// 'same' pads of a pool of `pool` frames: l before the frame, r after it
struct DecPad { int l, r; };
__host__ __device__ __forceinline__ DecPad dec_pad(int pool) {
    const int l = (pool - 1) / 2;
    return {l, pool - 1 - l};
}

// 64-frame bit words of t frames, and the event capacity of one (file, class); long long on the host, which sums them over the
// files to refuse what does not fit an int before the device computes them as int
template <typename I>
__host__ __device__ __forceinline__ I dec_words(I t) { return (t + 63) >> 6; }
template <typename I>
__host__ __device__ __forceinline__ I dec_pairs(I t) { return (t + 1) / 2 + 1; }

// step 1: p[v] of class k, 0 <= v < T_f, for the file whose W windows start at row w0 of preds
__device__ __forceinline__ float dec_overlap_avg(const float* __restrict__ preds, int w0, int W, int n_frame, int hop, int n_out,
                                                 int up, int K, int v, int k) {
    const int w_hi = min(v / hop, W - 1);
    const int w_lo = v >= n_frame ? (v - n_frame) / hop + 1 : 0;
    float s = 0.f;
    for (int w = w_lo; w <= w_hi; ++w) s += preds[((size_t)(w0 + w) * n_out + (v - w * hop) / up) * K + k];
    return s / (float)(w_hi - w_lo + 1);
}

// step 2: a[u], 0 <= u < T, from an array that holds p of frame v at p[base + v]
__device__ __forceinline__ float dec_smooth(const float* p, int base, int u, DecPad avg, int T) {
    const int lo = max(u - avg.l, 0), hi = min(u + avg.r, T - 1);
    float s = 0.f;
    for (int v = lo; v <= hi; ++v) s += p[base + v];
    return s / (float)(hi - lo + 1);
}
__device__ __forceinline__ bool dec_is_on(float a, float thr) { return a >= thr; }
__device__ __forceinline__ bool dec_is_nan(float a) { return a != a; }

// any bit of w[] in [lo, hi] (lo <= hi, indices into the word array)
__device__ __forceinline__ bool dec_any(const uint64_t* w, int lo, int hi) {
    const int ja = lo >> 6, jb = hi >> 6;
    uint64_t acc = 0ull;
    for (int j = ja; j <= jb; ++j) {
        uint64_t x = w[j];
        if (j == ja) x &= ~0ull << (lo & 63);
        if (j == jb) x &= ~0ull >> (63 - (hi & 63));
        acc |= x;
    }
    return acc != 0ull;
}
// step 3: d of the frame whose max-pool window is bits [lo, hi] of the "a >= thr" and "a is NaN" words
__device__ __forceinline__ bool dec_dilate(const uint64_t* on, const uint64_t* nan, int lo, int hi) {
    return dec_any(on, lo, hi) && !dec_any(nan, lo, hi);
}

// step 4: the first / last frames of the runs in word `cur` of d, given bit 63 of the word before (0 or 1) and the word after
// (of which bit 0 counts)
__device__ __forceinline__ uint64_t dec_run_starts(uint64_t cur, uint64_t prev_top) { return cur & ~((cur << 1) | prev_top); }
__device__ __forceinline__ uint64_t dec_run_ends(uint64_t cur, uint64_t next) { return cur & ~((cur >> 1) | (next << 63)); }

__device__ __forceinline__ int dec_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int dec_wave_incl_scan(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}
