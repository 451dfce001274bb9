// k_ipd.h -- stereo complex spectrum -> mel-band inter-channel phase difference (cos, sin).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K3p: spectrum [B, F, T, 4] = (re0, re1, im0, im1) -> ipd [B, M, T, 2] = (cos, sin), the magnitude-weighted band average
//   per bin k:  re_k = re0 re1 + im0 im1,  im_k = im0 re1 - re0 im1   (X0 conj X1: phase = phi0 - phi1)
//               a_k  = sqrt((re0^2 + im0^2)(re1^2 + im1^2))           (= |X0| |X1|)
//   per band m: den = sum_k W[k,m] a_k,  cos = sum_k W[k,m] re_k / (den + eps),  sin = sum_k W[k,m] im_k / (den + eps)
//   block = 64 consecutive frames x (4 or 8) waves over the mel bands, as K3 (k_magmel): one thread per frame, one 16-byte
//   load per lane and bin (1 KiB per wave, coalesced along t), three fp32 accumulators per open band.  Any plan mel matrix:
//   the band's bin range comes from band_lo / band_len, the weights from the dense [F][M] table (uniform loads).  Under a
//   triangular filterbank a bin feeds two bands: its second read comes from L1 / L2.  No LDS, no atomics, a fixed summation
//   order: the same inputs give the same bits.  sqrt and the two divisions are the IEEE ones (the build has no fast-math).
// ---------------------------------------------------------------------------
constexpr float kIpdEps = 1e-20f;

struct IpdArgs {
    const float* spec;  // [B, F, T, 4], 16-byte aligned
    float* out;         // [B, M, T, 2], 8-byte aligned
    const float* w;     // dense [F][M]
    const int* band_lo;
    const int* band_len;
    const int* t_bands;
    int n_tb;
    const int* f_bands;
    int n_fb;
    int B, F, T, M;
};

// im0 re1 - re0 im1 as two rounded products and one subtraction (no contraction into an FMA): swapping the channels then
// negates the value EXACTLY, so sin flips its sign bit for bit; the error is still within 2 u a_k.
__device__ __forceinline__ float ipd_cross_im(float re0, float re1, float im0, float im1) {
#pragma clang fp contract(off)
    const float p = im0 * re1, q = re0 * im1;
    return p - q;
}

__global__ __launch_bounds__(512) void k_spec_ipd(const IpdArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    typedef float vec2 __attribute__((ext_vector_type(2)));
    constexpr int U = 8;  // bins in flight per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 64 + lane;
    const bool valid = t < a.T;  // tail frames: no load, no store
    const int* tb = a.t_bands ? a.t_bands + (size_t)b * a.n_tb * 2 : nullptr;
    const int* fb = a.f_bands ? a.f_bands + (size_t)b * a.n_fb * 2 : nullptr;
    const bool live = valid && !(tb && in_bands(tb, a.n_tb, t));  // a masked frame reads nothing: its sums stay 0 -> (0, 0)
    const vec4* sp = reinterpret_cast<const vec4*>(a.spec) + (size_t)b * a.F * a.T + (valid ? t : 0);
    vec2* out = reinterpret_cast<vec2*>(a.out) + (size_t)b * a.M * a.T + (valid ? t : 0);
    for (int m = wave; m < a.M; m += nw) {
        const int lo = a.band_lo[m], len = a.band_len[m];  // uniform
        float s_re = 0.f, s_im = 0.f, s_a = 0.f;
        for (int i0 = 0; i0 < len; i0 += U) {
            vec4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int f = lo + min(i0 + u, len - 1);
                v[u] = live ? sp[(size_t)f * a.T] : vec4(0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int f = lo + i0 + u;
                if (i0 + u >= len) break;
                if (fb && in_bands(fb, a.n_fb, f)) continue;  // uniform: a masked bin contributes nothing
                const float w = a.w[(size_t)f * a.M + m];
                const float re0 = v[u][0], re1 = v[u][1], im0 = v[u][2], im1 = v[u][3];
                const float re = fmaf(im0, im1, re0 * re1);
                const float im = ipd_cross_im(re0, re1, im0, im1);
                const float mag = sqrtf(fmaf(re0, re0, im0 * im0) * fmaf(re1, re1, im1 * im1));
                s_re = fmaf(w, re, s_re);
                s_im = fmaf(w, im, s_im);
                s_a = fmaf(w, mag, s_a);
            }
        }
        const float den = s_a + kIpdEps;
        const vec2 cs = {s_re / den, s_im / den};
        if (valid) out[(size_t)m * a.T] = cs;
    }
}
