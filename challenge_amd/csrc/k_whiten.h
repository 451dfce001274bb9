// k_whiten.h -- stereo complex spectrum -> spatially whitened mel-band energy (two-microphone noise nulling).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K3w: spectrum [B, F, T, 4] = (re0, re1, im0, im1) -> e [B, M, T], x^H (R + d I)^-1 x summed over the mel bands, with R the
// 2x2 inter-channel covariance of a block of frames.  Frames are grouped into J = ceil(T / block) consecutive blocks from
// frame 0 (the last one may be shorter).  Two launches, no atomics, fixed summation orders: the same inputs give the same
// bits, and a sample's values do not depend on the batch it sits in.
//
//   1. k_whiten_factors: per (sample, bin, block), over the block's n frames (unmasked)
//        r00 = mean |X0|^2,  r11 = mean |X1|^2,  r10 = mean X1 conj(X0),  d = loading (r00 + r11) / 2
//        d == 0 (a silent block): a = b = c = 0
//        else l00 = sqrt(r00 + d),  l10 = r10 / l00,  l11 = sqrt(r11 + d - |l10|^2),  a = 1 / l00,  b = 1 / l11,  c = l10 / l00
//      written as (a, b, Re c, Im c) fp32 into [B, F, J, 4].  A group of G lanes owns one block, G = a quarter of the power
//      of two >= block, between 1 and 64 - a function of `block` alone, so a block's summation order depends on neither T
//      nor the batch - and a wave owns 64 / G consecutive blocks of one bin: 16-byte loads coalesced along t (lane l of a
//      group reads the block's frames l, l + G, ...: four in flight), the fp32 inputs converted to double BEFORE squaring,
//      four double sums per lane in frame order, a fixed xor tree over the group, the factorisation in double on the group's
//      lane 0 (a few values per row; in fp32 the cancellation in l11^2 would bring 1 / loading into the error) as
//      a = 1 / sqrt(r00 + d), c = r10 a^2, b = 1 / sqrt(r11 + d - |r10|^2 a^2): two square roots and two divisions.  The
//      only fp32 roundings are the four final conversions.
//   2. k_spec_whiten: one thread per frame, 4 waves over the mel bands, as K3p (k_ipd.h): per bin one 16-byte load of the
//      spectrum and one of the frame's block factors (lanes of one block share the address; a 64-frame tile straddles two
//      blocks when `block` is not a multiple of 64), then
//        z0 = a X0,  z1 = b (X1 - c X0),  q = |z0|^2 + |z1|^2,   e[m, t] = wnorm[m] sum_k W[k, m] q[k, t]
//      wnorm[m] = 1 / (2 sum_k W[k, m]) from the plan's table (built in double on the host, 0 for an all-zero band), and
//      ln(e + 1e-8) behind a flag.  SpecAugment bands act on the OUTPUT only - a frame in a time band gives e = 0, a bin in a
//      frequency band adds nothing to the sum - while the covariance and wnorm never see them (zeroing the spectrum first,
//      as K3p does, would change R).
//   fp32 roundings of pass 2, in units of u = 2^-24 of A = wnorm sum_k W (|z0|^2 + ((|X1| + |c| |X0|) b)^2):
//      |z0|^2: a stored in fp32 (2) + the products a re0, a im0 (2);  y = X1 - c X0: c stored in fp32 (1) + two fmas per
//      component (2), all relative to |X1| + |c| |X0|;  z1 = b y: b stored in fp32 (1) + the product (1) -> (3 + 2) 2 = 10 on
//      |z1|^2;  the sum of the four squares: one product + three fmas (4)  ->  14 per bin;  the band sum: one fma per bin
//      (n_m);  wnorm stored in fp32 (1) and the final product (1)  ->  (n_m + 16) u A.
//
// K18: k_whiten_factors<true>, the factors of a block from the frames OUTSIDE the detected events (iris_spec_whiten_factors_ranges).
//   A host-built table names, per (sample, block), the frames [t0, t1) behind the block's covariance - the block itself or the
//   block and up to `reach` neighbours a side, at most (2 reach + 1) block frames - and whether the byte mask [B, T] (non-zero:
//   the frame is inside an event) applies.  The same text as pass 1 (a template flag): the same G lanes per (row, block), G a
//   function of `block` alone, lane l taking the frames t0 + l, t0 + l + G, ... of the RANGE in frame order; the mask byte is
//   loaded first and a masked frame's 16 bytes are never loaded (four frames a step: the four bytes in flight together, then
//   the 16-byte loads of the frames that count, then the sums - a byte load followed by its dependent 16-byte load, frame
//   after frame, left one load in flight and measured 1.43 x pass 1 with an empty mask); four double sums and an integer
//   count per lane, the same xor tree, the mean = sum * (1 / count) and the factorisation in double on the group's lane 0.
//   count == 0: a = b = c = 0.
//   The same four fp32 roundings: a, b, |c| within 4 u of the float64 form.  use_mask == 0 over a block's own frames is pass 1,
//   bit for bit.  One launch, no workspace, no atomics; a row depends on its own sample's spectrum, mask and table rows only.
// ---------------------------------------------------------------------------
constexpr float kWhitenLogEps = 1e-8f;  // log_on_mel's epsilon

struct WhitenFactorArgs {
    const float* spec;  // [B, F, T, 4], 16-byte aligned
    float* fac;         // [B, F, J, 4], 16-byte aligned
    double loading;
    int B, F, T, J, block;
    int log2g;          // G = 1 << log2g lanes per block
    long long n_waves;  // B * F * ceil(J / (64 / G))
};

struct WhitenRangeArgs : WhitenFactorArgs {  // K18: the frames behind a block's covariance come from a table
    const unsigned char* mask;  // [B, T], non-zero: the frame is inside an event
    const int* ranges;          // [B, J, 3] = (t0, t1, use_mask): frames [t0, t1), without the masked ones when use_mask
};

struct WhitenArgs {
    const float* spec;  // [B, F, T, 4], 16-byte aligned
    const float* fac;   // [B, F, J, 4], 16-byte aligned
    float* out;         // [B, M, T]
    const float* w;     // dense [F][M]
    const float* wnorm; // [M]
    const int* band_lo;
    const int* band_len;
    const int* t_bands;
    int n_tb;
    const int* f_bands;
    int n_fb;
    int B, F, T, M, J, block, log;
};

// RANGES = false is K3w's pass 1; RANGES = true is K18 (the same text: the same lane mapping, sums, tree and factorisation)
template <bool RANGES>
__global__ __launch_bounds__(256) void k_whiten_factors(const std::conditional_t<RANGES, WhitenRangeArgs, WhitenFactorArgs> a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= a.n_waves) return;  // wave-uniform
    const int G = 1 << a.log2g, per_wave = 64 >> a.log2g;
    const int jw = (a.J + per_wave - 1) / per_wave;  // waves per (sample, bin) row
    const long long row = wave / jw;                 // b * F + f
    const int j = (int)(wave % jw) * per_wave + (lane >> a.log2g);
    const int l = lane & (G - 1);
    int t0, t1;
    [[maybe_unused]] const unsigned char* mk = nullptr;  // the sample's mask row
    [[maybe_unused]] bool use_mask = false;              // false: every frame of the range counts
    if constexpr (RANGES) {
        t0 = t1 = a.T;  // (a group past the last block reads nothing and writes nothing)
        if (j < a.J) {
            const int* r = a.ranges + ((row / a.F) * a.J + j) * 3;
            t0 = max(r[0], 0);
            t1 = min(r[1], a.T);  // (the host checked the table's host copy; the clamps keep a differing device copy in bounds)
            use_mask = r[2] != 0;
            mk = a.mask + (row / a.F) * a.T;
        }
    } else {
        t0 = j < a.J ? j * a.block : a.T;  // (a group past the last block reads nothing and writes nothing)
        t1 = min(t0 + a.block, a.T);
    }
    const vec4* sp = reinterpret_cast<const vec4*>(a.spec) + row * a.T;
    double s00 = 0., s11 = 0., sre = 0., sim = 0.;
    [[maybe_unused]] int cnt = 0;  // RANGES: the frames this lane summed
// one frame into the four sums (sre + i sim: X1 conj(X0)); the one text of both kernels
#define WHITEN_ADD_FRAME(v)                                              \
    {                                                                    \
        const double re0 = v[0], re1 = v[1], im0 = v[2], im1 = v[3];     \
        s00 += re0 * re0 + im0 * im0;                                    \
        s11 += re1 * re1 + im1 * im1;                                    \
        sre += re1 * re0 + im1 * im0;                                    \
        sim += im1 * re0 - re1 * im0;                                    \
    }
    if constexpr (RANGES) {
        // four frames a step, in three passes so that the loads of one pass are in flight together: the mask bytes first, then
        // the 16 bytes of the frames that count (a masked frame's are never loaded), then the sums in frame order
        constexpr int U = 4;
        for (int t = t0 + l; t < t1; t += U * G) {
            bool on[U];
            vec4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int tu = t + u * G;
                const unsigned char m = mk[min(tu, t1 - 1)];  // (unconditional, so that the four are in flight together: past
                on[u] = (tu < t1) & !(use_mask & (m != 0));    // the range the last byte again, dropped; unused when !use_mask)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = on[u] ? sp[t + u * G] : vec4(0.f);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!on[u]) continue;
                WHITEN_ADD_FRAME(v[u]);
                ++cnt;
            }
        }
    } else {
#pragma unroll 4  // (loads of four frames in flight; the sums keep their frame order)
        for (int t = t0 + l; t < t1; t += G) {
            const vec4 v = sp[t];
            WHITEN_ADD_FRAME(v);
        }
    }
#undef WHITEN_ADD_FRAME
    for (int off = G >> 1; off; off >>= 1) {  // the fixed tree: lanes of other groups never mix in (off < G)
        s00 += __shfl_xor(s00, off);
        s11 += __shfl_xor(s11, off);
        sre += __shfl_xor(sre, off);
        sim += __shfl_xor(sim, off);
        if constexpr (RANGES) cnt += __shfl_xor(cnt, off);
    }
    if (l != 0 || j >= a.J) return;
    int n = t1 - t0;
    if constexpr (RANGES) n = cnt;
    const double inv_n = 1.0 / (double)n;
    const double r00 = s00 * inv_n, r11 = s11 * inv_n, rre = sre * inv_n, rim = sim * inv_n;
    const double d = a.loading * (r00 + r11) * 0.5;
    vec4 o = {0.f, 0.f, 0.f, 0.f};
    if (d != 0. && (!RANGES || n > 0)) {  // (n == 0, a masked range without a quiet frame: NaN above; zero factors, as a silent block)
        const double fa = 1.0 / sqrt(r00 + d), fa2 = fa * fa;  // 1 / l00, 1 / l00^2
        const double l11sq = r11 + d - (rre * rre + rim * rim) * fa2;  // r11 + d - |l10|^2
        o[0] = (float)fa;
        o[1] = (float)(1.0 / sqrt(l11sq));
        o[2] = (float)(rre * fa2);  // l10 / l00 = r10 / l00^2
        o[3] = (float)(rim * fa2);
    }
    reinterpret_cast<vec4*>(a.fac)[row * a.J + j] = o;
}

__global__ __launch_bounds__(256) void k_spec_whiten(const WhitenArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    constexpr int U = 4;  // bins in flight per wave (two 16-byte loads each)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 64 + lane;
    const bool valid = t < a.T;  // tail frames: no load, no store
    const int* tb = a.t_bands ? a.t_bands + (size_t)b * a.n_tb * 2 : nullptr;
    const int* fb = a.f_bands ? a.f_bands + (size_t)b * a.n_fb * 2 : nullptr;
    const bool live = valid && !(tb && in_bands(tb, a.n_tb, t));  // a masked frame reads nothing: its sum stays 0
    const vec4* sp = reinterpret_cast<const vec4*>(a.spec) + (size_t)b * a.F * a.T + (valid ? t : 0);
    const vec4* fp = reinterpret_cast<const vec4*>(a.fac) + (size_t)b * a.F * a.J + (valid ? t / a.block : 0);
    float* out = a.out + (size_t)b * a.M * a.T + (valid ? t : 0);
    for (int m = wave; m < a.M; m += nw) {
        const int lo = a.band_lo[m], len = a.band_len[m];  // uniform
        float s = 0.f;
        for (int i0 = 0; i0 < len; i0 += U) {
            vec4 v[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int f = lo + min(i0 + u, len - 1);
                v[u] = live ? sp[(size_t)f * a.T] : vec4(0.f);
                g[u] = live ? fp[(size_t)f * a.J] : vec4(0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int f = lo + i0 + u;
                if (i0 + u >= len) break;
                if (fb && in_bands(fb, a.n_fb, f)) continue;  // uniform: a masked bin contributes nothing
                const float w = a.w[(size_t)f * a.M + m];
                const float re0 = v[u][0], re1 = v[u][1], im0 = v[u][2], im1 = v[u][3];
                const float ga = g[u][0], gb = g[u][1], cr = g[u][2], ci = g[u][3];
                const float z0r = ga * re0, z0i = ga * im0;
                const float yr = fmaf(ci, im0, fmaf(-cr, re0, re1));   // Re (X1 - c X0)
                const float yi = fmaf(-ci, re0, fmaf(-cr, im0, im1));  // Im (X1 - c X0)
                const float z1r = gb * yr, z1i = gb * yi;
                const float q = fmaf(z1i, z1i, fmaf(z1r, z1r, fmaf(z0r, z0r, z0i * z0i)));
                s = fmaf(w, q, s);
            }
        }
        float e = a.wnorm[m] * s;
        if (a.log) e = logf(e + kWhitenLogEps);
        if (valid) out[(size_t)m * a.T] = e;
    }
}
