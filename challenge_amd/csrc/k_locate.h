// k_locate.h -- event localisation: the noise-whitened steered response of a two-microphone delay vector over event frames.
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K16: spectrum [B, F, T, 4] = (re0, re1, im0, im1), whitening factors [B, F, J, 4] = (a, b, Re c, Im c) of blocks of `block`
// frames (k_whiten.h; NULL: a = b = 1, c = 0, J = 1) and E events (sample, first frame, last frame) -> curve [E, L] double and
// n_terms [E] int64, L = 2 N + 1 lags n = -N .. N in steps of 1 / q sample.  An event is cut at block boundaries into
// segments j = first / block .. last / block; segment s of the call is one row of the workspace.  For (segment, bin k) with
// (a, b, c) = fac[b, k, j], a != 0:
//     z0 = a X0,  z1 = b (X1 - c X0),  p00 = sum |z0|^2,  p11 = sum |z1|^2,  p10 = sum z1 conj(z0)   over the segment's frames
//     e = exp(-i 2 pi k n / (n_fft q)),  s1 = b (e - c)
//     term = (a^2 p00 + |s1|^2 p11 + 2 a Re(conj(s1) p10)) / (a^2 + |s1|^2)            ( = sum_t |s^H z|^2 / (s^H s), s = [a, s1])
// curve[e, n] = the sum of the terms over the event's segments and the bins [k_lo, k_hi); n_terms[e] = the sum over the
// contributing (segment, bin) pairs of the segment's frame count.  Two launches, no atomics, fixed summation orders: the same
// inputs give the same bits, and an event's row depends on nothing but its own record, spectrum and factors.
//
//   1. k_locate_moments: one wave per (segment, bin).  The segment's event is found by bisection over the events' segment
//      offsets (uniform).  Lane l reads frames t0 + l, t0 + l + 64, ...: one 16-byte load each, coalesced along t, the fp32
//      inputs converted to double BEFORE any product, y = X1 - c X0 per frame (two fmas per component), three sums per lane
//      in frame order (|X0|^2, |y|^2, y conj(X0): four doubles), a fixed xor tree, then lane 0 scales by a^2, b^2 and a b and
//      writes (p00, p11, Re p10, Im p10) as doubles into the workspace [S, k_hi - k_lo, 4].  a == 0 writes zeros.
//   2. k_locate_scan: one wave per (event, lag).  Lane l walks the event's segments in order and, per segment, the bins
//      k_lo + l, k_lo + l + 64, ...; the phase is m = (k n) mod (n_fft q) in integers, folded to |m| <= n_fft q / 2, then
//      sincospi(2 m / (n_fft q)) in double; one double sum per lane in that order, the same xor tree, lane 0 writes.  The lag-0
//      wave of an event also counts n_terms (int64: the order cannot matter).
//   Error against the float64 definition from the same fp32 spectrum and factors, in units of u = 2^-53 (has
//   the derivation): with Y = |X1| + |c| |X0|, P00 = a^2 sum |X0|^2, P11 = b^2 sum Y^2, P10 = a b sum |X0| Y, S1 = b (1 + |c|),
//       A = (a^2 P00 + S1^2 P11 + 2 a S1 P10) (a^2 + S1^2) / (a^2 + |s1|^2)^2        (a term's magnitude: nothing cancelled)
//   |curve - exact| <= (n_l + n_s + 72) u sum A, n_l = ceil(longest segment / 64), n_s = segments x ceil((k_hi - k_lo) / 64).
// ---------------------------------------------------------------------------
constexpr int kLocateMaxLags = 4097;  // 2 N + 1 <= 4097: N <= 2048 steps either way

struct LocateArgs {
    const float* spec;   // [B, F, T, 4], 16-byte aligned
    const float* fac;    // [B, F, J, 4], 16-byte aligned, or nullptr (identity)
    const int* events;   // [E, 4] = (sample, first frame, last frame, first segment)
    double* mom;         // [S, nk, 4]
    double* curve;       // [E, L]
    long long* n_terms;  // [E]
    int B, F, T, J, block;
    int E, S, k_lo, nk;  // nk = k_hi - k_lo
    int N, q, L;         // L = 2 N + 1
    long long period;    // n_fft q
    int cut;             // K19 (k_track.h): rows are cut at multiples of `cut` frames (block % cut == 0 unless J == 1); K16 does not read it
};

template <typename T>
__device__ __forceinline__ T locate_wave_sum(T v) {  // the fixed xor tree over the 64 lanes
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// kSteps (K19, k_track.h): a row is a STEP of a.cut frames instead of a block - events[.][3] then counts steps, the factors are
// still those of the row's block t0 / block (block % cut == 0 unless there is one block: a step lies in one block).  false is K16's kernel, untouched.
template <bool kSteps>
__global__ __launch_bounds__(256) void k_locate_moments(const LocateArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (long long)a.S * a.nk) return;  // wave-uniform
    const int s = (int)(wave / a.nk), ki = (int)(wave % a.nk), k = a.k_lo + ki;
    int lo = 0, hi = a.E - 1;  // the last event whose first segment is <= s (uniform)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.events[4 * mid + 3] <= s) lo = mid; else hi = mid - 1;
    }
    const int b = a.events[4 * lo], first = a.events[4 * lo + 1], last = a.events[4 * lo + 2];
    const int cut = kSteps ? a.cut : a.block;
    const int r = first / cut + (s - a.events[4 * lo + 3]);
    const int t0 = max(first, r * cut), t1 = min(last, (r + 1) * cut - 1);  // inclusive
    const int j = kSteps ? t0 / a.block : r;
    double* out = a.mom + 4 * wave;
    // (the host checked every record; a record that does not fit writes zeros and reads nothing)
    const bool fits = b >= 0 && b < a.B && first >= 0 && last < a.T && j >= 0 && j < a.J && t0 <= t1;
    double fa = 1., fb = 1., cr = 0., ci = 0.;
    if (fits && a.fac) {
        const vec4 g = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
        fa = g[0], fb = g[1], cr = g[2], ci = g[3];
    }
    if (!fits || fa == 0.) {
        if (lane == 0) out[0] = 0., out[1] = 0., out[2] = 0., out[3] = 0.;
        return;
    }
    const vec4* sp = reinterpret_cast<const vec4*>(a.spec) + ((size_t)b * a.F + k) * a.T;
    double s00 = 0., s11 = 0., sre = 0., sim = 0.;
#pragma unroll 2
    for (int t = t0 + lane; t <= t1; t += 64) {
        const vec4 v = sp[t];
        const double re0 = v[0], re1 = v[1], im0 = v[2], im1 = v[3];
        const double yr = fma(ci, im0, fma(-cr, re0, re1));   // Re (X1 - c X0)
        const double yi = fma(-ci, re0, fma(-cr, im0, im1));  // Im (X1 - c X0)
        s00 += fma(im0, im0, re0 * re0);
        s11 += fma(yi, yi, yr * yr);
        sre += fma(yi, im0, yr * re0);  // y conj(X0)
        sim += fma(-yr, im0, yi * re0);
    }
    s00 = locate_wave_sum(s00);
    s11 = locate_wave_sum(s11);
    sre = locate_wave_sum(sre);
    sim = locate_wave_sum(sim);
    if (lane != 0) return;
    const double ab = fa * fb;
    out[0] = (fa * fa) * s00;
    out[1] = (fb * fb) * s11;
    out[2] = ab * sre;
    out[3] = ab * sim;
}

__global__ __launch_bounds__(256) void k_locate_scan(const LocateArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (long long)a.E * a.L) return;  // wave-uniform
    const int e = (int)(wave / a.L), li = (int)(wave % a.L);
    const long long n = (long long)li - a.N;
    const int b = a.events[4 * e], first = a.events[4 * e + 1], last = a.events[4 * e + 2], s0 = a.events[4 * e + 3];
    const bool fits = b >= 0 && b < a.B && first >= 0 && first <= last && last < a.T && s0 >= 0;
    const int j0 = fits ? first / a.block : 0, n_seg = fits ? last / a.block - j0 + 1 : 0;
    const double period = (double)a.period;
    double sum = 0.;
    long long count = 0;
    for (int i = 0; i < n_seg; ++i) {
        const int j = j0 + i;
        if (j >= a.J || s0 + i >= a.S) break;  // (never, for records the host checked)
        const int frames = min(last, (j + 1) * a.block - 1) - max(first, j * a.block) + 1;
        const double* mom = a.mom + (size_t)(s0 + i) * a.nk * 4;
        for (int ki = lane; ki < a.nk; ki += 64) {
            const int k = a.k_lo + ki;
            double fa = 1., fb = 1., cr = 0., ci = 0.;
            if (a.fac) {
                const vec4 g = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
                fa = g[0], fb = g[1], cr = g[2], ci = g[3];
            }
            if (fa == 0.) continue;  // a silent block contributes nothing
            count += frames;
            const double p00 = mom[4 * ki], p11 = mom[4 * ki + 1], pre = mom[4 * ki + 2], pim = mom[4 * ki + 3];
            long long m = ((long long)k * n) % a.period;  // exact: |k n| < 2^31 2^12
            if (m < 0) m += a.period;
            if (2 * m > a.period) m -= a.period;  // |m| <= period / 2
            double sn, cs;
            sincospi((double)(2 * m) / period, &sn, &cs);  // e = cs - i sn (one rounding in the argument)
            const double s1r = fb * (cs - cr), s1i = fb * (-sn - ci);
            const double s1sq = fma(s1i, s1i, s1r * s1r), a2 = fa * fa;
            const double cross = fma(s1i, pim, s1r * pre);  // Re(conj(s1) p10)
            const double num = a2 * p00 + s1sq * p11 + (2.0 * fa) * cross;
            sum += num / (a2 + s1sq);
        }
    }
    sum = locate_wave_sum(sum);
    if (li == 0) count = locate_wave_sum(count);
    if (lane != 0) return;
    a.curve[wave] = sum;
    if (li == 0) a.n_terms[e] = count;
}
