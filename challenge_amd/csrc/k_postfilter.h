// k_postfilter.h -- event extraction: the decision-directed Wiener post-filter on the beamformer's output.
// Part of the single translation unit iris_frontend.hip (after k_beamform.h: it shares beam_phase and beam_weights_core).
#pragma once
// ---------------------------------------------------------------------------
// K20: the slabs k_beamform / k_beamform_frames wrote - slab e = [F, T_e, 2] = (Re Y, Im Y) fp32 at float 2 F x (first output
// frame) - the SAME events, delays (one per event, or one per output frame: per_frame) and whitening factors [B, F, J, 4] =
// (a, b, Re c, Im c) of noise="quiet" (the covariance R of the frames outside the events), the loading they were made with, a
// smoothing alpha in [0, 1) and one gain floor g_min[e] in (0, 1] per event -> slabs Z of the same layout.
// The beamformer's output noise power is known in closed form: with w = (conj g0, conj g1) the MVDR weights of the LOADED
// covariance R + dI, w^H (R + dI) w = 1 / den (den = a^2 + |s1|^2 = d^H (R + dI)^-1 d), so
//     S = 1/a^2 + |c|^2/a^2 + 1/b^2          (the trace of R + dI from its Cholesky factor l00 = 1/a, l10 = c/a, l11 = 1/b)
//     d = loading S / (2 (1 + loading))      (d = loading tr R / 2 and tr (R + dI) = (1 + loading) tr R)
//     phi = max(1/den - d (|g0|^2 + |g1|^2), kPhiFloor / den)          ( = w^H R w; the floor guards a perfectly coherent R )
// For bin k in [k_lo, k_hi), frame t of event e, block j = t / block, in double from the fp32 inputs (g0, g1, den: the double
// values of beam_weights_core, before k_beamform rounds them):
//     gamma = |Y|^2 / phi;  gamma = 0 where Y is 0 by K17's definition (a == 0, j >= J, or a delay that is not finite)
// and along the event's frames, p = 1 before the first:
//     xi = alpha p + (1 - alpha) max(gamma - 1, 0),  G = max(xi / (1 + xi), g_min[e]),  p = G^2 gamma,  Z = fl32(G) Y
// (the decision-directed a-priori SNR of Ephraim & Malah with the Wiener gain).  Bins outside [k_lo, k_hi) are exactly 0 and
// are not read; g_min = 1 gives G = 1 and Z = Y bit for bit.  Every max is continuous: no rounding flips a branch into another
// value.  Error per real component against this definition: |Z - exact| <= 3 u |G| |Y|, u = 2^-24 - one u for fl32(G), one for
// the product, one spare for the double arithmetic (the recursion contracts by alpha: 2^-53 grows by at most 1 / (1 - alpha),
// and the cancellation in phi by at most 1 / kPhiFloor).
//
// The recursion is nonlinear - no scan - so it is one sequential chain per (event, bin), while the slabs store t fastest.
//   A workgroup (4 waves) takes (event, kPostBins = 64 bins) and walks the event in chunks of 64 frames:
//     1. all four waves, lanes along t, wave w the bins w, w + 4, ..: load Y (8 bytes a lane, coalesced), form gamma in double
//        and write it to an LDS tile [64 bins][65] doubles (33 280 bytes).
//     2. wave 0, a lane per bin, runs the chunk's steps out of LDS, writes G over gamma and keeps p in a register across
//        chunks.  The row stride of 65 doubles puts lane l of step s at bank 2 (l + s) mod 64: the 32 lanes an 8-byte LDS
//        read serves per cycle, and the 16 a write serves, fall on distinct banks - the column walk has no conflicts.
//     3. all four waves read G along t, round it ONCE to fp32, load Y again (the 32 KB a chunk's tile covers are still in
//        cache; holding them in 32 registers across the barriers cost 205 VGPRs and 44 spilled SGPRs), multiply and store
//        coalesced.
//   The delay is read per frame or per event by one flag and goes through the same statements either way, so per-frame delays
//   that are constant over an event give the per-event bits.  One launch, no atomics, no workspace; an event's value depends
//   on its own slab, record, delays and floor only.
// ---------------------------------------------------------------------------
constexpr int kPostBins = 64;     // bins per workgroup: a lane of wave 0 each
constexpr int kPostChunk = 64;    // frames per chunk: a lane each in phases 1 and 3
constexpr int kPostStride = 65;   // doubles per LDS row
constexpr double kPhiFloor = 1e-3;

struct PostfilterArgs {
    const float* in;      // [total, ...]: slab e = [F, T_e, 2] at float 2 F events[e][3], 8-byte aligned
    const float* fac;     // [B, F, J, 4], 16-byte aligned
    const int* events;    // [E, 4] = (sample, first frame, last frame, first output frame)
    const double* tdoa;   // [E], or [total] with per_frame
    const double* gmin;   // [E]
    float* out;           // as in
    int B, F, T, J, block;
    int E, k_lo, k_hi, per_frame;
    long long total;
    double n_fft, alpha, loading;
};

__global__ __launch_bounds__(256) void k_postfilter(const PostfilterArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    typedef float vec2 __attribute__((ext_vector_type(2)));
    __shared__ double tile[kPostBins * kPostStride];
    constexpr int kRows = kPostBins / 4;  // bins per wave in phases 1 and 3
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x, k0 = blockIdx.y * kPostBins;
    if (e >= a.E || k0 >= a.F) return;  // (workgroup-uniform, as every return below: no barrier is left waiting)
    const int b = a.events[4 * e], first = a.events[4 * e + 1], last = a.events[4 * e + 2], row0 = a.events[4 * e + 3];
    // (the host checked every record; a record that does not fit reads nothing and writes nothing)
    const bool fits = b >= 0 && b < a.B && first >= 0 && first <= last && last < a.T && row0 >= 0 &&
                      (long long)row0 + (last - first + 1) <= a.total;
    if (!fits) return;
    const int te = last - first + 1;
    const double gmin = a.gmin[e], om = 1.0 - a.alpha;
    const double tdoa_e = a.per_frame ? 0. : a.tdoa[e];
    const vec2* in = reinterpret_cast<const vec2*>(a.in) + (size_t)row0 * a.F;
    vec2* out = reinterpret_cast<vec2*>(a.out) + (size_t)row0 * a.F;
    double p = 1.0;  // wave 0, lane l: the chain of bin k0 + l
    for (int c0 = 0; c0 < te; c0 += kPostChunk) {
        const int n = min(kPostChunk, te - c0), tl = c0 + lane;
        const bool mine = lane < n;
        const int j = (first + tl) / a.block;
        double tdoa = tdoa_e;
        if (a.per_frame && mine) tdoa = a.tdoa[(size_t)row0 + tl];
        const bool steer = mine && isfinite(tdoa) && j < a.J;
#pragma unroll 2
        for (int r = 0; r < kRows; ++r) {
            const int kk = wave + 4 * r, k = k0 + kk;
            double gamma = 0.;
            if (steer && k >= a.k_lo && k < a.k_hi) {  // (k_hi <= F; bins outside are not read)
                const vec2 y = in[(size_t)k * te + tl];
                const vec4 q = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
                const double fa = q[0], fb = q[1], cr = q[2], ci = q[3];
                if (fa != 0.) {
                    double sn, cs, den, h0r, h0i, h1r, h1i;
                    beam_phase(k, tdoa, a.n_fft, sn, cs);
                    beam_weights_core(fa, fb, cr, ci, sn, cs, den, h0r, h0i, h1r, h1i);
                    const double a2 = fa * fa;
                    const double trace = 1.0 / a2 + (cr * cr + ci * ci) / a2 + 1.0 / (fb * fb);
                    const double d = a.loading * trace / (2.0 * (1.0 + a.loading));
                    const double w2 = (h0r * h0r + h0i * h0i) + (h1r * h1r + h1i * h1i);
                    const double phi = fmax(1.0 / den - d * w2, kPhiFloor / den);
                    gamma = ((double)y[0] * (double)y[0] + (double)y[1] * (double)y[1]) / phi;
                }
            }
            tile[kk * kPostStride + lane] = gamma;
        }
        __syncthreads();
        if (wave == 0) {
            double* row = tile + lane * kPostStride;
            for (int s = 0; s < n; ++s) {
                const double gamma = row[s];
                const double xi = a.alpha * p + om * fmax(gamma - 1.0, 0.);
                const double g = fmax(xi / (1.0 + xi), gmin);
                p = g * g * gamma;
                row[s] = g;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int kk = wave + 4 * r, k = k0 + kk;
            if (mine && k < a.F) {
                const float g = (float)tile[kk * kPostStride + lane];  // rounded ONCE
                vec2 y = vec2{0.f, 0.f};                                // bins outside [k_lo, k_hi): not read, exactly 0
                if (k >= a.k_lo && k < a.k_hi) y = in[(size_t)k * te + tl];
                out[(size_t)k * te + tl] = vec2{g * y[0], g * y[1]};
            }
        }
        __syncthreads();  // the next chunk overwrites the tile
    }
}
