// k_beamform.h -- event extraction: the MVDR beamformer of a two-microphone delay vector applied over the frames of events.
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K17: spectrum [B, F, T, 4] = (re0, re1, im0, im1), whitening factors [B, F, J, 4] = (a, b, Re c, Im c) of blocks of `block`
// frames (k_whiten.h; NULL: a = b = 1, c = 0, J = 1), E events (sample, first frame, last frame, first output frame) and their
// delays tdoa [E] (double, samples; positive: channel 1 hears the event later) -> one slab [F, T_e, 2] = (Re Y, Im Y) fp32 per
// event, T_e = last - first + 1, slab e at float 2 F x (first output frame): iris_istft's record layout for one channel.
// For frame t of the event, block j = t / block, bin k, (a, b, c) = fac[sample, k, j]:
//     k outside [k_lo, k_hi), a == 0 (a silent block) or tdoa not finite:  Y = 0 exactly (the spectrum is not read)
//     r = k tdoa / n_fft (double), r -= rint(r),  e = cos(2 pi r) - i sin(2 pi r)                     (sincospi(2 r))
//     s1 = b (e - c),  den = a^2 + |s1|^2,  g1 = b conj(s1) / den,  g0 = a^2 / den - g1 c
//     Y = g0 X0 + g1 X1      ( = s^H z / (s^H s), z = (a X0, b (X1 - c X0)), s = (a, s1): the MVDR output for d = [1, e] )
// One launch, no atomics, no workspace, one fixed operation sequence per value: the same inputs give the same bits, and a
// frame's value depends on its sample, frame, bin and delay only - not on the event it sits in, nor on the tiling below.
//
//   A wave takes (event, group of kBeamBins bins, chunk of kBeamChunk frames); waves past an event's last chunk leave at once.
//   Lane l < kBeamBins forms e for bin k0 + l once (it does not depend on the block), and per block the chunk touches g0, g1
//   in double from the fp32 factors, rounded ONCE to fp32 and kept in four registers: each (event, bin, block) coefficient is
//   formed by exactly one lane of one chunk's wave, 16 at a time, instead of once per frame.  The tile (bins x the block's
//   frames inside the chunk) is then walked as ONE flat index, t fastest, 64 elements per step: lane i takes (bin idx / n,
//   frame idx % n) - advanced by the uniform (64 / n, 64 % n), no division in the loop - fetches its bin's coefficients from
//   the lane that holds them (four __shfl, executed by the whole wave: the loop's trip count is uniform and only the load
//   and the store are predicated), loads one 16-byte spectrum record, stores 8 bytes; kBeamSteps steps are issued together,
//   so a lane has that many loads in flight.  Rows of a tile are contiguous in the spectrum (runs of n records) and in the
//   slab (runs of n pairs), so a 20-frame event fills a step with 3.2 bins instead of leaving 44 lanes idle.  24 bytes per
//   (bin, frame): a streaming kernel.
//   Per component: one product and three fmas in a fixed order,
//       Re Y = fma(-g1i, x1i, fma(g1r, x1r, fma(-g0i, x0i, g0r x0r))),  Im Y = fma(g1i, x1r, fma(g1r, x1i, fma(g0i, x0r, g0r x0i)))
//   Error against the float64 definition from the same fp32 inputs, per real component, u = 2^-24, A = |g0| |X0| + |g1| |X1|:
//       4 u A  the product and the three fmas: every partial sum is at most |g0r x0r| + |g0i x0i| + |g1r x1r| + |g1i x1i| <= A
//              (Cauchy-Schwarz per pair)
//       1 u A  the fp32 rounding of the stored coefficients: u (|g0r| |x0r| + |g0i| |x0i| + ...) <= u A
//       1 u A  spare: second-order terms and the double arithmetic of g0, g1 (2^-53 relative to their uncancelled parts)
//   |Y - exact| <= 6 u A.  Nothing is cancelled in A, since nulling is cancellation.
// ---------------------------------------------------------------------------
constexpr int kBeamBins = 16;     // bins per wave: one coefficient set per lane 0 .. 15 (at most 64: a lane each)
constexpr int kBeamChunk = 256;   // frames per wave
constexpr int kBeamSteps = 8;     // 64-element steps whose loads are issued together
// (32 bins x 4 steps measured 15.1 us per launch where 16 x 8 takes 9.1 us, 64 events of 64 frames at F = 257: twice the waves
// and a quarter of the dependent round trips per wave; 136 VGPRs, occupancy 3, against 46 and 8.)

struct BeamformArgs {
    const float* spec;    // [B, F, T, 4], 16-byte aligned
    const float* fac;     // [B, F, J, 4], 16-byte aligned, or nullptr (identity)
    const int* events;    // [E, 4] = (sample, first frame, last frame, first output frame)
    const double* tdoa;   // [E]
    float* out;           // [total, ...]: slab e = [F, T_e, 2] at float 2 F events[e][3], 8-byte aligned
    int B, F, T, J, block;
    int E, k_lo, k_hi;
    int groups;           // ceil(F / kBeamBins)
    long long total;      // the frames of all events: no slab reaches past 2 F total floats
    double n_fft;         // 2 (F - 1)
};

// The two double-precision steps both kernels of this file share, so that they cannot drift apart: the phase e = cs - i sn of
// bin k at a delay, and (g0, g1) of one (a, b, c), rounded ONCE to fp32.
__device__ __forceinline__ void beam_phase(int k, double tdoa, double n_fft, double& sn, double& cs) {
    double r = (double)k * tdoa / n_fft;
    r -= rint(r);
    sincospi(2.0 * r, &sn, &cs);  // e = cs - i sn
}

// (the double core is shared with k_postfilter.h, which needs den, g0 and g1 before the rounding)
__device__ __forceinline__ void beam_weights_core(double fa, double fb, double cr, double ci, double sn, double cs, double& den,
                                                  double& h0r, double& h0i, double& h1r, double& h1i) {
    const double s1r = fb * (cs - cr), s1i = fb * (-sn - ci), a2 = fa * fa;
    den = a2 + (s1r * s1r + s1i * s1i);
    h1r = fb * s1r / den, h1i = -(fb * s1i) / den;  // g1 = b conj(s1) / den
    h0r = a2 / den - (h1r * cr - h1i * ci);         // g0 = a^2 / den - g1 c
    h0i = -(h1r * ci + h1i * cr);
}

__device__ __forceinline__ void beam_weights(double fa, double fb, double cr, double ci, double sn, double cs, float& g0r,
                                             float& g0i, float& g1r, float& g1i) {
    double den, h0r, h0i, h1r, h1i;
    beam_weights_core(fa, fb, cr, ci, sn, cs, den, h0r, h0i, h1r, h1i);
    g1r = (float)h1r, g1i = (float)h1i;
    g0r = (float)h0r, g0i = (float)h0i;
}

__global__ __launch_bounds__(256) void k_beamform(const BeamformArgs a) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    typedef float vec2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x;
    const int w = blockIdx.y * 4 + (threadIdx.x >> 6);  // wave-uniform from here on
    const int g = w % a.groups, chunk = w / a.groups;
    if (e >= a.E) return;
    const int b = a.events[4 * e], first = a.events[4 * e + 1], last = a.events[4 * e + 2], row0 = a.events[4 * e + 3];
    // (the host checked every record; a record that does not fit reads nothing and writes nothing)
    const bool fits = b >= 0 && b < a.B && first >= 0 && first <= last && last < a.T && row0 >= 0 &&
                      (long long)row0 + (last - first + 1) <= a.total;
    if (!fits) return;
    const int te = last - first + 1;
    if ((long long)chunk * kBeamChunk >= te) return;
    const int k0 = g * kBeamBins, nkb = min(kBeamBins, a.F - k0);
    const int c0 = first + chunk * kBeamChunk, c1 = min(last, c0 + kBeamChunk - 1);  // inclusive
    const double tdoa = a.tdoa[e];
    const int k = k0 + lane;
    const bool steer = lane < nkb && k >= a.k_lo && k < a.k_hi && isfinite(tdoa);
    double sn = 0., cs = 1.;
    if (steer) beam_phase(k, tdoa, a.n_fft, sn, cs);
    const vec4* spec = reinterpret_cast<const vec4*>(a.spec) + ((size_t)b * a.F + k0) * a.T;
    vec2* slab = reinterpret_cast<vec2*>(a.out) + ((size_t)row0 * a.F + (size_t)k0 * te);
    for (int j = c0 / a.block; j <= c1 / a.block && j < a.J; ++j) {
        const int t0 = max(c0, j * a.block), t1 = min(c1, (j + 1) * a.block - 1);
        const int n = t1 - t0 + 1, count = nkb * n;
        float g0r = 0.f, g0i = 0.f, g1r = 0.f, g1i = 0.f;
        bool live = false;
        if (steer) {
            double fa = 1., fb = 1., cr = 0., ci = 0.;
            if (a.fac) {
                const vec4 q = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
                fa = q[0], fb = q[1], cr = q[2], ci = q[3];
            }
            if (fa != 0.) {
                live = true;
                beam_weights(fa, fb, cr, ci, sn, cs, g0r, g0i, g1r, g1i);
            }
        }
        const unsigned long long alive = __ballot(live);
        int kk = lane / n, tl = lane % n;
        const int dq = 64 / n, dr = 64 % n;
        for (int base = 0; base < count; base += 64 * kBeamSteps) {  // uniform: every lane runs the shuffles
            vec4 v[kBeamSteps], c[kBeamSteps];
            size_t at[kBeamSteps];
            bool on[kBeamSteps], hot[kBeamSteps];
#pragma unroll
            for (int u = 0; u < kBeamSteps; ++u) {  // kBeamSteps loads in flight per lane
                c[u] = vec4{__shfl(g0r, kk), __shfl(g0i, kk), __shfl(g1r, kk), __shfl(g1i, kk)};
                on[u] = base + 64 * u + lane < count;  // then kk < nkb <= kBeamBins
                hot[u] = on[u] && ((alive >> (kk & 63)) & 1);
                v[u] = vec4{0.f, 0.f, 0.f, 0.f};
                if (hot[u]) v[u] = spec[(size_t)kk * a.T + t0 + tl];  // (re0, re1, im0, im1)
                at[u] = (size_t)kk * te + (t0 - first) + tl;
                kk += dq, tl += dr;
                if (tl >= n) tl -= n, ++kk;
            }
#pragma unroll
            for (int u = 0; u < kBeamSteps; ++u) {
                vec2 y;
                y[0] = __builtin_fmaf(-c[u][3], v[u][3], __builtin_fmaf(c[u][2], v[u][1], __builtin_fmaf(-c[u][1], v[u][2], c[u][0] * v[u][0])));
                y[1] = __builtin_fmaf(c[u][3], v[u][1], __builtin_fmaf(c[u][2], v[u][3], __builtin_fmaf(c[u][1], v[u][0], c[u][0] * v[u][2])));
                if (!hot[u]) y = vec2{0.f, 0.f};  // exactly 0, whatever the spectrum holds there
                if (on[u]) slab[at[u]] = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// K19 (with k_track.h): the same beamformer with one delay PER OUTPUT FRAME - tdoa [total] double, frame t of event e reads
// tdoa[row0 + (t - first)], row0 the event's first output frame - for an event whose delay moves (transforms.track_delays).
// Everything else is K17's definition, read per frame: Y = 0 exactly where k is outside [k_lo, k_hi), a == 0 or the frame's
// delay is not finite.  One thread per (bin, frame): a wave takes one bin and 64 consecutive frames of an event (16-byte loads
// and 8-byte stores, both coalesced along t); the thread forms e, g0, g1 in double with beam_phase / beam_weights - the very
// statements of k_beamform - rounds once, and runs the same product and three fmas.  So the 6 u A bound above holds unchanged,
// a frame's value depends on its sample, frame, bin and delay only, and a delay that is constant over an event gives the bits
// of k_beamform.  It pays one double sincospi per (bin, frame) where k_beamform pays one per (bin, chunk): a small launch,
// deliberately not tuned further.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_beamform_frames(const BeamformArgs a, const int chunks) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    typedef float vec2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x;
    const long long w = (long long)blockIdx.y * 4 + (threadIdx.x >> 6);  // wave-uniform: (bin, chunk of 64 frames)
    const int k = (int)(w / chunks), chunk = (int)(w % chunks);
    if (e >= a.E || k >= a.F) return;
    const int b = a.events[4 * e], first = a.events[4 * e + 1], last = a.events[4 * e + 2], row0 = a.events[4 * e + 3];
    // (the host checked every record; a record that does not fit reads nothing and writes nothing)
    const bool fits = b >= 0 && b < a.B && first >= 0 && first <= last && last < a.T && row0 >= 0 &&
                      (long long)row0 + (last - first + 1) <= a.total;
    if (!fits) return;
    const int te = last - first + 1;
    const long long tl = (long long)chunk * 64 + lane;  // the frame inside the event
    if (tl >= te) return;
    const int t = first + (int)tl, j = t / a.block;
    const double tdoa = a.tdoa[(size_t)row0 + tl];
    vec2 y = vec2{0.f, 0.f};  // exactly 0 unless the bin is steered, whatever the spectrum holds there
    if (k >= a.k_lo && k < a.k_hi && isfinite(tdoa) && j < a.J) {
        double fa = 1., fb = 1., cr = 0., ci = 0.;
        if (a.fac) {
            const vec4 q = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
            fa = q[0], fb = q[1], cr = q[2], ci = q[3];
        }
        if (fa != 0.) {
            double sn, cs;
            beam_phase(k, tdoa, a.n_fft, sn, cs);
            float g0r, g0i, g1r, g1i;
            beam_weights(fa, fb, cr, ci, sn, cs, g0r, g0i, g1r, g1i);
            const vec4 v = reinterpret_cast<const vec4*>(a.spec)[((size_t)b * a.F + k) * a.T + t];  // (re0, re1, im0, im1)
            y[0] = __builtin_fmaf(-g1i, v[3], __builtin_fmaf(g1r, v[1], __builtin_fmaf(-g0i, v[2], g0r * v[0])));
            y[1] = __builtin_fmaf(g1i, v[1], __builtin_fmaf(g1r, v[3], __builtin_fmaf(g0i, v[0], g0r * v[2])));
        }
    }
    reinterpret_cast<vec2*>(a.out)[(size_t)row0 * a.F + (size_t)k * te + tl] = y;
}
