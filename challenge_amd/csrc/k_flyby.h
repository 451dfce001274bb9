// k_flyby.h -- fly-by augmentation: a static source heard by a moving microphone array.  A time-varying fractional delay per
// channel (Doppler shift, a changing inter-channel delay), the spherical-spreading level and one ground reflection over a ragged
// set of waveforms, each with its own flight, in one launch.  Part of the single translation unit iris_frontend.hip.
//
// Per record (iris_flyby_src): x [C, L] -> y [C, L], channel c from row c.  Source at (0, 0, z_s) over the ground plane z = 0,
// array centre p0 + v t (t = n / 16000), microphone c at the centre + mic[c]; path 0 the direct sound (a_0 = 1), path 1 the image
// source (0, 0, -z_s) with a_1 = beta.  With d the distance from the microphone at sample n to the (image) source:
//     pos = n - (d - r_ref) * (16000 / 343),   g = a_p * r_ref / d,   i0 = floor(pos), frac = (float)(pos - i0)
//     y[c, n] = sum_p g * sum_s x[c, s] * cut * w(cut * ((s - i0) - frac)),      cut = 0.99 / (1 + |v| / 343),
//     w(t)    = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,               x[c, s] = 0 outside [0, L)
// - k_speed.h's window at a position that follows the flight.  A static source and a moving receiver in a still medium: the
// emission time is explicit, there is no retarded-time equation to solve.  d pos / d n <= 1 + |v| / 343, so one cut per record
// is alias-safe for the whole clip and the tap count 2 H + 2, H = ceil(6 / cut), is constant.
//   blockIdx.y = record, blockIdx.x = a tile of kFlybyTile consecutive output samples; the 256-thread workgroup handles all
//   channels and paths of its tile:
//   1. pos is monotonic in n (|v| < 343), so the input a (channel, path) needs is one contiguous span, [i0(first) - H,
//      i0(last) + H + 1]; the spans of a tile differ by the microphone spacing and by the detour of the reflection (at most
//      2 z_s, 140 samples at 1.5 m), so ONE span [lo, hi] over all of them is staged per channel: coalesced, 16 bytes per lane
//      where the rows are aligned, zeros outside [0, L).  Its ends come from 2 C P threads that evaluate the first and the last
//      position of their (channel, path) and meet in LDS.  A span too long for the buffer (many channels, microphones far apart)
//      is read from global memory instead.
//   2. neighbouring threads take neighbouring n: their LDS reads sit about one word apart, their stores are coalesced.  The
//      float64 work per (sample, channel, path) - three fmas for the offset, three operations for d^2, a square root, a divide
//      for the gain, an fma and a floor for the position - sits outside the tap loop.  Every channel has its own position, so
//      unlike k_speed.h no tap is shared between channels.
// Every rounding is spelled out (fma / fmaf where one is meant), and a tap is read only where both the source and the span
// have it - the span clamp changes nothing for a monotonic position - so the value does not depend on the tile or on the
// staging: bitwise reproducible, a batch equals the single calls.  Vector stores only; no atomics, no workspace; every loop bound
// comes from the record.  n_paths == 0 copies the source bit for bit.
#pragma once

constexpr int kFlybyThreads = 256;
constexpr int kFlybyTile = 1024;    // output samples per workgroup (4 per thread)
constexpr int kFlybyLds = 8192;     // floats of input spans held in LDS (32 KiB): 6 channels at 15 m/s with the ground path
constexpr double kFlybySound = 343.0, kFlybyFs = 16000.0;
constexpr double kFlybyScale = kFlybyFs / kFlybySound;   // samples per metre

static_assert(sizeof(iris_flyby_src) == 96 + 24 * IRIS_FLYBY_MAX_CHAN,
              "iris_flyby_src: two pointers, two ints, nine doubles, the microphones");

// |v|^2, the same statements wherever it is needed
__device__ __forceinline__ double flyby_vv(const iris_flyby_src& d) {
    return fma(d.v[2], d.v[2], fma(d.v[1], d.v[1], d.v[0] * d.v[0]));
}

// a record the kernel leaves alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool flyby_skip(const iris_flyby_src& d, int channels, int max_len) {
    if (channels < 1 || channels > IRIS_FLYBY_MAX_CHAN) return true;   // (iris_flyby refuses these: `ends` and `mic` hold 8)
    if (!d.src || !d.dst || d.len <= 0 || d.len > max_len || d.n_paths < 0 || d.n_paths > 2) return true;
    if (d.n_paths == 0) return false;   // the identity reads no geometry
    bool finite = isfinite(d.z_s) && isfinite(d.beta) && isfinite(d.r_ref);
    for (int a = 0; a < 3; ++a) finite = finite && isfinite(d.p0[a]) && isfinite(d.v[a]);
    for (int c = 0; c < channels; ++c)
        for (int a = 0; a < 3; ++a) finite = finite && isfinite(d.mic[c][a]);
    return !finite || !(d.r_ref > 0.0) || !(flyby_vv(d) < kFlybySound * kFlybySound);
}

// the position pos of output sample n on path p of channel c, and the distance behind it
__device__ __forceinline__ double flyby_pos(const iris_flyby_src& d, int c, int p, int n, double* dist) {
    const double t = (double)n / kFlybyFs;
    const double qx = d.p0[0] + d.mic[c][0], qy = d.p0[1] + d.mic[c][1];
    const double qz = (d.p0[2] + d.mic[c][2]) - (p ? -d.z_s : d.z_s);
    const double dx = fma(d.v[0], t, qx), dy = fma(d.v[1], t, qy), dz = fma(d.v[2], t, qz);
    *dist = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
    return fma(-(*dist - d.r_ref), kFlybyScale, (double)n);
}

// floor(pos) as a double inside +-4e9 (NaN: the lower end): whatever lies beyond is further than any source is long
__device__ __forceinline__ double flyby_floor(double pos) { return fmin(fmax(floor(pos), -4.0e9), 4.0e9); }

// the output samples n_beg, n_beg + 256, ... < n_end of every channel; x[c * stride + s - base] is sample s of channel c for
// s_lo <= s <= s_hi (the staged span, which holds zeros outside the source, or the source itself): one body, inlined once per
// address space
__device__ __forceinline__ void flyby_tile(const float* x, size_t stride, long long base, long long s_lo, long long s_hi,
                                           float* __restrict__ dst, const iris_flyby_src& d, int L, int channels, int n_beg,
                                           int n_end, float cut, long long H) {
    for (int n = n_beg; n < n_end; n += kFlybyThreads) {
        for (int c = 0; c < channels; ++c) {
            const float* xc = x + (size_t)c * stride;
            float y = 0.f;
            for (int p = 0; p < d.n_paths; ++p) {
                double dist;
                const double pos = flyby_pos(d, c, p, n, &dist);
                const double fl = flyby_floor(pos);
                const long long i0 = (long long)fl;
                const float frac = (float)(pos - fl);
                const float g = (float)((p ? d.beta : 1.0) * d.r_ref / dist);
                // taps outside the source multiply zeros: skipped (the sum is the same)
                const long long sb = max(max(i0 - H, 0LL), s_lo), se = min(min(i0 + H + 1, (long long)L - 1), s_hi);
                const int s_beg = se < sb ? 0 : (int)sb, s_end = se < sb ? -1 : (int)se;   // 0 <= sb <= se < L, or no tap at all
                float acc = 0.f;
                for (int s = s_beg; s <= s_end; ++s) {
                    const float t = cut * ((float)(s - i0) - frac);
                    if (fabsf(t) < 6.f) {
                        const float pt = 3.14159274101257324f * t;
                        const float sinc = pt == 0.f ? 1.f : sinf(pt) / pt;
                        const float cs = cosf(pt / 12.f);
                        const float tap = (cut * sinc) * (cs * cs);
                        acc = fmaf(xc[(int)(s - base)], tap, acc);
                    }
                }
                y = p ? fmaf(g, acc, y) : g * acc;   // path 0 before path 1
            }
            dst[(size_t)c * L + n] = y;
        }
    }
}

__global__ __launch_bounds__(kFlybyThreads) void k_flyby(const iris_flyby_src* __restrict__ table, int channels, int max_len) {
    __shared__ __attribute__((aligned(16))) float span[kFlybyLds];
    __shared__ long long ends[4 * IRIS_FLYBY_MAX_CHAN];   // floor(pos) of the tile's first (even) / last (odd) sample per (channel, path)
    const iris_flyby_src& d = table[blockIdx.y];
    if (flyby_skip(d, channels, max_len)) return;   // (uniform)
    const int L = d.len, tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * kFlybyTile;
    if (n0 >= L) return;
    const int n_end = (int)min(n0 + kFlybyTile, (long long)L);   // one past the tile's last output sample
    const float* __restrict__ src = d.src;
    float* __restrict__ dst = d.dst;
    if (d.n_paths == 0) {   // the identity: a copy
        for (int c = 0; c < channels; ++c)
            for (int n = (int)n0 + tid; n < n_end; n += kFlybyThreads) dst[(size_t)c * L + n] = src[(size_t)c * L + n];
        return;
    }
    const double cut_d = 0.99 / (1.0 + sqrt(flyby_vv(d)) / kFlybySound);   // in (0.495, 0.99]
    const float cut = (float)cut_d;
    const long long H = (long long)ceil(6.0 / cut_d);   // taps of a sample: s = i0 - H .. i0 + H + 1; 7 .. 13

    // ---- the input span of the tile over all (channel, path), from a multiple of 4 samples (so that 16-byte loads and LDS
    //      writes line up) ----
    const int n_ends = 2 * channels * d.n_paths;
    if (tid < n_ends) {
        const int cp = tid >> 1;
        double dist;
        ends[tid] = (long long)flyby_floor(flyby_pos(d, cp / d.n_paths, cp % d.n_paths, (tid & 1) ? n_end - 1 : (int)n0, &dist));
    }
    __syncthreads();
    long long first = ends[0], last = ends[1];
    for (int k = 2; k < n_ends; k += 2) first = min(first, ends[k]), last = max(last, ends[k + 1]);
    const long long lo = (first - H) & ~3LL;
    const long long hi = last + H + 1;
    const long long len4 = (hi - lo + 4) & ~3LL;                      // floats per channel in LDS, a multiple of 4
    const bool staged = len4 > 0 && len4 * channels <= (long long)kFlybyLds;   // (uniform)
    if (staged) {
        const int quads = (int)(len4 >> 2);
        const bool rows16 = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // every channel row starts on 16 bytes
        for (int q = tid; q < quads * channels; q += kFlybyThreads) {
            const int c = q / quads, j = (q - c * quads) * 4;
            const long long s = lo + j;
            const float* row = src + (size_t)c * L;
            float4 v;
            if (rows16 && s >= 0 && s + 3 < L) {
                v = *reinterpret_cast<const float4*>(row + s);
            } else {
                v.x = (s >= 0 && s < L) ? row[s] : 0.f;
                v.y = (s + 1 >= 0 && s + 1 < L) ? row[s + 1] : 0.f;
                v.z = (s + 2 >= 0 && s + 2 < L) ? row[s + 2] : 0.f;
                v.w = (s + 3 >= 0 && s + 3 < L) ? row[s + 3] : 0.f;
            }
            *reinterpret_cast<float4*>(span + (size_t)c * len4 + j) = v;
        }
        __syncthreads();
    }

    if (staged) flyby_tile(span, (size_t)len4, lo, lo, hi, dst, d, L, channels, (int)n0 + tid, n_end, cut, H);
    else flyby_tile(src, (size_t)L, 0, 0, (long long)L - 1, dst, d, L, channels, (int)n0 + tid, n_end, cut, H);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int iris_flyby(const void* table_dev, int n_src, int channels, int max_len, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_flyby: n_src = %d is negative", n_src);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_flyby: channels = %d must be positive", channels);
    if (channels > IRIS_FLYBY_MAX_CHAN)
        return fail(IRIS_E_UNSUPPORTED, "iris_flyby: channels = %d > %d", channels, IRIS_FLYBY_MAX_CHAN);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_flyby: table is NULL");
    if (max_len <= 0) return fail(IRIS_E_INVALID, "iris_flyby: max_len = %d must be positive", max_len);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_flyby: n_src = %d > 65535", n_src);
    const unsigned tiles = (unsigned)(((long long)max_len + kFlybyTile - 1) / kFlybyTile);
    k_flyby<<<dim3(tiles, (unsigned)n_src), kFlybyThreads, 0, (hipStream_t)stream>>>(
        static_cast<const iris_flyby_src*>(table_dev), channels, max_len);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
