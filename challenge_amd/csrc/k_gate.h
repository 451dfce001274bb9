// k_gate.h -- activity gate of a waveform corpus: per frame, is the voice speaking?  Exact zeros are written elsewhere, so the
// mixers' label rule (a frame is active when any sample under its window is non-zero: k_mix_wave_frame_active, k_mix.h) means
// something on clips that come straight from a microphone.  A ragged set of waveforms in three launches.  Part of the single
// translation unit iris_frontend.hip.
//
// Per record: x [C, L], hop; h2 = hop / 2, T = 1 + L / hop (the mixers' frame count), owner(s) = min((s + h2) / hop, T - 1):
//   1. E[t] = sum_c sum_{owner(s) = t} (double)x[c, s]^2 in double                                        (k_gate_energy)
//   2. P = max of the E[t] that are not NaN (0 if none), thr = max(P * ratio, floor), m0[t] = E[t] >= thr && E[t] > 0
//   3. close: a run of zeros of m0 of length <= min_gap with a one on both sides becomes ones -> m1
//   4. drop:  a run of ones of m1 shorter than min_event becomes zeros -> m2
//   5. hang:  m[t] = OR of m2[u] over |u - t| <= hang                                           (2 .. 5: k_gate_mask)
//   6. y[c, s] = x[c, s] where m[owner(s)], +0.0f elsewhere                                              (k_gate_apply)
//
// k_gate_energy: blockIdx.y = record, one WAVE per frame (four frames per workgroup).  Lane l takes the quads l, l + 64, ... of
//   the frame's samples of every channel, counted from the frame's first sample, and adds the four squares of a quad in order;
//   a quad is one 16-byte load where its address allows and four 4-byte loads where it does not (rows of [C, L] are not
//   aligned in general), so the order of the sum - and with it every bit of E - does not depend on where the record lies.  The
//   squares are exact in double; the 64 partial sums are added by a butterfly, whose result is the same in every lane.
// k_gate_mask: one workgroup per record.  The peak is a maximum (exact in any order).  The masks are bit words in LDS, one
//   64-bit word per wave and step (`__ballot`); steps 3 - 5 ask for the nearest set (or clear) bit on either side of a frame,
//   found by walking words, no farther than the parameter of the step reaches.  Frames per record: at most kGateMaxFrames.
// k_gate_apply: blockIdx.y = record, four consecutive samples per thread and channel, 16 bytes at a time where both rows allow.
//   A sample is kept by selection, never multiplied: bit for bit.
// Every energy is read (launch 1) before anything is written (launch 3): dst == src gates in place.  No atomics, no
// workspace; every loop bound comes from the record: bitwise reproducible, and a record's result does not depend on the
// records around it.
#pragma once

constexpr int kGateThreads = 256;
constexpr int kGateMaxFrames = IRIS_GATE_MAX_FRAMES;   // 131072: two bit buffers of 16 KiB in LDS
constexpr int kGateWords = kGateMaxFrames / 64;

static_assert(sizeof(iris_gate_rec) == 40, "iris_gate_rec is 40 bytes: four pointers, the length and a pad");

// a record the kernels leave alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool gate_skip(const iris_gate_rec& d, int max_len) {
    return d.len <= 0 || d.len > max_len || !d.src || !d.dst || !d.mask || !d.energy;
}

__global__ __launch_bounds__(kGateThreads) void k_gate_energy(const iris_gate_rec* __restrict__ table, int channels, int hop,
                                                              int max_len) {
    const iris_gate_rec d = table[blockIdx.y];
    if (gate_skip(d, max_len)) return;
    const int L = d.len, T = 1 + L / hop, h2 = hop / 2, lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * (kGateThreads / 64) + (threadIdx.x >> 6);
    if (t >= T) return;   // (uniform in the wave)
    // the samples frame t owns: [t hop - h2, (t + 1) hop - h2), the last frame to the end of the clip
    const long long lo = max(t * hop - h2, 0LL);
    const long long hi = t == T - 1 ? (long long)L : min((t + 1) * hop - h2, (long long)L);
    const int n = (int)max(hi - lo, 0LL), quads = (n + 3) >> 2;
    double acc = 0.0;
    for (int c = 0; c < channels; ++c) {
        const float* row = d.src + (size_t)c * L + lo;
        const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;   // (uniform)
        for (int q = lane; q < quads; q += 64) {
            const int j = q * 4;
            float4 v;
            if (wide && j + 3 < n) {
                v = *reinterpret_cast<const float4*>(row + j);
            } else {   // (a sample beyond the frame adds +0.0: the sum is the same)
                v.x = row[j];
                v.y = j + 1 < n ? row[j + 1] : 0.f;
                v.z = j + 2 < n ? row[j + 2] : 0.f;
                v.w = j + 3 < n ? row[j + 3] : 0.f;
            }
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    }
    for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) d.energy[t] = acc;
}

// The nearest bit at or below frame t that is set (inv: clear), or -1 when the words down to the one of frame t - reach hold
// none.  What it returns may lie farther than `reach` away: `reach` only bounds the walk.
__device__ __forceinline__ int gate_prev(const unsigned long long* bits, bool inv, int t, int reach) {
    int w = t >> 6;
    unsigned long long x = (inv ? ~bits[w] : bits[w]) & (~0ULL >> (63 - (t & 63)));
    const int stop = (int)(max((long long)t - reach, 0LL) >> 6);
    while (!x && w > stop) {
        --w;
        x = inv ? ~bits[w] : bits[w];
    }
    return x ? (w << 6) + 63 - __clzll((long long)x) : -1;
}

// The nearest bit at or above frame t that is set (inv: clear), or T when the words up to the one of frame t + reach hold none
// (the bits of the last word beyond T are clear in every buffer: as clear bits they count as the end of the clip, T).
__device__ __forceinline__ int gate_next(const unsigned long long* bits, bool inv, int t, int reach, int T) {
    int w = t >> 6;
    unsigned long long x = (inv ? ~bits[w] : bits[w]) & (~0ULL << (t & 63));
    const int stop = (int)(min((long long)t + reach, (long long)T - 1) >> 6);
    while (!x && w < stop) {
        ++w;
        x = inv ? ~bits[w] : bits[w];
    }
    return x ? min((w << 6) + __ffsll((long long)x) - 1, T) : T;
}

__global__ __launch_bounds__(kGateThreads) void k_gate_mask(const iris_gate_rec* __restrict__ table, int hop, int min_gap,
                                                            int min_event, int hang, double ratio, double floor, int max_len) {
    __shared__ unsigned long long a[kGateWords], b[kGateWords];
    __shared__ double red[kGateThreads];
    const iris_gate_rec d = table[blockIdx.x];
    if (gate_skip(d, max_len)) return;
    const int T = 1 + d.len / hop;
    if (T > kGateMaxFrames) return;   // (refused on the host through max_len)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, words = (T + 63) >> 6;
    constexpr int kWaves = kGateThreads / 64;

    // ---- the peak over the energies that are not NaN (they are sums of squares: none is negative) ----
    double p = 0.0;
    for (int t = tid; t < T; t += kGateThreads) {
        const double e = d.energy[t];
        if (e > p) p = e;   // (false on NaN)
    }
    red[tid] = p;
    __syncthreads();
    for (int s = kGateThreads / 2; s; s >>= 1) {
        if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
        __syncthreads();
    }
    const double scaled = red[0] * ratio, thr = scaled > floor ? scaled : floor;

    // ---- m0 -> a ----
    for (int w = wave; w < words; w += kWaves) {
        const int t = (w << 6) + lane;
        bool on = false;
        if (t < T) {
            const double e = d.energy[t];
            on = e >= thr && e > 0.0;
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) a[w] = word;
    }
    __syncthreads();
    // ---- close: a -> b.  A zero is closed when the ones around it are no more than min_gap zeros apart ----
    for (int w = wave; w < words; w += kWaves) {
        const int t = (w << 6) + lane;
        bool on = false;
        if (t < T) {
            on = (a[w] >> lane) & 1;
            if (!on) {
                const int lo = gate_prev(a, false, t, min_gap), hi = gate_next(a, false, t, min_gap, T);
                on = lo >= 0 && hi < T && hi - lo - 1 <= min_gap;
            }
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) b[w] = word;
    }
    __syncthreads();
    // ---- drop: b -> a.  A one stays when its run, cut at the ends of the clip, has min_event frames ----
    for (int w = wave; w < words; w += kWaves) {
        const int t = (w << 6) + lane;
        bool on = false;
        if (t < T && ((b[w] >> lane) & 1)) {
            // (no zero found below: the ones reach frame 0, or farther down than min_event - either way t of them count)
            const int lo = gate_prev(b, true, t, min_event), hi = gate_next(b, true, t, min_event, T);
            const int left = lo >= 0 ? t - lo - 1 : t, right = hi - t - 1;
            on = (long long)left + right + 1 >= min_event;
        }
        const unsigned long long word = __ballot(on);
        if (lane == 0) a[w] = word;
    }
    __syncthreads();
    // ---- hang: a -> the mask ----
    for (int t = tid; t < T; t += kGateThreads) {
        const int lo = gate_prev(a, false, t, hang), hi = gate_next(a, false, t, hang, T);
        d.mask[t] = (lo >= 0 && t - lo <= hang) || (hi < T && hi - t <= hang) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kGateThreads) void k_gate_apply(const iris_gate_rec* __restrict__ table, int channels, int hop,
                                                             int max_len) {
    const iris_gate_rec d = table[blockIdx.y];
    if (gate_skip(d, max_len)) return;
    const int L = d.len, T = 1 + L / hop;
    const long long first = ((long long)blockIdx.x * kGateThreads + threadIdx.x) * 4;
    if (first >= L || T > kGateMaxFrames) return;
    const int s = (int)first, n = min(4, L - s);
    const unsigned h2 = (unsigned)hop / 2, last = (unsigned)T - 1;
    // (s + 3 + h2 < 2^31 + 2^30: no overflow in 32 bits)
    const unsigned o0 = min(((unsigned)s + h2) / (unsigned)hop, last), o3 = min(((unsigned)s + 3u + h2) / (unsigned)hop, last);
    bool keep[4];
    keep[0] = d.mask[o0] != 0;
    if (o3 == o0) {
        keep[1] = keep[2] = keep[3] = keep[0];
    } else {
        for (int k = 1; k < 4; ++k) keep[k] = d.mask[min(((unsigned)s + (unsigned)k + h2) / (unsigned)hop, last)] != 0;
    }
    for (int c = 0; c < channels; ++c) {
        const float* x = d.src + (size_t)c * L + s;   // (dst may be src: no __restrict__)
        float* y = d.dst + (size_t)c * L + s;
        if (n == 4 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
            float4 v = *reinterpret_cast<const float4*>(x);
            v.x = keep[0] ? v.x : 0.f;
            v.y = keep[1] ? v.y : 0.f;
            v.z = keep[2] ? v.z : 0.f;
            v.w = keep[3] ? v.w : 0.f;
            *reinterpret_cast<float4*>(y) = v;
        } else {
            for (int k = 0; k < n; ++k) y[k] = keep[k] ? x[k] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int iris_activity_gate(const void* table_dev, int n, int channels, int hop, int min_gap, int min_event, int hang,
                                  double ratio, double floor, int max_len, void* stream) {
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_activity_gate: table is NULL");
    if (n <= 0) return fail(IRIS_E_INVALID, "iris_activity_gate: n = %d must be positive", n);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_activity_gate: channels = %d must be positive", channels);
    if (hop < 1 || min_gap < 0 || min_event < 1 || hang < 0)
        return fail(IRIS_E_INVALID, "iris_activity_gate: hop %d >= 1, min_gap %d >= 0, min_event %d >= 1, hang %d >= 0 do not all hold",
                    hop, min_gap, min_event, hang);
    if (!(ratio > 0.0 && ratio < 1.0))
        return fail(IRIS_E_INVALID, "iris_activity_gate: ratio = %g is outside (0, 1): it is 10^(-range_db / 10)", ratio);
    if (!(floor >= 0.0)) return fail(IRIS_E_INVALID, "iris_activity_gate: floor = %g must be >= 0", floor);
    if (max_len <= 0) return fail(IRIS_E_INVALID, "iris_activity_gate: max_len = %d must be positive", max_len);
    if (n > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_activity_gate: n = %d > 65535", n);
    const int max_frames = 1 + max_len / hop;
    if (max_frames > kGateMaxFrames)
        return fail(IRIS_E_UNSUPPORTED, "iris_activity_gate: %d samples at hop %d are %d frames (> %d)", max_len, hop, max_frames,
                    kGateMaxFrames);
    const iris_gate_rec* table = static_cast<const iris_gate_rec*>(table_dev);
    hipStream_t s = (hipStream_t)stream;
    constexpr int kWaves = kGateThreads / 64;
    k_gate_energy<<<dim3((unsigned)((max_frames + kWaves - 1) / kWaves), (unsigned)n), kGateThreads, 0, s>>>(table, channels, hop,
                                                                                                              max_len);
    HIP_TRY(hipGetLastError());
    k_gate_mask<<<dim3((unsigned)n), kGateThreads, 0, s>>>(table, hop, min_gap, min_event, hang, ratio, floor, max_len);
    HIP_TRY(hipGetLastError());
    const unsigned tiles = (unsigned)(((long long)max_len + kGateThreads * 4 - 1) / (kGateThreads * 4));
    k_gate_apply<<<dim3(tiles, (unsigned)n), kGateThreads, 0, s>>>(table, channels, hop, max_len);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
