// k_speed.h -- speed perturbation of a waveform corpus (Ko et al. 2015; Kaldi's 0.9 / 1.0 / 1.1): a batched band-limited
// resampler over a ragged set of waveforms, each at its own real-valued rate, in one launch - and the frame activity of the
// results in one more.  Part of the single translation unit iris_frontend.hip.
//
// Per source: x [C, L], rate r > 0 (r > 1 = faster and shorter), output y [C, n] with n = ceil(L / r).  Output sample m sits at
// pos = (double)m * r: i0 = floor(pos), frac = (float)(pos - i0), and
//     y[c, m] = sum_s x[c, s] * cut * g(cut * ((s - i0) - frac)),      cut = 0.99 * min(1, 1 / r),
//     g(t)    = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,     x[c, s] = 0 outside [0, L)
// - the Hann-windowed sinc of torchaudio.functional.resample (width 6, rolloff 0.99) at a real-valued position; for a rational
// r = o / n it is the polyphase filter of k_resample.h, without a host-built tap table.
//   blockIdx.y = source, blockIdx.x = a tile of kSpeedTile consecutive output samples; the 256-thread workgroup handles all
//   channels of its tile:
//   1. the input samples the tile needs are one contiguous span per channel, [i0(first) - H, i0(last) + H + 1] with
//      H = ceil(6 / cut) (7 at rate 1, 8 at 1.2): staged into LDS coalesced, 16 bytes per lane where the rows are aligned,
//      zeros outside [0, L) (a span too long for the buffer - rates far above 2, many channels - is read from global memory
//      instead);
//   2. neighbouring threads take neighbouring output samples: their LDS reads sit r words apart, their stores are coalesced.
//      The taps of a sample are evaluated on the fly with sinf / cosf per tap (no recurrence: every tap is an independent
//      function of its own argument) and shared by a pair of channels; the sum runs in ascending s.
// A fixed sequence of fp32 operations per value (the position alone is fp64) that does not depend on the tile or on the
// staging: bitwise reproducible, a batch equals the single calls.  No atomics, no workspace, no synchronisation; every loop
// bound comes from the descriptor.  r == 1 copies the source bit for bit.
#pragma once

constexpr int kSpeedThreads = 256;
constexpr int kSpeedTile = 1024;    // output samples per workgroup (4 per thread)
constexpr int kSpeedLds = 8192;     // floats of input spans held in LDS (32 KiB): stereo up to rate ~3.9

static_assert(sizeof(iris_speed_src) == 32, "iris_speed_src is 32 bytes: two pointers, two ints, one double");

// a record the kernels leave alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool speed_skip(const iris_speed_src& d, int max_out_len) {
    return d.len_in <= 0 || d.len_out <= 0 || d.len_out > max_out_len || !(d.rate > 0.0) || !d.src || !d.dst;
}

// the output samples m_beg, m_beg + 256, ... < m_end of every channel; x[c * stride + s - base] is sample s of channel c (the staged
// span, which holds zeros outside the source, or the source itself): one body, inlined once per address space
__device__ __forceinline__ void speed_tile(const float* x, size_t stride, long long base, float* __restrict__ dst,
                                           int L, int n, int channels, int m_beg, int m_end, double r, float cut, long long H) {
    for (int m = m_beg; m < m_end; m += kSpeedThreads) {
        const double pos = (double)m * r;
        const double fl = floor(pos);
        const long long i0 = (long long)fl;
        const float frac = (float)(pos - fl);
        // taps outside the source multiply zeros: skipped (the sum is the same)
        const int s_beg = (int)max(i0 - H, 0LL), s_end = (int)min(i0 + H + 1, (long long)L - 1);
        for (int c0 = 0; c0 < channels; c0 += 2) {
            const bool two = c0 + 1 < channels;
            const float* x0 = x + (size_t)c0 * stride;
            const float* x1 = two ? x0 + stride : x0;
            float acc0 = 0.f, acc1 = 0.f;
            for (int s = s_beg; s <= s_end; ++s) {
                const float t = cut * ((float)(s - i0) - frac);
                if (fabsf(t) < 6.f) {
                    const float pt = 3.14159274101257324f * t;
                    const float sinc = pt == 0.f ? 1.f : sinf(pt) / pt;
                    const float cs = cosf(pt / 12.f);
                    const float tap = (cut * sinc) * (cs * cs);
                    acc0 += x0[(int)(s - base)] * tap;
                    acc1 += x1[(int)(s - base)] * tap;
                }
            }
            dst[(size_t)c0 * n + m] = acc0;
            if (two) dst[(size_t)(c0 + 1) * n + m] = acc1;
        }
    }
}

__global__ __launch_bounds__(kSpeedThreads) void k_speed_perturb(const iris_speed_src* __restrict__ table, int channels,
                                                                 int max_out_len) {
    __shared__ __attribute__((aligned(16))) float span[kSpeedLds];
    const iris_speed_src d = table[blockIdx.y];
    if (speed_skip(d, max_out_len)) return;
    const int L = d.len_in, n = d.len_out, tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * kSpeedTile;
    if (m0 >= n) return;
    const int m_end = (int)min(m0 + kSpeedTile, (long long)n);   // one past the tile's last output sample
    const double r = d.rate;
    const float* __restrict__ src = d.src;
    float* __restrict__ dst = d.dst;
    if (r == 1.0) {   // the identity: a copy (n == L)
        for (int c = 0; c < channels; ++c)
            for (int m = (int)m0 + tid; m < min(m_end, L); m += kSpeedThreads) dst[(size_t)c * n + m] = src[(size_t)c * L + m];
        return;
    }
    const double cut_d = 0.99 * fmin(1.0, 1.0 / r);
    const float cut = (float)cut_d;
    const long long H = (long long)fmin(ceil(6.0 / cut_d), 4.0e9);   // taps of a sample: s = i0 - H .. i0 + H + 1

    // ---- the input span of the tile, from a multiple of 4 samples (so that 16-byte loads and LDS writes line up) ----
    const long long lo = ((long long)floor((double)m0 * r) - H) & ~3LL;
    const long long hi = (long long)floor((double)(m_end - 1) * r) + H + 1;
    const long long len4 = (hi - lo + 4) & ~3LL;                      // floats per channel in LDS, a multiple of 4
    const bool staged = len4 * channels <= (long long)kSpeedLds;      // (uniform)
    if (staged) {
        const int quads = (int)(len4 >> 2);
        const bool rows16 = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // every channel row starts on 16 bytes
        for (int q = tid; q < quads * channels; q += kSpeedThreads) {
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

    if (staged) speed_tile(span, (size_t)len4, lo, dst, L, n, channels, (int)m0 + tid, m_end, r, cut, H);
    else speed_tile(src, (size_t)L, 0, dst, L, n, channels, (int)m0 + tid, m_end, r, cut, H);
}

// active[i][t] = 1 when any sample under the support of frame t's periodic-Hann window is non-zero in any channel of the
// waveform table[i].dst [C, len_out]: k_mix_wave_frame_active (k_mix.h) for every record of the table in one launch
__global__ __launch_bounds__(256) void k_mix_wave_frame_active_batch(const iris_speed_src* __restrict__ table,
                                                                     float* const* __restrict__ active, int channels, int n_fft,
                                                                     int hop, int max_frames) {
    const iris_speed_src d = table[blockIdx.y];
    float* out = active[blockIdx.y];
    const int len = d.len_out, t = blockIdx.x;
    if (len <= 0 || !d.dst || !out) return;
    const int n_frames = 1 + len / hop;
    if (n_frames > max_frames || t >= n_frames) return;   // (uniform)
    const long long centre = (long long)t * hop;
    const int lo = (int)max(centre - n_fft / 2 + 1, 0LL), hi = (int)min(centre + n_fft / 2 - 1, (long long)len - 1);
    int any = 0;
    for (int c = 0; c < channels; ++c)
        for (int i = lo + (int)threadIdx.x; i <= hi; i += blockDim.x) any |= d.dst[(size_t)c * len + i] != 0.f;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) out[t] = any ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" long long iris_speed_len(long long len, double rate) {
    if (len <= 0 || !(rate > 0.0) || !std::isfinite(rate)) return 0;
    return (long long)std::ceil((double)len / rate);
}

extern "C" int iris_speed_perturb(const void* table_dev, int n_src, int channels, int max_out_len, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_speed_perturb: n_src = %d is negative", n_src);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_speed_perturb: channels = %d must be positive", channels);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_speed_perturb: table is NULL");
    if (max_out_len <= 0) return fail(IRIS_E_INVALID, "iris_speed_perturb: max_out_len = %d must be positive", max_out_len);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_speed_perturb: n_src = %d > 65535", n_src);
    const unsigned tiles = (unsigned)(((long long)max_out_len + kSpeedTile - 1) / kSpeedTile);
    k_speed_perturb<<<dim3(tiles, (unsigned)n_src), kSpeedThreads, 0, (hipStream_t)stream>>>(
        static_cast<const iris_speed_src*>(table_dev), channels, max_out_len);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_mix_wave_frame_active_batch(const void* table_dev, int n_src, int channels, int n_fft, int hop,
                                                const void* active_ptrs_dev, int max_frames, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_mix_wave_frame_active_batch: n_src = %d is negative", n_src);
    if (channels <= 0 || n_fft <= 1 || hop <= 0)
        return fail(IRIS_E_INVALID, "iris_mix_wave_frame_active_batch: bad sizes (%d channels, n_fft %d, hop %d)", channels, n_fft,
                    hop);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev || !active_ptrs_dev) return fail(IRIS_E_INVALID, "iris_mix_wave_frame_active_batch: NULL argument");
    if (max_frames <= 0)
        return fail(IRIS_E_INVALID, "iris_mix_wave_frame_active_batch: max_frames = %d must be positive", max_frames);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_mix_wave_frame_active_batch: n_src = %d > 65535", n_src);
    k_mix_wave_frame_active_batch<<<dim3((unsigned)max_frames, (unsigned)n_src), 256, 0, (hipStream_t)stream>>>(
        static_cast<const iris_speed_src*>(table_dev), static_cast<float* const*>(active_ptrs_dev), channels, n_fft, hop,
        max_frames);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
