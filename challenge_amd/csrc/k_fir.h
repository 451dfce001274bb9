// k_fir.h -- reverberation of a waveform corpus (Ko et al. 2017; Kaldi's reverberate_data_dir): a batched direct-form FIR over a
// ragged set of waveforms, each channel with its own taps, in one launch.  Part of the single translation unit
// iris_frontend.hip.
//
// Per record: x [C, L], h [C, K] (rows K floats apart, or `tap_pitch` apart: what k_ism_rir writes), output y [C, L] (the causal convolution cut at the input length: the direct sound sits at
// tap 0 and what rings past the end of the voice is dropped, so lengths and frame counts do not move):
//     y[c, m] = sum_{k = 0}^{K - 1} h[c, k] * x[c, m - k],      x[c, i] = 0 for i < 0
//   blockIdx.z = record, blockIdx.y = channel, blockIdx.x = a tile of kFirTile consecutive output samples.  The 256-thread
//   workgroup walks the taps in chunks of kFirChunk:
//   1. the chunk's taps and the kFirChunk + kFirTile input samples under them are staged into LDS coalesced, 16 bytes per
//      lane where the row is aligned and whole (a scalar path otherwise), zeros outside [0, L) and beyond K;
//   2. every thread owns two groups of 4 consecutive outputs (group t and group t + 256 of the tile) and keeps, per group, a
//      sliding pair of 16-byte input windows in registers: a step of 4 taps reads the 4 taps (one address for the whole
//      workgroup: a broadcast) and the next window of each group (neighbouring lanes read neighbouring 16-byte slots:
//      conflict-free) and issues 32 FMAs, which the compiler pairs into 16 packed ones.
//   LDS: 12 KiB of samples + 4 KiB of taps = 16 KiB per workgroup; at 52 VGPRs the 32 wave slots of a CU hold 8 workgroups,
//   128 KiB of its 160 KiB.  Taps above the tile's last sample meet only x = 0 and are not visited.
// One fp32 FMA chain per output in ascending k, started from -0 (the first product passes through with its sign) and holding
// no term beyond K - 1: independent of the tile, the chunking and the neighbours, so the result is bitwise reproducible, a
// batch equals the single calls, and h = [1] copies the source bit for bit.  No atomics, no workspace, no synchronisation;
// every loop bound comes from the descriptor.
#pragma once

constexpr int kFirThreads = 256;
constexpr int kFirTile = 2048;     // output samples per workgroup (two groups of 4 per thread)
constexpr int kFirChunk = 1024;    // taps staged per pass
constexpr int kFirMaxTaps = 4096;  // what the Python surface accepts (the kernel itself takes any max_taps)

static_assert(sizeof(iris_fir_src) == 32, "iris_fir_src is 32 bytes: three pointers, two ints");
static_assert(kFirTile == 8 * kFirThreads && kFirChunk % 4 == 0 && kFirTile % 4 == 0, "two groups of 4 outputs per thread");

// a record the kernel leaves alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool fir_skip(const iris_fir_src& d, int max_len, int max_taps) {
    return d.len <= 0 || d.n_taps <= 0 || d.len > max_len || d.n_taps > max_taps || !d.src || !d.dst || !d.taps;
}

// floats row[i0 .. i0 + 3] with zeros outside [0, n): one 16-byte load where the row is aligned (i0 is a multiple of 4)
__device__ __forceinline__ float4 fir_load4(const float* __restrict__ row, long long i0, int n, bool row16) {
    float4 v;
    if (row16 && i0 >= 0 && i0 + 3 < n) {
        v = *reinterpret_cast<const float4*>(row + i0);
    } else {
        v.x = (i0 >= 0 && i0 < n) ? row[i0] : 0.f;
        v.y = (i0 + 1 >= 0 && i0 + 1 < n) ? row[i0 + 1] : 0.f;
        v.z = (i0 + 2 >= 0 && i0 + 2 < n) ? row[i0 + 2] : 0.f;
        v.w = (i0 + 3 >= 0 && i0 + 3 < n) ? row[i0 + 3] : 0.f;
    }
    return v;
}

// tap 4q + R of a step on one group: acc[j] += h * x[m_j - 4q - R], where a = x[m_0 - 4q .. + 3] and b = the 4 samples below
template <int R>
__device__ __forceinline__ void fir_tap(float (&acc)[4], float h, const float4& a, const float4& b) {
    const float w[8] = {b.x, b.y, b.z, b.w, a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(h, w[4 + j - R], acc[j]);
}

// `n` (1 .. 4, uniform) taps of one step
__device__ __forceinline__ void fir_step(float (&acc)[4], const float4& h, const float4& a, const float4& b, int n) {
    fir_tap<0>(acc, h.x, a, b);
    if (n > 1) fir_tap<1>(acc, h.y, a, b);
    if (n > 2) fir_tap<2>(acc, h.z, a, b);
    if (n > 3) fir_tap<3>(acc, h.w, a, b);
}

// tap_pitch: floats between the rows of a record's taps (0: the rows are dense, n_taps apart)
__global__ __launch_bounds__(kFirThreads) void k_fir_batch(const iris_fir_src* __restrict__ table, int max_len, int max_taps,
                                                           int tap_pitch) {
    __shared__ __attribute__((aligned(16))) float xs[kFirChunk + kFirTile];   // xs[i] = x[m0 - k0 - kFirChunk + i]
    __shared__ __attribute__((aligned(16))) float hs[kFirChunk];              // hs[i] = h[k0 + i]
    const iris_fir_src d = table[blockIdx.z];
    if (fir_skip(d, max_len, max_taps)) return;
    const int L = d.len, K = d.n_taps, tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * kFirTile;
    if (m0 >= L) return;
    const int tile = (int)min((long long)kFirTile, L - m0);          // outputs of this tile
    const int tile4 = (tile + 3) & ~3;
    const int k_end = (int)min((long long)K, m0 + tile);             // taps k >= m0 + tile meet x = 0 only
    const float* __restrict__ x = d.src + (size_t)blockIdx.y * L;
    const float* __restrict__ h = d.taps + (size_t)blockIdx.y * (tap_pitch ? tap_pitch : K);
    float* __restrict__ y = d.dst + (size_t)blockIdx.y * L;
    const bool x16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0, h16 = (reinterpret_cast<uintptr_t>(h) & 15) == 0;
    const bool y16 = (reinterpret_cast<uintptr_t>(y) & 15) == 0;

    const int g0 = 4 * tid, g1 = 4 * tid + kFirTile / 2;             // first output of the thread's two groups, within the tile
    const bool on0 = g0 < tile, on1 = g1 < tile;
    float acc0[4] = {-0.f, -0.f, -0.f, -0.f}, acc1[4] = {-0.f, -0.f, -0.f, -0.f};
    const float4* xs4 = reinterpret_cast<const float4*>(xs);
    const float4* hs4 = reinterpret_cast<const float4*>(hs);

    for (int k0 = 0; k0 < k_end; k0 += kFirChunk) {
        const int kc = min(kFirChunk, k_end - k0), kc4 = (kc + 3) & ~3;   // taps of this pass
        if (k0) __syncthreads();                                           // the previous pass has been read
        for (int i = 4 * tid; i < kc4; i += 4 * kFirThreads)
            *reinterpret_cast<float4*>(hs + i) = fir_load4(h, (long long)k0 + i, K, h16);
        const long long origin = m0 - k0 - kFirChunk;                     // a multiple of 4
        for (int i = kFirChunk - kc4 + 4 * tid; i < kFirChunk + tile4; i += 4 * kFirThreads)
            *reinterpret_cast<float4*>(xs + i) = fir_load4(x, origin + i, L, x16);
        __syncthreads();

        const int full = kc >> 2, rest = kc & 3;
        if (on0) {
            const int s0 = (kFirChunk + g0) >> 2, s1 = (kFirChunk + g1) >> 2;   // slots of the windows at tap k0
            float4 a0 = xs4[s0], a1 = on1 ? xs4[s1] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (on1) {
#pragma unroll 1
                for (int q = 0; q < full; ++q) {
                    const float4 t = hs4[q], b0 = xs4[s0 - q - 1], b1 = xs4[s1 - q - 1];
                    fir_step(acc0, t, a0, b0, 4);
                    fir_step(acc1, t, a1, b1, 4);
                    a0 = b0, a1 = b1;
                }
                if (rest) {
                    const float4 t = hs4[full];
                    fir_step(acc0, t, a0, xs4[s0 - full - 1], rest);
                    fir_step(acc1, t, a1, xs4[s1 - full - 1], rest);
                }
            } else {
#pragma unroll 1
                for (int q = 0; q < full; ++q) {
                    const float4 t = hs4[q], b0 = xs4[s0 - q - 1];
                    fir_step(acc0, t, a0, b0, 4);
                    a0 = b0;
                }
                if (rest) fir_step(acc0, hs4[full], a0, xs4[s0 - full - 1], rest);
            }
        }
    }

    // ---- the tile's outputs: 16 bytes per lane where the row is aligned and the group is whole ----
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int g = half ? g1 : g0;
        const float (&acc)[4] = half ? acc1 : acc0;
        if (g >= tile) continue;
        float* out = y + m0 + g;
        if (y16 && g + 3 < tile) {
            *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (g + j < tile) out[j] = acc[j];
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int fir_batch_launch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, int tap_pitch, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_fir_batch: n_src = %d is negative", n_src);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_fir_batch: channels = %d must be positive", channels);
    if (tap_pitch < 0) return fail(IRIS_E_INVALID, "iris_fir_batch: tap_pitch = %d is negative", tap_pitch);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_fir_batch: table is NULL");
    if (max_len <= 0) return fail(IRIS_E_INVALID, "iris_fir_batch: max_len = %d must be positive", max_len);
    if (max_taps <= 0) return fail(IRIS_E_INVALID, "iris_fir_batch: max_taps = %d must be positive", max_taps);
    if (tap_pitch && tap_pitch < max_taps)
        return fail(IRIS_E_INVALID, "iris_fir_batch: tap_pitch = %d is below max_taps = %d", tap_pitch, max_taps);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_fir_batch: n_src = %d > 65535", n_src);
    if (channels > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_fir_batch: channels = %d > 65535", channels);
    const unsigned tiles = (unsigned)(((long long)max_len + kFirTile - 1) / kFirTile);
    k_fir_batch<<<dim3(tiles, (unsigned)channels, (unsigned)n_src), kFirThreads, 0, (hipStream_t)stream>>>(
        static_cast<const iris_fir_src*>(table_dev), max_len, max_taps, tap_pitch);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_fir_batch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, void* stream) {
    return fir_batch_launch(table_dev, n_src, channels, max_len, max_taps, 0, stream);
}

extern "C" int iris_fir_batch_pitch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, int tap_pitch,
                                    void* stream) {
    return fir_batch_launch(table_dev, n_src, channels, max_len, max_taps, tap_pitch, stream);
}
