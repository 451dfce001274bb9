// k_fft_fir.h -- reverberation with LONG impulse responses (up to 32768 taps, 2 s at 16 kHz): a uniformly partitioned
// overlap-save convolution of a ragged set of waveforms on the wave-per-frame FFT core (iris_fft.h), two launches.  Part of
// the single translation unit iris_frontend.hip.
//
// One fixed geometry: block B = 1024 new samples, transform N = 2048 (the largest the core has).  Per record x [C, L],
// h [C, K] (rows K floats apart, or `tap_pitch` apart), y [C, L] = the causal convolution cut at the input length (k_fir.h's
// definition):  y[c, m] = sum_{k < K, k <= m} h[c, k] x[c, m - k].  With nblk = ceil(L / B) and P = ceil(K / B):
//   input frame j   (0 <= j < nblk) = x[(j - 1) B, (j + 1) B), zero before sample 0 and from L on
//   tap partition p (0 <= p < P)    = h[p B, (p + 1) B) followed by B zeros
//   y[j B + i]      = IFFT( sum_{p = 0}^{min(P - 1, j)} FFT(frame_{j - p}) FFT(part_p) )[B + i]          (0 <= i < B)
//   (a) k_fft_fir_spectra: one wave per frame or partition: load (zeros outside the row), the packed real transform
//       (NC = 1024 complex points in registers, the untangle of spectrum.h), and the spectrum into the record's slice of the
//       workspace in LANE ORDER: float4 slot q * 64 + lane holds (X[k], X[NC - k]) with k = lane + 64 q, q < 8; slot 512
//       (first half) holds X[NC / 2].  X[0] and X[NC] are real and sit in lane 0's slot 0.  kFfSpec = 1032 complex = 8256
//       bytes per spectrum; the product is bin by bin, so no natural order is ever needed;
//   (b) k_fft_fir_apply: one wave per (record, channel, output block j): every lane accumulates its 17 bins in registers in
//       ascending p (two FMAs per component, a fixed order), folds them back into the packed spectrum Z (its own bin k and the
//       partner NC - k come from the same lane: Z[NC - k] = conj(E) + i conj(O) where Z[k] = E + i O; one LDS exchange puts
//       the partners into their lanes), inverts as k_istft.h does - conj, the forward core, conj - and stores the last B
//       samples of the frame, cut at L.
// Workspace of a record: C (nblk + P) spectra (iris_fft_fir_workspace), at the record's own `ws_off`.  No atomics, no
// dependence on the neighbours, a summation order fixed by (j, p) alone: bitwise reproducible, a batch equals the single
// calls, an all-zero voice gives 0.  Both launches are capturable once the twiddles of the device are resident (the first
// call on a device uploads them: make that call outside any capture).
// Against the float64 convolution the error is norm-wise per output block, not tap by tap:
//     |y - ref| <= C u R[c, m],   u = 2^-24,   R = sum_{p <= j} ||frame_{j - p}||_2 ||part_p||_2,   j = m / B
// (DESIGN.md K2f for C and how it was measured).
#pragma once
#include <mutex>

constexpr int kFfBlock = 1024;          // B: new samples per frame
constexpr int kFfLog2N = 11;            // N = 2048
constexpr int kFfN = 1 << kFfLog2N, kFfNC = kFfN / 2, kFfP = FftCfg<kFfLog2N>::P, kFfNTW = FftCfg<kFfLog2N>::NTW;
constexpr int kFfSpec = kFfNC + 8;      // complex slots per stored spectrum (slot NC: the bin NC / 2; 64-byte multiple)
constexpr int kFfWaves = 4;             // waves (frames, output blocks) per workgroup
constexpr int kFfMaxTaps = 32768;       // IRIS_FFT_FIR_MAX_TAPS
constexpr int kFfConsts = kFfNTW + kFfP / 2;   // per-lane constants: the core's twiddles, then the untangle twiddles
constexpr int kFfWaveBuf = (lds_padded(kFfNC, FftCfg<kFfLog2N>::PMMAX) + 1) & ~1;   // complex slots of a wave's exchange buffer

static_assert(sizeof(iris_fft_fir_src) == 40, "iris_fft_fir_src is 40 bytes: three pointers, two ints, one 64-bit offset");
static_assert(IRIS_FFT_FIR_MAX_TAPS == kFfMaxTaps, "the header's limit");
static_assert(kFfP == 16 && kFfBlock * 2 == kFfN, "overlap-save with half-frame blocks, 16 points per lane");
static_assert(untangle_pm(kFfLog2N) == 1, "the fold-back exchange uses the untangle's padding");

__host__ __device__ inline long long fft_fir_blocks(long long n) { return (n + kFfBlock - 1) / kFfBlock; }
// bytes of workspace of one well-formed record
__host__ __device__ inline long long fft_fir_bytes(int channels, int len, int n_taps) {
    return (long long)channels * (fft_fir_blocks(len) + fft_fir_blocks(n_taps)) * kFfSpec * (long long)sizeof(cf);
}

// a record the kernels leave alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool fft_fir_skip(const iris_fft_fir_src& d, int channels, int max_len, int max_taps, long long ws_bytes) {
    if (d.len <= 0 || d.n_taps <= 0 || d.len > max_len || d.n_taps > max_taps || !d.src || !d.dst || !d.taps) return true;
    if (d.ws_off < 0 || (d.ws_off & 15) || d.ws_off > ws_bytes) return true;
    return fft_fir_bytes(channels, d.len, d.n_taps) > ws_bytes - d.ws_off;
}

__device__ __forceinline__ void fft_fir_consts(const cf* __restrict__ consts, int lane, cf (&tw)[kFfNTW], cf (&post)[kFfP / 2]) {
#pragma unroll
    for (int i = 0; i < kFfNTW; ++i) tw[i] = consts[i * kWave + lane];
#pragma unroll
    for (int i = 0; i < kFfP / 2; ++i) post[i] = consts[(kFfNTW + i) * kWave + lane];
}

// acc += a * b in a fixed order: two FMAs per component
__device__ __forceinline__ cf fft_fir_cmac(cf acc, cf a, cf b) {
    acc = __builtin_elementwise_fma(a.xx, b, acc);
    return __builtin_elementwise_fma(a.yy, mk(-b.y, b.x), acc);
}

// ---- (a) spectra of the input frames and of the tap partitions ----
__global__ __launch_bounds__(64 * kFfWaves) void k_fft_fir_spectra(const iris_fft_fir_src* __restrict__ table,
                                                                   const cf* __restrict__ consts, int channels, int max_len,
                                                                   int max_taps, int tap_pitch, char* __restrict__ ws,
                                                                   long long ws_bytes) {
    __shared__ __attribute__((aligned(16))) cf smem[kFfWaves * kFfWaveBuf];
    const iris_fft_fir_src d = table[blockIdx.z];
    if (fft_fir_skip(d, channels, max_len, max_taps, ws_bytes)) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nblk = (int)fft_fir_blocks(d.len), npart = (int)fft_fir_blocks(d.n_taps);
    const int f = (int)blockIdx.x * kFfWaves + wv;   // frames first, then partitions
    if (f >= nblk + npart) return;                   // (wave-uniform; the kernel has no workgroup barrier)
    const int c = blockIdx.y;
    const bool is_x = f < nblk;
    const float* __restrict__ row = is_x ? d.src + (size_t)c * d.len : d.taps + (size_t)c * (tap_pitch ? tap_pitch : d.n_taps);
    const long long start = is_x ? (long long)(f - 1) * kFfBlock : (long long)(f - nblk) * kFfBlock;
    const int n = is_x ? d.len : d.n_taps;
    const int span = is_x ? kFfN : kFfBlock;         // samples of the frame that may be non-zero

    cf x[kFfP];
    const bool whole = start >= 0 && start + span <= n && (reinterpret_cast<uintptr_t>(row + start) & 7) == 0;
    if (whole) {   // wave-uniform
        const cf* p = reinterpret_cast<const cf*>(row + start);
#pragma unroll
        for (int q = 0; q < kFfP; ++q) x[q] = (2 * kWave * q < span) ? p[lane + kWave * q] : mk(0.f, 0.f);
    } else {
#pragma unroll
        for (int q = 0; q < kFfP; ++q) {
            const int i = 2 * (lane + kWave * q);
            const long long s = start + i;
            const float v0 = (i < span && s >= 0 && s < n) ? row[s] : 0.f;
            const float v1 = (i + 1 < span && s + 1 >= 0 && s + 1 < n) ? row[s + 1] : 0.f;
            x[q] = mk(v0, v1);
        }
    }

    cf tw[kFfNTW], post[kFfP / 2];
    fft_fir_consts(consts, lane, tw, post);
    cf* lds = smem + wv * kFfWaveBuf;
    fft_frame<kFfLog2N>(x, tw, lds, lane);
    cf xlo[kFfP / 2], xhi[kFfP / 2];
    untangle<kFfLog2N, true, true>(x, post, lds, lane, xlo, xhi);

    const long long spec = is_x ? (long long)c * nblk + f : (long long)channels * nblk + (long long)c * npart + (f - nblk);
    cf* out = reinterpret_cast<cf*>(ws + d.ws_off) + spec * kFfSpec;
    float4* out4 = reinterpret_cast<float4*>(out);
#pragma unroll
    for (int q = 0; q < kFfP / 2; ++q) out4[q * kWave + lane] = make_float4(xlo[q].x, xlo[q].y, xhi[q].x, xhi[q].y);
    if (lane == 0) out[kFfNC] = mk(x[kFfP / 2].x, -x[kFfP / 2].y);   // X[NC / 2] = conj Z[NC / 2]
}

// ---- (b) the products summed over the partitions, the inverse transform, the block's outputs ----
__global__ __launch_bounds__(64 * kFfWaves) void k_fft_fir_apply(const iris_fft_fir_src* __restrict__ table,
                                                                 const cf* __restrict__ consts, int channels, int max_len,
                                                                 int max_taps, const char* __restrict__ ws, long long ws_bytes) {
    __shared__ __attribute__((aligned(16))) cf smem[kFfWaves * kFfWaveBuf];
    const iris_fft_fir_src d = table[blockIdx.z];
    if (fft_fir_skip(d, channels, max_len, max_taps, ws_bytes)) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nblk = (int)fft_fir_blocks(d.len), npart = (int)fft_fir_blocks(d.n_taps);
    const int j = (int)blockIdx.x * kFfWaves + wv;
    if (j >= nblk) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const int c = blockIdx.y, L = d.len;
    const cf* base = reinterpret_cast<const cf*>(ws + d.ws_off);
    const cf* xs = base + (long long)c * nblk * kFfSpec;
    const cf* hs = base + ((long long)channels * nblk + (long long)c * npart) * kFfSpec;

    cf lo[kFfP / 2], hi[kFfP / 2], mid = mk(0.f, 0.f);
#pragma unroll
    for (int q = 0; q < kFfP / 2; ++q) lo[q] = hi[q] = mk(0.f, 0.f);
    const int p_end = min(npart - 1, j);
    for (int p = 0; p <= p_end; ++p) {
        const cf* xf = xs + (long long)(j - p) * kFfSpec;
        const cf* hp = hs + (long long)p * kFfSpec;
        const float4* x4 = reinterpret_cast<const float4*>(xf) + lane;
        const float4* h4 = reinterpret_cast<const float4*>(hp) + lane;
#pragma unroll
        for (int q = 0; q < kFfP / 2; ++q) {
            const float4 a = x4[q * kWave], b = h4[q * kWave];
            lo[q] = fft_fir_cmac(lo[q], mk(a.x, a.y), mk(b.x, b.y));
            hi[q] = fft_fir_cmac(hi[q], mk(a.z, a.w), mk(b.z, b.w));
        }
        mid = fft_fir_cmac(mid, xf[kFfNC], hp[kFfNC]);   // one address for the wave
    }

    cf tw[kFfNTW], post[kFfP / 2];
    fft_fir_consts(consts, lane, tw, post);
    cf* lds = smem + wv * kFfWaveBuf;
    // conj(2 Z[k]) for the lane's own k = lane + 64 q, q < 8, and conj(2 Z[NC - k]) to its place in LDS
    cf x[kFfP];
    {
        cf* wp = lds + lds_pad<1>(kWave - lane);
#pragma unroll
        for (int q = 0; q < kFfP / 2; ++q) {
            const float ar = lo[q].x, br = hi[q].x;   // X[k], conj X[NC - k]
            float ai = lo[q].y, bi = -hi[q].y;
            if (q == 0 && lane == 0) ai = bi = 0.f;   // bins 0 and N / 2 are real by definition
            const float ex = ar + br, ey = ai + bi, dx = ar - br, dy = ai - bi;
            const float twr = post[q].x, twi = -post[q].y;                     // w^-k
            const float ox = dx * twr - dy * twi, oy = dx * twi + dy * twr;    // 2 O
            x[q] = mk(ex - oy, -(ey + ox));                                    // conj(2 E + 2 i O)
            wp[lds_pad<1>(kWave * (kFfP - 1 - q))] = mk(ex + oy, ey - ox);     // conj(conj(2 E) + i conj(2 O)); lane 0, q 0: slot NC, unused
        }
        if (lane == 0) lds[lds_pad<1>(kFfNC / 2)] = mk(2.f * mid.x, 2.f * mid.y);   // Z[NC / 2] = conj X[NC / 2]
        wave_sync_lds();
        const cf* rp = lds + lds_pad<1>(lane);
#pragma unroll
        for (int q = kFfP / 2; q < kFfP; ++q) x[q] = rp[lds_pad<1>(kWave * q)];
        wave_sync_lds();
    }
    fft_frame<kFfLog2N>(x, tw, lds, lane);

    // samples 2 m, 2 m + 1 of the frame, m = lane + 64 q; the last B of them are the block's outputs
    constexpr float inv_n = 1.0f / (float)kFfN;
    float* __restrict__ y = d.dst + (size_t)c * L;
    const long long m0 = (long long)j * kFfBlock;
    const bool y8 = (reinterpret_cast<uintptr_t>(y + m0) & 7) == 0;
#pragma unroll
    for (int q = kFfP / 2; q < kFfP; ++q) {
        const long long m = m0 + 2 * (lane + kWave * (q - kFfP / 2));
        const float v0 = x[q].x * inv_n, v1 = -x[q].y * inv_n;
        if (y8 && m + 1 < L) {
            *reinterpret_cast<cf*>(y + m) = mk(v0, v1);
        } else {
            if (m < L) y[m] = v0;
            if (m + 1 < L) y[m + 1] = v1;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the per-lane constants of N = 2048 ([kFfConsts][64] complex), built in double as a plan's are, resident once per device
static int fft_fir_device_consts(const cf** out) {
    static std::mutex mu;
    static cf* resident[64] = {};
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(IRIS_E_UNSUPPORTED, "iris_fft_fir_batch: device ordinal %d is outside 0 .. 63", dev);
    std::lock_guard<std::mutex> lock(mu);
    if (!resident[dev]) {
        std::vector<float2> tw, post, win;
        build_tables(kFfLog2N, tw, post, win);
        std::vector<float2> block;
        block.insert(block.end(), tw.begin(), tw.begin() + (size_t)kFfNTW * 64);
        block.insert(block.end(), post.begin(), post.begin() + (size_t)(kFfP / 2) * 64);
        float2* dptr = nullptr;
        const int rc = upload(&dptr, block);
        if (rc) {
            if (dptr) (void)hipFree(dptr);
            return rc;
        }
        resident[dev] = reinterpret_cast<cf*>(dptr);
    }
    *out = resident[dev];
    return IRIS_OK;
}

extern "C" long long iris_fft_fir_workspace(int channels, int len, int n_taps) {
    if (channels <= 0 || len <= 0 || n_taps <= 0 || n_taps > kFfMaxTaps) return 0;
    return fft_fir_bytes(channels, len, n_taps);
}

extern "C" int iris_fft_fir_batch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, int tap_pitch,
                                  void* workspace, long long workspace_bytes, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: n_src = %d is negative", n_src);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: channels = %d must be positive", channels);
    if (tap_pitch < 0) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: tap_pitch = %d is negative", tap_pitch);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: table is NULL");
    if (max_len <= 0) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: max_len = %d must be positive", max_len);
    if (max_taps <= 0) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: max_taps = %d must be positive", max_taps);
    if (tap_pitch && tap_pitch < max_taps)
        return fail(IRIS_E_INVALID, "iris_fft_fir_batch: tap_pitch = %d is below max_taps = %d", tap_pitch, max_taps);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_fft_fir_batch: n_src = %d > 65535", n_src);
    if (channels > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_fft_fir_batch: channels = %d > 65535", channels);
    if (max_taps > kFfMaxTaps) return fail(IRIS_E_UNSUPPORTED, "iris_fft_fir_batch: max_taps = %d > %d", max_taps, kFfMaxTaps);
    if (!workspace) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: workspace is NULL");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(IRIS_E_INVALID, "iris_fft_fir_batch: workspace is not 16-byte aligned");
    // the smallest record there can be: one channel row of one frame and one partition
    if (workspace_bytes < fft_fir_bytes(channels, 1, 1))
        return fail(IRIS_E_INVALID, "iris_fft_fir_batch: workspace of %lld bytes is below the %lld of the smallest record",
                    workspace_bytes, fft_fir_bytes(channels, 1, 1));
    const cf* consts = nullptr;
    const int rc = fft_fir_device_consts(&consts);
    if (rc) return rc;
    const unsigned blocks = (unsigned)fft_fir_blocks(max_len), parts = (unsigned)fft_fir_blocks(max_taps);
    const iris_fft_fir_src* table = static_cast<const iris_fft_fir_src*>(table_dev);
    k_fft_fir_spectra<<<dim3((blocks + parts + kFfWaves - 1) / kFfWaves, (unsigned)channels, (unsigned)n_src), 64 * kFfWaves, 0,
                        (hipStream_t)stream>>>(table, consts, channels, max_len, max_taps, tap_pitch, static_cast<char*>(workspace),
                                               workspace_bytes);
    HIP_TRY(hipGetLastError());
    k_fft_fir_apply<<<dim3((blocks + kFfWaves - 1) / kFfWaves, (unsigned)channels, (unsigned)n_src), 64 * kFfWaves, 0,
                      (hipStream_t)stream>>>(table, consts, channels, max_len, max_taps, static_cast<const char*>(workspace),
                                             workspace_bytes);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
