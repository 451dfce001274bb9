// k_curves.h -- the per-class score histogram split by label, the one primitive behind the threshold-free validation numbers
// (ROC-AUC, average precision, best-F1 threshold, calibration error: host arithmetic on the counts, metrics.curve_metrics).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// counts[k][label][slot], int64, CUMULATIVE: slot = min(bins - 1, max(0, floor(p * bins))) for a non-NaN prediction p (bins a
// power of two: p * bins is exact in fp32, so "slot >= b" is the predicate p >= b / bins), slot `bins` for a NaN prediction;
// label = y_true >= 0.5f (a NaN label is negative).  Integer adds only: the result does not depend on the order, two runs give
// the same bits, and the counts of several ranks can be summed exactly.
//   * grid (x, y): y tiles the classes - kc classes per workgroup, as many as keep kc * 2 * (bins + 1) uint32 counters within
//     kCurveLdsBytes of LDS (one class at bins = 4096) - and x strides over the B * T frames;
//   * a workgroup walks its classes one after the other, every lane a frame: all lanes of a wave then count into the SAME
//     (class) table, and the two end slots 0 and bins - 1 - where sigmoid outputs pile up, the worst case for same-address
//     LDS atomics - are counted in four registers per lane, summed over the wave and added once per class;
//   * every other slot is one ds_add_u32; the flush adds the non-zero counters to the global int64 counts with vector atomics.
// A workgroup counts at most ceil(B * T / gridDim.x) + 256 < 2^31 frames: the uint32 counters cannot wrap.
// ---------------------------------------------------------------------------

constexpr int kCurveMaxK = 16;
constexpr int kCurveMinBins = 16;
constexpr int kCurveMaxBins = 4096;
constexpr int kCurveThreads = 256;
// frames per lane and class the grid is sized for.  A lane's frames are dependent load -> add steps, a workgroup more is one more
// zero-fill and flush of the tile: measured at 64 x 512 x 3, bins 1024 - 1: 8.6 us, 2: 7.7, 4: 8.9, 8: 12.2, 16: 18.0, 32: 30.0
constexpr int kCurveFramesPerLane = 2;
constexpr int kCurveMaxBlocksX = 1024;
constexpr int kCurveLdsBytes = 40 * 1024;  // >= 2 * (kCurveMaxBins + 1) * 4: one class always fits

__device__ __forceinline__ unsigned curve_wave_sum_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kCurveThreads) void k_score_hist(const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                                               int n_frames, int K, int bins, int kc,
                                                               unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned curve_lds[];   // [kc][2][bins + 1]
    const int row = bins + 1, lane = threadIdx.x & 63;
    const int k0 = blockIdx.y * kc, nk = min(kc, K - k0);
    const int n_slots = nk * 2 * row;
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) curve_lds[i] = 0u;
    __syncthreads();
    const float fb = (float)bins, top = (float)(bins - 1);
    const int stride = gridDim.x * blockDim.x;   // (<= 2^18)
    for (int kk = 0; kk < nk; ++kk) {
        unsigned* const tab = curve_lds + kk * 2 * row;
        const float* const yt = y_true + (k0 + kk);
        const float* const yp = y_pred + (k0 + kk);
        unsigned lo0 = 0u, lo1 = 0u, hi0 = 0u, hi1 = 0u;   // slots 0 and bins - 1, negative / positive frames
        // (64-bit frame index: n_frames + stride may pass 2^31)
        for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_frames; f += stride) {
            const float t = yt[(size_t)f * K], p = yp[(size_t)f * K];
            const bool pos = t >= 0.5f;   // (NaN: false)
            if (p != p) {
                atomicAdd(&tab[(pos ? row : 0) + bins], 1u);
                continue;
            }
            // floor, then the clamp in fp32 (+-inf and products beyond the int range never reach the conversion)
            const int slot = (int)fminf(fmaxf(floorf(p * fb), 0.f), top);
            if (slot == 0) {
                lo0 += pos ? 0u : 1u;
                lo1 += pos ? 1u : 0u;
            } else if (slot == bins - 1) {
                hi0 += pos ? 0u : 1u;
                hi1 += pos ? 1u : 0u;
            } else {
                atomicAdd(&tab[(pos ? row : 0) + slot], 1u);
            }
        }
        lo0 = curve_wave_sum_u32(lo0);
        lo1 = curve_wave_sum_u32(lo1);
        hi0 = curve_wave_sum_u32(hi0);
        hi1 = curve_wave_sum_u32(hi1);
        if (lane == 0) {
            if (lo0) atomicAdd(&tab[0], lo0);
            if (lo1) atomicAdd(&tab[row], lo1);
            if (hi0) atomicAdd(&tab[bins - 1], hi0);
            if (hi1) atomicAdd(&tab[row + bins - 1], hi1);
        }
    }
    __syncthreads();
    unsigned long long* const out = counts + (size_t)k0 * 2 * row;   // this tile's classes are contiguous in [K][2][bins + 1]
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
        const unsigned v = curve_lds[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
}

extern "C" int iris_score_hist(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes, int bins,
                               long long* counts, void* stream) {
    if (!y_true || !y_pred || !counts) return fail(IRIS_E_INVALID, "iris_score_hist: NULL y_true / y_pred / counts");
    if (batch < 1 || n_time < 1 || n_classes < 1)
        return fail(IRIS_E_INVALID, "iris_score_hist: batch %d, T %d, K %d", batch, n_time, n_classes);
    if (n_classes > kCurveMaxK) return fail(IRIS_E_UNSUPPORTED, "iris_score_hist: K %d (<= %d)", n_classes, kCurveMaxK);
    if (bins < kCurveMinBins || bins > kCurveMaxBins || (bins & (bins - 1)) != 0)
        return fail(IRIS_E_UNSUPPORTED, "iris_score_hist: bins %d (a power of two in [%d, %d])", bins, kCurveMinBins, kCurveMaxBins);
    const long long frames = (long long)batch * (long long)n_time;
    if (frames > 2147483647LL)
        return fail(IRIS_E_UNSUPPORTED, "iris_score_hist: batch %d x T %d frames (<= 2^31 - 1)", batch, n_time);
    const int row_bytes = 2 * (bins + 1) * (int)sizeof(unsigned);
    const int kc = std::min(n_classes, kCurveLdsBytes / row_bytes);   // (>= 1: static_assert below)
    static_assert(2 * (kCurveMaxBins + 1) * sizeof(unsigned) <= (size_t)kCurveLdsBytes, "one class of the widest histogram fits the LDS tile");
    const long long per_block = (long long)kCurveThreads * kCurveFramesPerLane;
    const int gx = (int)std::min<long long>((frames + per_block - 1) / per_block, kCurveMaxBlocksX);
    const dim3 grid((unsigned)gx, (unsigned)((n_classes + kc - 1) / kc));
    k_score_hist<<<grid, kCurveThreads, (size_t)kc * row_bytes, (hipStream_t)stream>>>(
        y_true, y_pred, (int)frames, n_classes, bins, kc, reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
