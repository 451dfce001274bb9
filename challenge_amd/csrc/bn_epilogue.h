// bn_epilogue.h -- the copies of the per-channel BatchNorm sums, and how a convolution kernel's epilogue contributes to them.
// Included by k_elementwise.h (the BatchNorm passes) and by the convolution kernels (k_conv_wino.h, k_conv_wino_b3.h, k_conv_c32.h),
// also when those are built alone (scripts/microbench/wino_conv.hip).
#pragma once
#ifndef IRIS_BN_SLOTS
#define IRIS_BN_SLOTS 8
#endif
// The per-channel sums are accumulated by fp64 atomics of every block.  A 32-channel layer has 64 addresses and 2048
// blocks: the same-address atomics queue up behind one another.  Blocks therefore add into one of kBnSlots copies
// (sums[slot][2][C], slot = block % bn_slots(C)) and the consumers add the copies up while they form their per-channel
// coefficients (their blocks are fat - at most 2048 per launch - so that this setup is amortised).  A last-block fold behind an
// arrival counter was measured too: the counter is one more hot address (reductions 0.88 -> 0.99 ms per step).
constexpr int kBnSlots = IRIS_BN_SLOTS;  // at most; bn_slots(channels) of them are used (wide layers have few blocks per address)
__host__ __device__ constexpr int bn_slots(int channels) {
    return channels <= 64 ? kBnSlots : channels <= 128 ? kBnSlots / 2 : channels <= 256 ? kBnSlots / 4 : 1;
}

// ---- ReLU and MaxPool of every convolution / BatchNorm epilogue: a NaN stays a NaN, as in torch.relu / max_pool2d (fmaxf(NaN, c)
// is c: a diverged activation would leave these layers as 0 and never reach the loss, where fit.py's TerminateOnNaN looks for it).
// IEEE-754 maximum() - NaN if either operand is - is ONE v_maximum3_f32 on gfx950, like the v_max_f32 it replaces (and two of them
// in a row fold into one).  max_keep_nan(v, -INFINITY) is v for every v, NaN included: the bare form of the Winograd kernels.
__device__ __forceinline__ float max_keep_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }
// E[z^2] - E[z]^2 floored at 0 - and NaN where the sums are (fmax(NaN, 0.0) is 0: running_var and rstd would come out finite
// beside a NaN mean)
__device__ __forceinline__ double bn_var_floor(double v) { return v < 0.0 ? 0.0 : v; }

// ---- BatchNorm statistics from a convolution's EPILOGUE (round 6): the kernel that produces z adds each lane's share of
// sum z and sum z^2 of its output channel to `sums` itself, so that the separate read of z by k_bn_reduce<false> disappears.
// A lane accumulates in fp32 about a LOCAL shift K (one of its own values: the partial sums are then of the size of the
// channel's spread, whatever its mean), and converts to sums about ZERO in fp64 when it flushes:
//   sum z = S1 + n K,   sum z^2 = S2 + 2 K S1 + n K^2      (fp64: E[z^2] - E[z]^2 then cancels to 2^-53 (mean / sigma)^2)
// The consumers are told (`sums_about_zero`) that their K is 0 and that the sums lie in windows (below).  [slot][2][C] copies as k_bn_reduce's.
struct BnEpilogue {
    float k, s1, s2, n;
};
__device__ __forceinline__ void bn_epilogue_add(BnEpilogue& a, float v, float valid /*1 or 0*/) {
    const float d = (v - a.k) * valid;
    a.s1 += d;
    a.s2 = fmaf(d, d, a.s2);
    a.n += valid;
}
// The flush is REPRODUCIBLE to the bit: fp64 atomics arrive in any order, and a rounded sum depends on it (1 - 2 ulp between two
// calls on the same input).  So a share is split over kBnBins exponent windows - its multiples of 1, of 2^-40 below 1 and of 2^-80
// below 2^-40 (what lies below 2^-80 is dropped: 1e-24 absolute per share) - and each window has its own copy of the
// [slot][2][C] block, `bn_region(C)` doubles apart.  Inside a window every share is a multiple of its grid and smaller than 2^40
// grid steps, so with fewer than 2^13 shares per address (the largest layer of the CRNN: 2^10) every partial sum is exact in fp64
// whatever the order (the top window: exact below 2^53).  bn_sum_binned (k_elementwise.h) folds windows and slots in a fixed order.
// A NaN share is NaN in all three windows, an infinite one non-finite.
constexpr int kBnBins = 3;
__host__ __device__ constexpr size_t bn_region(int channels) { return (size_t)bn_slots(channels) * 2 * channels; }
__device__ __forceinline__ void bn_binned_add(double* at, size_t region, double a) {
    const double hi = trunc(a);
    double r = a - hi;                                          // exact; |r| < 1
    const double mid = trunc(r * 0x1p40) * 0x1p-40;
    r -= mid;                                                   // exact; |r| < 2^-40
    const double lo = trunc(r * 0x1p80) * 0x1p-80;
    if (hi != 0.0) atomicAdd(at, hi);                           // (NaN != 0)
    if (mid != 0.0) atomicAdd(at + region, mid);
    if (lo != 0.0) atomicAdd(at + 2 * region, lo);
}
__device__ __forceinline__ void bn_epilogue_flush(const BnEpilogue& a, double* sums, int C, int channel, int slot) {
    if (a.n > 0.f) {
        const double K = (double)a.k, n = (double)a.n, S1 = (double)a.s1, S2 = (double)a.s2;
        bn_binned_add(sums + (size_t)slot * 2 * C + channel, bn_region(C), S1 + n * K);
        bn_binned_add(sums + (size_t)slot * 2 * C + C + channel, bn_region(C), S2 + 2.0 * K * S1 + n * K * K);
    }
}

