// k_fused_mfma.h -- the fused hot path with the mel step on the matrix cores (fp16 inputs, fp32 accumulate).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K1m: waveform -> mel magnitudes, mel contraction as v_mfma_f32_16x16x32_f16   (BASELINE configs[4])
//   mel[m, frame] = sum_f W[f, m] |X[f, frame]|   (transforms.py:65, tf.tensordot over the bin axis)
//   as D[16 mel x 16 frames] += A[16 mel x 32 bins] . B[32 bins x 16 frames] per MFMA:
//     A = 0.5 W^T in fp16, one 16-band tile per wave, held in REGISTERS for the whole kernel: only the
//         k-steps (32 bins) that hold a non-zero of the tile are kept (a triangular filterbank touches
//         2-8 of them per tile; with the default 3800 Hz edge two thirds of the bins feed no band at all);
//     B = 2 |X| in fp16, written by the waves that transformed the frames into an LDS tile [8 frames][bins];
//     D = fp32, lane (n = lane & 15, r = lane >> 4) holds mel 4 r + i of frame n.
//   Workgroup = 8 waves, walking its chunk in groups of 8 wave-frames: every wave transforms one frame
//   (same FFT core as K1; next frame in flight by LDS-DMA), converts 2|X| to fp16 into the group's tile
//   (double-buffered: ONE workgroup barrier per group), then runs the MFMAs of its band tile over all 8
//   frames of the group (columns 8..15 of B repeat 0..7 and are dropped) and stores 4 bands x 8 frames.
//   Supported: n_fft 512 / 1024 / 2048, n_mel <= 128, bands within the lower half of the spectrum, <= 8
//   k-steps per tile, no SpecAugment bands (those calls take the fp32 kernel).  fp16 carries 11 bits: the
//   stated tolerance of this variant is 2e-3 relative (tests/test_frontend_gpu.py), not north_star's 1e-5 -
//   which is why the banded fp32 kernel stays the default.
// ---------------------------------------------------------------------------
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int kMfmaWaves = 8, kMfmaKsMax = 8, kMfmaGroup = 8;

// untangle (lower half only) + magnitude, stored as fp16 into `row` for bins k < kb_pad (a multiple of 64)
template <int LOG2N>
__device__ __forceinline__ void untangle_mag_half(const cf (&x)[FftCfg<LOG2N>::P], const cf* post, cf* lds, _Float16* row,
                                                  int kb_pad, int lane) {
    constexpr int P = FftCfg<LOG2N>::P;
    cf* wp = lds + lds_pad<untangle_pm(LOG2N)>(lane);
#pragma unroll
    for (int q = P / 2; q < P; ++q) wp[lds_pad<untangle_pm(LOG2N)>(kWave * q)] = x[q];
    wave_sync_lds();
    const cf* rp = lds + lds_pad<untangle_pm(LOG2N)>(kWave - lane);
    cf zp[P / 2];
#pragma unroll
    for (int q = 0; q < P / 2; ++q) zp[q] = rp[lds_pad<untangle_pm(LOG2N)>(kWave * (P - 1 - q))];
    if (lane == 0) zp[0] = x[0];  // k = 0 pairs with itself
#pragma unroll
    for (int q = 0; q < P / 2; ++q) {
        if (kWave * q < kb_pad) {  // wave-uniform
            const cf e = __builtin_elementwise_fma(zp[q], mk(1.0f, -1.0f), x[q]);  // 2 E
            const cf d = __builtin_elementwise_fma(zp[q], mk(-1.0f, 1.0f), x[q]);  // 2 i O
            const cf lo = e + cmul_mi_tw(d, post[q]);
            row[lane + kWave * q] = (_Float16)cabs_rn(lo);  // 2 |X[k]|
        }
    }
    wave_sync_lds();
}

// K1m itself lives in k_fused_mfma_kernel.h, expanded twice: k_wav_to_mel_mfma, and k_wav_to_mel_mfma_gain (FilterAugment)
#define IRIS_K_GAIN 0
#include "k_fused_mfma_kernel.h"
#undef IRIS_K_GAIN
#define IRIS_K_GAIN 1
#include "k_fused_mfma_kernel.h"
#undef IRIS_K_GAIN
