// k_magmel.h -- spectrum -> mel (complex_to_magphase + magphase_to_mel fused).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K3: spectrum -> mel (complex_to_magphase + magphase_to_mel fused)
//   block = 256 threads: 64 consecutive (t, c) columns x 4 waves over mel bands
// ---------------------------------------------------------------------------
struct MagmelArgs {
    const float* spec;  // [B, F, T, 2C]
    float* mel;         // [B, M, T, C]
    const float* w;     // dense [F][M]
    const int* band_lo;
    const int* band_len;
    const int* t_bands;
    int n_tb;
    const int* f_bands;
    int n_fb;
    int B, C, F, T, M, is_magphase;
};
struct MagmelGainArgs {  // the FilterAugment siblings: the same block, then the [B, M] per-sample mel-band gains
    MagmelArgs a;
    const float* gain;
};

// K3b: streaming variant for triangular filterbanks (every bin feeds at most two adjacent
// bands, which is what linear_to_mel_weight_matrix produces): one thread per frame t walks the
// bins once with two open accumulators per channel; a band is written as soon as the walk
// has passed its last bin.  Every spectrum element is read exactly once, with one 8/16-byte
// load per bin (all 2C components), coalesced along t.
struct MagmelTriArgs {
    const float* spec;   // [B, F, T, 2C]
    float* mel;          // [B, M, T, C]
    const int* bin_band; // [F] first band fed by bin f (-1: none)
    const float* bin_w;  // [F][2] weights for bands bin_band[f] and bin_band[f] + 1
    const int* t_bands;
    int n_tb;
    const int* f_bands;
    int n_fb;
    int B, F, T, M, is_magphase, f_lo, f_hi;  // bins outside [f_lo, f_hi) feed nothing
};
struct MagmelTriGainArgs {
    MagmelTriArgs a;
    const float* gain;
};

// K3 and K3b themselves live in k_magmel_kernel.h, expanded twice: k_magmel / k_magmel_tri, and their FilterAugment
// siblings k_magmel_gain / k_magmel_tri_gain
#define IRIS_K_GAIN 0
#include "k_magmel_kernel.h"
#undef IRIS_K_GAIN
#define IRIS_K_GAIN 1
#include "k_magmel_kernel.h"
#undef IRIS_K_GAIN
