// k_agc_adam.h -- adaptive gradient clipping + clipvalue + the Adam update of a whole model in ONE launch (round 6): the tail of the
// reference's train_step (sj_train.py:145-155 adaptive_clip_grad, :434-435 Adam(clipvalue), :176-182 apply_gradients).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// k_agc_clip (k_elementwise.h) reads a unit's parameters and gradients for the two norms and rewrites the gradients; torch's fused
// Adam then reads parameters, gradients and both moments again through three multi-tensor launches at 1.9 TB/s (143 us for the
// CRNN's 9.9 M parameters; profiles/r6/c4_split0_step_kernel_stats.csv).  Here a wave keeps going after it has the unit's clip
// factor: gradient -> scaled, clamped, written back (p.grad still holds what the reference's optimiser would have been handed),
// moments and parameter updated in the same pass - 32 bytes of traffic per parameter instead of 52, one launch instead of four.
// Arithmetic = ATen's fused Adam (adam_math, ADAM_MODE ORIGINAL, fp32 op-math):
//     m += (g - m) (1 - beta1);   v = beta2 v + (1 - beta2) g g;
//     p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with t read from the optimiser's own (already incremented) device-side step counter and lr from its device tensor when it has one
// (capturable optimisers: a replayed hipGraph sees every new value).  No weight decay, no amsgrad, no maximize: the caller (FusedAGC
// in hip_autograd.py) takes torch's path for anything else.
// ---------------------------------------------------------------------------

// The kernel itself lives in k_agc_adam_kernel.h, expanded twice: k_agc_clip_adam, and k_agc_clip_adam_ema, which also keeps an
// exponential moving average of the weights (a shadow row per unit, in the parameter's own layout):
//     d_t = min(decay, (1 + t) / (10 + t));   e += (p' - e) (float)(1 - d_t)
// with the same t and p' the update has just produced in its register - 40 bytes of traffic per parameter instead of 32, no launch
// and no graph node of its own.  The float4 path also wants the shadow row 16-byte aligned.  A NaN in p' goes into e.
#define IRIS_K_EMA 0
#include "k_agc_adam_kernel.h"
#undef IRIS_K_EMA
#define IRIS_K_EMA 1
#include "k_agc_adam_kernel.h"
#undef IRIS_K_EMA

extern "C" int iris_agc_clip_adam(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                  int use_agc, const float* lr_dev, float lr_host, double beta1, double beta2, float eps,
                                  const float* step_dev, void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (!rows_dev || !step_dev) return fail(IRIS_E_INVALID, "iris_agc_clip_adam: NULL argument");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f))
        return fail(IRIS_E_INVALID, "iris_agc_clip_adam: betas (%g, %g) / eps %g", beta1, beta2, (double)eps);
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_adam<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue, use_agc ? 1 : 0, lr_dev,
                                                                     lr_host, beta1, beta2, eps, step_dev);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_agc_clip_adam_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                      int use_agc, const float* lr_dev, float lr_host, double beta1, double beta2, float eps,
                                      const float* step_dev, double decay, void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (!rows_dev || !step_dev) return fail(IRIS_E_INVALID, "iris_agc_clip_adam_ema: NULL argument");
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f))
        return fail(IRIS_E_INVALID, "iris_agc_clip_adam_ema: betas (%g, %g) / eps %g", beta1, beta2, (double)eps);
    if (!(decay >= 0.0 && decay < 1.0)) return fail(IRIS_E_INVALID, "iris_agc_clip_adam_ema: decay %g outside [0, 1)", decay);
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_adam_ema<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue, use_agc ? 1 : 0,
                                                                         lr_dev, lr_host, beta1, beta2, eps, step_dev, decay);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
