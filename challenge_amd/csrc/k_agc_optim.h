// k_agc_optim.h -- adaptive gradient clipping + clipvalue + the sgd / rmsprop update of a whole model in ONE launch: the siblings of
// k_agc_clip_adam (k_agc_adam.h) for the other two values of `--optimizer` (sj_train.py:436-439 upstream).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// The same launch shape: one wave per unit row and the grid-stride row loop, the float4 path where 4 | len and every pointer the
// update reads is 16-byte aligned, the unit's two norms first, then one pass that rewrites gradient, state and parameter.  x is the
// gradient after AGC and clipvalue exactly as k_agc_clip_adam forms it and is written back to `grad`.
//     sgd      (torch.optim.SGD, momentum mu, no dampening / nesterov / weight decay):
//                  b' = mu b + x;                                    p' = p - lr b'        24 bytes of traffic per parameter
//     rmsprop  (torch.optim.RMSprop, momentum mu, not centered, no weight decay):
//                  s' = alpha s + (float)(1 - alpha) x x;  a = sqrtf(s') + eps
//                  b' = mu b + x / a;                                p' = p - lr b'        32 bytes
//     _ema     e' = e + (p' - e) (float)(1 - min(decay, (1 + t) / (10 + t)))               8 more; t = step_dev[0]
// A zero momentum buffer gives torch's first step (mu 0 + x = x).  Neither update has a bias correction: only the _ema siblings are
// handed a counter.  The rows are the Adam launch's records (iris_agc_adam_row / iris_agc_adam_ema_row) with the momentum buffer in
// the `exp_avg` slot and rmsprop's square average in `exp_avg_sq`; sgd never touches that second slot.
// ---------------------------------------------------------------------------
#define IRIS_K_RMS 0
#define IRIS_K_EMA 0
#define IRIS_K_NAME k_agc_clip_sgd
#include "k_agc_optim_kernel.h"
#undef IRIS_K_NAME
#undef IRIS_K_EMA
#define IRIS_K_EMA 1
#define IRIS_K_NAME k_agc_clip_sgd_ema
#include "k_agc_optim_kernel.h"
#undef IRIS_K_NAME
#undef IRIS_K_EMA
#undef IRIS_K_RMS
#define IRIS_K_RMS 1
#define IRIS_K_EMA 0
#define IRIS_K_NAME k_agc_clip_rmsprop
#include "k_agc_optim_kernel.h"
#undef IRIS_K_NAME
#undef IRIS_K_EMA
#define IRIS_K_EMA 1
#define IRIS_K_NAME k_agc_clip_rmsprop_ema
#include "k_agc_optim_kernel.h"
#undef IRIS_K_NAME
#undef IRIS_K_EMA
#undef IRIS_K_RMS

// every argument is looked at before the first HIP call; nothing is allocated, nothing synchronised
static int agc_optim_args(const char* who, const void* rows_dev, double mu, bool rms, double alpha, float eps, bool ema,
                          const void* step_dev, double decay) {
    if (!rows_dev) return fail(IRIS_E_INVALID, "%s: NULL row table", who);
    if (!(mu >= 0.0 && mu < 1.0)) return fail(IRIS_E_INVALID, "%s: momentum %g outside [0, 1)", who, mu);
    if (rms && !(alpha >= 0.0 && alpha < 1.0 && eps >= 0.f)) return fail(IRIS_E_INVALID, "%s: alpha %g / eps %g", who, alpha, (double)eps);
    if (ema && !step_dev) return fail(IRIS_E_INVALID, "%s: NULL step counter", who);
    if (ema && !(decay >= 0.0 && decay < 1.0)) return fail(IRIS_E_INVALID, "%s: decay %g outside [0, 1)", who, decay);
    return IRIS_OK;
}

extern "C" int iris_agc_clip_sgd(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                 int use_agc, const float* lr_dev, float lr_host, double mu, void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (int rc = agc_optim_args("iris_agc_clip_sgd", rows_dev, mu, false, 0.0, 0.f, false, nullptr, 0.0)) return rc;
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_sgd<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue, use_agc ? 1 : 0, lr_dev,
                                                                    lr_host, (float)mu);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_agc_clip_sgd_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                     int use_agc, const float* lr_dev, float lr_host, double mu, const float* step_dev, double decay,
                                     void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (int rc = agc_optim_args("iris_agc_clip_sgd_ema", rows_dev, mu, false, 0.0, 0.f, true, step_dev, decay)) return rc;
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_sgd_ema<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue, use_agc ? 1 : 0,
                                                                        lr_dev, lr_host, (float)mu, step_dev, decay);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_agc_clip_rmsprop(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                                     int use_agc, const float* lr_dev, float lr_host, double mu, double alpha, float eps, void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (int rc = agc_optim_args("iris_agc_clip_rmsprop", rows_dev, mu, true, alpha, eps, false, nullptr, 0.0)) return rc;
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_rmsprop<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue, use_agc ? 1 : 0,
                                                                        lr_dev, lr_host, (float)mu, alpha, eps);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_agc_clip_rmsprop_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc,
                                         float clipvalue, int use_agc, const float* lr_dev, float lr_host, double mu, double alpha, float eps,
                                         const float* step_dev, double decay, void* stream) {
    if (n_rows == 0) return IRIS_OK;
    if (int rc = agc_optim_args("iris_agc_clip_rmsprop_ema", rows_dev, mu, true, alpha, eps, true, step_dev, decay)) return rc;
    const size_t blocks = std::min<size_t>((n_rows + 3) / 4, 8192);
    k_agc_clip_rmsprop_ema<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps_agc, clipvalue,
                                                                            use_agc ? 1 : 0, lr_dev, lr_host, (float)mu, alpha, eps, step_dev,
                                                                            decay);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
