"""CPU tests of the C-ABI boundary: the library loads, exports every symbol
include/iris_frontend.h declares, and its host-only entry points behave
(no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from challenge_amd import _native as N
from oracle import frontend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "iris_frontend.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(iris_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_header_symbol():
    lib = N.lib()
    syms = header_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/iris_frontend.h but not exported"
        assert s in N.SIGNATURES, f"{s} has no ctypes signature in challenge_amd/_native.py"
    assert sorted(N.SIGNATURES) == syms
    assert lib.iris_abi_version() == 1


@pytest.mark.parametrize("m,f,sr", [(80, 257, 16000), (64, 513, 16000), (128, 1025, 22050), (40, 129, 16000)])
def test_host_mel_matrix_matches_oracle(m, f, sr):
    from challenge_amd.frontend import mel_weight_matrix
    w = mel_weight_matrix(m, f, sr)
    ref = R.linear_to_mel_weight_matrix(m, f, sr)
    assert w.shape == ref.shape
    assert np.array_equal(w, ref)  # same fp32 op sequence, correctly rounded log: bit-identical
    assert np.all(w[0] == 0)


def test_host_mel_matrix_kwargs_and_errors():
    from challenge_amd.frontend import mel_weight_matrix
    w = mel_weight_matrix(20, 129, 8000, 300.0, 3400.0)
    ref = R.linear_to_mel_weight_matrix(20, 129, 8000, 300.0, 3400.0)
    assert np.array_equal(w, ref)
    for bad in [(0, 129, 8000, 125.0, 3800.0), (20, 129, 8000, 3800.0, 125.0),
                (20, 129, 8000, 125.0, 5000.0), (20, 129, 8000, -1.0, 3800.0)]:
        with pytest.raises(ValueError):
            mel_weight_matrix(*bad)
    assert b"" != N.lib().iris_last_error()


def test_argument_validation_without_gpu():
    lib = N.lib()
    h = C.c_void_p()
    # unsupported n_fft and inconsistent n_bins are rejected before any HIP call
    assert lib.iris_plan_create(C.byref(h), 0, 300, 150, 64, 151, 16000.0, 125.0, 3800.0, 1, 1, 1000, None) == -2
    assert lib.iris_plan_create(C.byref(h), 0, 1024, 256, 64, 512, 16000.0, 125.0, 3800.0, 1, 1, 10000, None) == -1
    assert lib.iris_plan_create(C.byref(h), 0, 1024, 0, 64, 513, 16000.0, 125.0, 3800.0, 1, 1, 10000, None) == -1
    assert lib.iris_plan_create(C.byref(h), 0, 1024, 256, 64, 513, 16000.0, 125.0, 3800.0, 1, 1, 512, None) == -1
    assert lib.iris_wav_to_logmel(None, None, None, 1, 1, 3, None, 0, None, 0, None) == -1
    assert lib.iris_minmax_log_workspace(32, 40064) == 2 * 32 * 10
    assert lib.iris_normalize_workspace(32, 160000) == 32 * 40
    # the STFT's geometry query: host arithmetic only, refuses NULL before it reads the plan
    geom = (C.c_int * 5)(7, 7, 7, 7, 7)
    assert lib.iris_stft_geometry(None, 1, 1000, geom) == -1 and lib.iris_last_error().startswith(b"iris_stft_geometry:")
    assert lib.iris_stft_geometry(None, 1, 1000, None) == -1
    assert list(geom) == [7] * 5
    assert lib.iris_mask_apply(None, 1, 1, 1, 4, None, 0, 1, None) == -1
    assert lib.iris_mask_apply(C.c_void_p(8), 1, 1, 1, 2, None, 0, 1, None) == -2
    # batched synthesis, spectrum and waveform domain: NULL / inconsistent sizes are rejected before any launch
    p8 = C.c_void_p(8)
    assert lib.iris_mix_specs(None, 1, None, None, None, None, 1, 257, 64, 4, 4, 3, None, 0, None) == -1
    assert lib.iris_mix_specs(p8, 1, p8, p8, p8, p8, 1, 257, 64, 3, 4, 3, p8, 1, None) == -2        # chan2 not in {1,2,4,8}
    assert lib.iris_mix_waves(None, 1, None, None, None, None, 1, 2, 256, 64, 4, 3, None, 0, None) == -1
    assert lib.iris_mix_waves(p8, 1, p8, p8, p8, p8, 2, 2, 256, 64, 4, 3, p8, 1, None) == -1        # fewer sources than samples
    assert lib.iris_mix_waves(p8, 4, p8, p8, p8, p8, 1, 2, 256, 64, 4, 3, p8, 1, None) == -3        # workspace too small
    assert lib.iris_mix_waves(p8, 1, p8, p8, p8, p8, 1, 2, 256, 1, 4, 3, p8, 1, None) == -1         # n_frame must exceed 1
    assert lib.iris_mix_wave_frame_active(None, 1, 100, 1024, 256, None, None) == -1
    assert lib.iris_mix_wave_frame_active(p8, 1, 100, 1024, 0, p8, None) == -1


def test_round3_entry_points_validate_before_any_launch():
    """bias/ReLU epilogues, BatchNorm passes, device-side draws, epilogue mode and the timing sampler reject NULL,
    misaligned and out-of-range arguments before any HIP call (error codes of include/iris_frontend.h)."""
    lib = N.lib()
    p16, p8 = C.c_void_p(16), C.c_void_p(8)
    INVALID, UNSUPPORTED = -1, -2
    assert lib.iris_bias_relu(None, p16, 4, 8, None) == INVALID
    assert lib.iris_bias_relu(p16, p16, 4, 6, None) == UNSUPPORTED            # channels not a multiple of 4
    assert lib.iris_bias_relu(p8, p16, 4, 8, None) == INVALID                 # 16-byte alignment
    assert lib.iris_bias_relu(p16, p16, 0, 8, None) == 0                      # empty: nothing to do, no launch
    assert lib.iris_bias_relu_maxpool(p16, p16, None, 1, 4, 4, 8, None) == INVALID
    assert lib.iris_bias_relu_maxpool(p16, p16, p16, 1, 4, 4, 7, None) == UNSUPPORTED
    assert lib.iris_bias_relu_maxpool(p16, p16, p16, 0, 4, 4, 8, None) == INVALID
    assert lib.iris_bias_relu_nchw(p16, None, 4, 8, 64, None) == INVALID
    assert lib.iris_bias_relu_nchw(p16, p16, 4, 8, 6, None) == UNSUPPORTED    # inner size not a multiple of 4
    assert lib.iris_bias_relu_maxpool_nchw(p16, p16, None, 1, 4, 4, 8, None) == INVALID
    assert lib.iris_bias_relu_maxpool_nchw(p16, p16, p16, 1, 0, 4, 8, None) == INVALID
    assert lib.iris_bn_stats(None, 16, 8, p16, None) == INVALID
    assert lib.iris_bn_stats(p16, 16, 6, p16, None) == UNSUPPORTED
    assert lib.iris_bn_stats(p16, 16, 8192, p16, None) == UNSUPPORTED         # more than 4096 channels
    assert lib.iris_bn_relu_apply(None, None, 16, 8, None, None, None, None, 1e-3, 0.01, None, None, None, None, None) == INVALID
    assert lib.iris_bn_relu_apply(p16, p16, 16, 8, p16, p16, p16, None, 1e-3, 0.01, p16, p16, p16, p16, None) == INVALID  # y aliases z
    assert lib.iris_bn_relu_bwd_reduce(None, p16, 16, 8, p16, p16, p16, p16, p16, None) == INVALID
    assert lib.iris_bn_relu_bwd_dx(None, p16, p16, 16, 8, p16, p16, p16, p16, p16, p16, p16, None) == INVALID
    assert lib.iris_mix_draw(None, None, None, 1, 64, 4, 4, 0.5, 1.0, 1.0, 7, None, None, None, None) == INVALID
    assert lib.iris_augment_draw(0, 64, 64, 2, 2, 8, 8, 7, None, None, None, None) == INVALID
    assert lib.iris_plan_set_epilogue(None, 0) == INVALID
    assert lib.iris_plan_status(None, None) == INVALID
    assert lib.iris_plan_set_epilogue_timeout(None, 0) == INVALID
    n = C.c_int(0)
    assert lib.iris_timing_samples(None, 0, None, 0, C.byref(n)) == INVALID
    assert lib.iris_timing_enable(None, 1) == INVALID
    assert lib.iris_plan_kernel_name(None, 32, None, 0) == INVALID
    assert lib.iris_conv3x3_small_bias_relu_nchw(None, p16, p16, p16, 1, 1, 32, 8, 8, None) == INVALID
    assert lib.iris_conv3x3_small_bias_relu_nchw(p16, p16, p16, p16, 1, 3, 32, 8, 8, None) == UNSUPPORTED   # 1 or 2 input channels
    assert lib.iris_conv3x3_small_bias_relu_nchw(p16, p16, p16, p16, 1, 1, 32, 8, 6, None) == UNSUPPORTED   # width % 4
    assert lib.iris_conv3x3_small_bias_relu_nchw(p8, p16, p16, p16, 1, 1, 32, 8, 8, None) == INVALID        # alignment
    assert lib.iris_conv3x3_small_bias_relu_nhwc(p16, p16, None, p16, 1, 1, 32, 8, 8, None) == INVALID
    assert lib.iris_conv3x3_small_bias_relu_nhwc(p16, p16, p16, p16, 1, 1, 48, 8, 8, None) == UNSUPPORTED   # 48 does not divide 1024
    assert lib.iris_conv3x3_small_bias_relu_nhwc(p16, p16, p16, p16, 1, 1, 32, 8, 4096, None) == UNSUPPORTED  # rows beyond the LDS
    assert lib.iris_conv3x3_c32_bias_relu(None, p16, p16, p16, 1, 8, 8, 0, 0, None) == INVALID
    assert lib.iris_conv3x3_c32_bias_relu(p8, p16, p16, p16, 1, 8, 8, 1, 0, None) == INVALID                  # alignment
    assert lib.iris_conv3x3_c32_bias_relu(p16, p16, p16, p16, 0, 8, 8, 1, 1, None) == INVALID
    assert lib.iris_conv3x3_wino(None, p16, p16, p16, 1, 8, 8, 64, 64, 0, None) == INVALID
    assert lib.iris_conv3x3_wino(p16, p16, p16, p16, 1, 8, 8, 12, 64, 0, None) == UNSUPPORTED    # cin % 8
    assert lib.iris_conv3x3_wino(p16, p16, p16, p16, 1, 8, 8, 64, 96, 0, None) == UNSUPPORTED    # cout % 64
    assert lib.iris_conv3x3_wino(p8, p16, p16, p16, 1, 8, 8, 64, 64, 0, None) == INVALID         # alignment
    assert lib.iris_conv3x3_wino(p16, p16, p16, p16, 0, 8, 8, 64, 64, 0, None) == INVALID
    assert lib.iris_conv3x3_wino(p16, p16, None, p16, 1, 8, 8, 64, 64, 16, None) == INVALID                          # unknown flag
    assert lib.iris_wino_pack_weights_device(None, 9, 1, 3, 1, 8, 64, 0, p16, None) == INVALID
    assert lib.iris_wino_pack_weights_device(p16, 9, 1, 3, 1, 8, 48, 0, p16, None) == UNSUPPORTED
    assert lib.iris_wino_pack_weights(None, 8, 64, p16) == INVALID and lib.iris_wino_pack_weights(p16, 8, 48, p16) == UNSUPPORTED
    assert lib.iris_wino_packed_len(8, 64) == 16 * 8 * 64 and lib.iris_wino_packed_len(0, 64) == 0
    assert lib.iris_bilstm128_forward(None, p16, p16, None, 4, 16, None) == INVALID
    assert lib.iris_bilstm128_forward(p16, p8, p16, None, 4, 16, None) == INVALID     # w_hh must be 16-byte aligned
    assert lib.iris_bilstm128_forward(p16, p16, p16, None, 0, 16, None) == INVALID
    assert lib.iris_bilstm128_backward(p16, None, p16, p16, 4, 16, None) == INVALID
    assert lib.iris_bilstm128_backward(p16, p16, p16, p16, 4, 0, None) == INVALID
    assert lib.iris_bn_relu_pool_apply(None, None, 1, 4, 4, 8, None, None, None, None, 1e-3, 0.01, None, None, None, None, None) == INVALID
    assert lib.iris_bn_relu_pool_apply(p16, p16, 0, 4, 4, 8, p16, p16, p16, None, 1e-3, 0.01, p16, p16, p16, p16, None) == INVALID
    assert lib.iris_bn_relu_pool_bwd_reduce(p16, None, 1, 4, 4, 8, p16, p16, p16, p16, p16, None) == INVALID
    assert lib.iris_bn_relu_pool_bwd_dx(p16, p16, p16, 1, 4, 4, 6, p16, p16, p16, p16, p16, p16, p16, None) == UNSUPPORTED
    assert b"" != lib.iris_last_error()


def test_convolution_training_forms_validate_before_any_launch():
    """The split-bf16 Winograd convolution, the BatchNorm-statistics forms of both Winograd kernels, the device packers and the
    c32 training forms refuse NULL, misaligned, empty and unsupported arguments before any HIP call; the error names the entry
    point that was called.  (The `_bn` entry points take no bias, so their "no bias with the statistics" rule is only reachable
    through frontend.conv3x3_wino.)"""
    lib = N.lib()
    p16, p8 = C.c_void_p(16), C.c_void_p(8)
    INVALID, UNSUPPORTED = -1, -2
    POOL, OUT_NHWC, RELU = N.IRIS_WINO_POOL, N.IRIS_WINO_OUT_NHWC, N.IRIS_WINO_RELU

    def refused(rc, code, name):
        assert rc == code, (name, rc)
        assert lib.iris_last_error().startswith(name.encode() + b":"), (name, lib.iris_last_error())

    b3 = "iris_conv3x3_wino_b3"
    refused(lib.iris_conv3x3_wino_b3(None, p16, p16, p16, 1, 8, 8, 64, 64, 0, None), INVALID, b3)
    refused(lib.iris_conv3x3_wino_b3(p16, None, p16, p16, 1, 8, 8, 64, 64, 0, None), INVALID, b3)
    refused(lib.iris_conv3x3_wino_b3(p16, p16, p16, None, 1, 8, 8, 64, 64, 0, None), INVALID, b3)
    refused(lib.iris_conv3x3_wino_b3(p16, p16, p16, p16, 1, 8, 8, 24, 64, 0, None), UNSUPPORTED, b3)    # cin % 16 (a multiple of 8)
    refused(lib.iris_conv3x3_wino_b3(p16, p16, p16, p16, 1, 8, 8, 64, 96, 0, None), UNSUPPORTED, b3)    # cout % 64
    refused(lib.iris_conv3x3_wino_b3(p8, p16, p16, p16, 1, 8, 8, 64, 64, 0, None), INVALID, b3)         # x alignment
    refused(lib.iris_conv3x3_wino_b3(p16, p8, p16, p16, 1, 8, 8, 64, 64, 0, None), INVALID, b3)         # packed alignment
    refused(lib.iris_conv3x3_wino_b3(p16, p16, p16, p16, 0, 8, 8, 64, 64, 0, None), INVALID, b3)        # empty
    refused(lib.iris_conv3x3_wino_b3(p16, p16, p16, p16, 1, 8, 0, 64, 64, 0, None), INVALID, b3)
    refused(lib.iris_conv3x3_wino_b3(p16, p16, None, p16, 1, 8, 8, 64, 64, 16, None), INVALID, b3)      # unknown flag
    refused(lib.iris_conv3x3_wino(p16, p8, p16, p16, 1, 8, 8, 64, 64, 0, None), INVALID, "iris_conv3x3_wino")

    for bn in ("iris_conv3x3_wino_bn", "iris_conv3x3_wino_b3_bn"):
        fn = getattr(lib, bn)
        refused(fn(p16, p16, p16, 1, 8, 8, 64, 64, OUT_NHWC, None, None), INVALID, bn)                # NULL sums
        refused(fn(p16, p16, p16, 1, 8, 8, 64, 64, OUT_NHWC | POOL, p16, None), INVALID, bn)          # sums with pooling
        refused(fn(p16, p16, p16, 1, 8, 8, 64, 64, OUT_NHWC | RELU, p16, None), INVALID, bn)          # sums with ReLU
        refused(fn(p16, p16, p16, 1, 8, 8, 64, 64, 0, p16, None), INVALID, bn)                        # sums need channels-last out
        refused(fn(None, p16, p16, 1, 8, 8, 64, 64, OUT_NHWC, p16, None), INVALID, bn[:-3])           # then the plain form's checks
        refused(fn(p16, p16, p16, 1, 8, 8, 64, 96, OUT_NHWC, p16, None), UNSUPPORTED, bn[:-3])

    for name, kc in (("iris_wino_pack_weights_device", 8), ("iris_wino_b3_pack_weights_device", 16)):
        fn = getattr(lib, name)
        refused(fn(None, 9, 1, 3, 1, kc, 64, 0, p16, None), INVALID, name)
        refused(fn(p16, 9, 1, 3, 1, kc, 64, 0, None, None), INVALID, name)
        refused(fn(p16, 9, 1, 3, 1, kc + 4, 64, 0, p16, None), UNSUPPORTED, name)                     # cin % granularity
        refused(fn(p16, 9, 1, 3, 1, kc, 48, 0, p16, None), UNSUPPORTED, name)                         # cout % 64
        refused(fn(p16, 9, 1, 3, 1, 0, 64, 0, p16, None), UNSUPPORTED, name)
        refused(fn(p16, 9, 1, 3, 1, kc, 64, 0, p8, None), INVALID, name)                              # packed alignment
    refused(lib.iris_wino_b3_pack_weights_device(p16, 9, 1, 3, 1, 8, 64, 0, p16, None), UNSUPPORTED, "iris_wino_b3_pack_weights_device")

    multi = "iris_wino_pack_weights_device_multi"

    def jobs(*spec):
        arr = (N.PackJob * len(spec))()
        for k, (weight, packed, cin, cout) in enumerate(spec):
            arr[k] = N.PackJob(weight, packed, 9, 1, 3, 1, cin, cout, 0, 0)
        return C.cast(arr, C.c_void_p)

    ok8, ok16 = (16, 16, 8, 64), (16, 16, 16, 64)
    refused(lib.iris_wino_pack_weights_device_multi(None, 1, 0, None), INVALID, multi)
    refused(lib.iris_wino_pack_weights_device_multi(jobs(ok8), 0, 0, None), INVALID, multi)                         # no jobs
    for split, ok in ((0, ok8), (1, ok16)):   # every job is checked before the first launch: a bad second job refuses the call
        refused(lib.iris_wino_pack_weights_device_multi(jobs(ok, (None, 16, 16, 64)), 2, split, None), INVALID, multi)
        assert b"job 1" in lib.iris_last_error()
        refused(lib.iris_wino_pack_weights_device_multi(jobs(ok, (16, None, 16, 64)), 2, split, None), INVALID, multi)
        refused(lib.iris_wino_pack_weights_device_multi(jobs(ok, (16, 8, 16, 64)), 2, split, None), INVALID, multi)  # alignment
        refused(lib.iris_wino_pack_weights_device_multi(jobs(ok, (16, 16, 16, 48)), 2, split, None), UNSUPPORTED, multi)
    refused(lib.iris_wino_pack_weights_device_multi(jobs((16, 16, 12, 64)), 1, 0, None), UNSUPPORTED, multi)        # 8 | cin
    refused(lib.iris_wino_pack_weights_device_multi(jobs((16, 16, 8, 64)), 1, 1, None), UNSUPPORTED, multi)         # 16 | cin
    refused(lib.iris_wino_pack_weights_device_multi(jobs((16, 16, 24, 64)), 1, 1, None), UNSUPPORTED, multi)

    c32 = "iris_conv3x3_c32"
    refused(lib.iris_conv3x3_c32(None, p16, 288, 9, 3, 1, 0, p16, 1, 8, 8, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32(p16, None, 288, 9, 3, 1, 0, p16, 1, 8, 8, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32(p16, p16, 288, 9, 3, 1, 0, None, 1, 8, 8, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32(p16, p16, 288, 9, 3, 1, 1, p16, 0, 8, 8, None), INVALID, c32)          # empty
    refused(lib.iris_conv3x3_c32(p16, p16, 288, 9, 3, 1, 0, p16, 1, 0, 8, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32(p8, p16, 288, 9, 3, 1, 0, p16, 1, 8, 8, None), INVALID, c32)           # alignment
    refused(lib.iris_conv3x3_c32_bn(p16, p16, 288, 9, 3, 1, p16, 1, 8, 8, None, None), INVALID, "iris_conv3x3_c32_bn")
    refused(lib.iris_conv3x3_c32_bn(None, p16, 288, 9, 3, 1, p16, 1, 8, 8, p16, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32_bn(p16, p16, 288, 9, 3, 1, p16, 1, 8, 0, p16, None), INVALID, c32)
    refused(lib.iris_conv3x3_c32_bn(p8, p16, 288, 9, 3, 1, p16, 1, 8, 8, p16, None), INVALID, c32)
    relu = "iris_conv3x3_c32_bias_relu"
    refused(lib.iris_conv3x3_c32_bias_relu(p16, p16, None, p16, 1, 8, 8, 0, 0, None), INVALID, relu)   # NULL bias
    refused(lib.iris_conv3x3_c32_bias_relu(p16, p16, p16, None, 1, 8, 8, 1, 1, None), INVALID, relu)
    refused(lib.iris_conv3x3_c32_bias_relu(p16, p16, p16, p16, 1, 8, 0, 0, 1, None), INVALID, relu)

    assert lib.iris_wino_b3_packed_len(16, 64) == 24 * 16 * 64 == 96 * 16 * 64 // 4
    assert lib.iris_wino_b3_packed_len(0, 64) == 0 and lib.iris_wino_b3_packed_len(16, 0) == 0 and lib.iris_wino_b3_packed_len(-16, 64) == 0


def test_product_code_refuses_cpu_tensors():
    import torch
    from challenge_amd import frontend as FE
    x = torch.zeros(2, 3, 4, 2)
    for fn in (FE.complex_to_magphase, FE.minmax_log, FE.magphase_to_complex):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(RuntimeError):
        FE.mask_apply(x, 1, [[0, 1]])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FE.FrontendPlan(1024, 256, 64)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "challenge_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, fn)).read()
                assert "import oracle" not in text and "from oracle" not in text, fn


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    """The device assembly of the library as `make all` compiles it (hipcc cross-compiles gfx950 here, ~30 s, once per module)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "challenge_amd", "csrc", "iris_frontend.hip")
    asm = str(tmp_path_factory.mktemp("asm") / "iris_frontend.s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-S", "--cuda-device-only",
                    "-o", asm, src], check=True, capture_output=True)
    return asm


def test_hot_kernels_use_no_scratch_and_fit_their_wave_budget(device_asm):
    """Static check on the device assembly (hipcc cross-compiles here): no variant of the fused kernel, the STFT kernel or the
    min-max / log kernel may use scratch memory (a kernel with scratch pays ~5 us more per dispatch on this chip, and a spill
    inside the frame loop costs far more - both happened silently during round 4 before this test existed), and every fused
    variant must fit the register budget of the wave count it is launched with (`fused_waves`: 16 waves = 128 VGPRs,
    12 = 168, 8 = 256)."""
    import re
    import subprocess
    asm = device_asm
    name, cur, rows = None, {}, []
    for line in open(asm):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, cur = m.group(1), {}
            continue
        if name:
            m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", line)
            if m:
                cur[m.group(1)] = int(m.group(2))
            if ".end_amdhsa_kernel" in line:
                rows.append((name, cur))
                name = None
    names = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True).stdout.split("\n")
    hot = [(d, c) for (n, c), d in zip(rows, names) if any(k in d for k in ("k_wav_to_mel", "k_stft", "k_minmax_log_apply", "k_magmel"))]
    assert len(hot) >= 120, len(hot)   # the fused variants + the MFMA / STFT / magmel / min-max kernels
    spills = [(d, c["private_segment_fixed_size"]) for d, c in hot if c.get("private_segment_fixed_size", 0)]
    assert not spills, spills
    for d, c in hot:
        m = re.match(r"void k_wav_to_mel<(\d+), (\d+), (true|false), (true|false), 1, (\d)>", d)
        if not m:
            continue
        log2n, mode, hi, bands, fuse = int(m.group(1)), int(m.group(2)), m.group(3) == "true", m.group(4) == "true", int(m.group(5))
        if log2n >= 11:
            waves = 12 if (not bands and not hi and (not fuse or (mode != 2 and fuse != 2))) else 8
        elif log2n == 10:
            waves = 12 if bands else 16
        else:
            waves = 16
        budget = {16: 128, 12: 168, 8: 256}[waves]
        assert c["next_free_vgpr"] <= budget, (d, c["next_free_vgpr"], budget)


def test_hand_set_vmcnt_has_enough_loads_behind_the_staging_rows(device_asm):
    """The fused kernel stages its constant block by LDS-DMA (`global_load_lds_dwordx4` from inline asm) BEFORE the first frame
    loads and waits for it with a hand-set `s_waitcnt vmcnt(P)` (csrc/k_fused.h: a wave's vector-memory operations return in
    order, so once at most P are outstanding the older staging rows have landed).  That is only correct while the compiler
    really issues AT LEAST P vector-memory loads between the last staging row and the wait on every path that loads a frame:
    if it ever merges, widens or sinks those loads, constants would be read from LDS before they arrive - silently wrong
    twiddles / window / mel weights.  Checked here on the assembly of every variant: each basic block between the staging
    loop and the hand-set wait that holds frame loads holds >= P of them."""
    import re
    text = open(device_asm).read()
    fns = re.split(r"\n(?=_Z12k_wav_to_melILi\d+E[^\n]*:\s)", text)
    checked = 0
    for fn in fns[1:]:
        head = fn.split(":", 1)[0]
        body = fn.split(".end_amdhsa_kernel")[0] if ".end_amdhsa_kernel" in fn else fn
        body = body.split("s_endpgm")[0]
        lines = body.split("\n")
        # the hand-set wait: `s_waitcnt vmcnt(N)`, N > 0, as the only instruction of an inline-asm statement
        wait_at, n_wait = None, None
        for i, ln in enumerate(lines):
            m = re.match(r"\s*s_waitcnt vmcnt\((\d+)\)\s*$", ln)
            if m and int(m.group(1)) > 0 and i > 0 and "ASMSTART" in lines[i - 1] and "ASMEND" in lines[i + 1]:
                wait_at, n_wait = i, int(m.group(1))
                break
        if wait_at is None:
            continue   # variants without direct frame loads have no hand-set wait
        log2n = int(re.match(r"_Z12k_wav_to_melILi(\d+)E", head).group(1))
        assert n_wait == (1 << log2n) // 128, (head, n_wait)   # P = points per lane
        dma = [i for i in range(wait_at) if "global_load_lds_dwordx4" in lines[i]]
        assert dma, head
        # basic blocks of the region in between: split at labels and branches
        blocks, cur = [], 0
        for ln in lines[dma[-1] + 1:wait_at]:
            t = ln.strip()
            if re.match(r"\.LBB\d+_\d+:", t) or t.startswith(("s_cbranch", "s_branch")):
                blocks.append(cur)
                cur = 0
            elif re.match(r"global_load_(dword|dwordx2|dwordx3|dwordx4|ubyte|ushort)\b", t):
                cur += 1
        blocks.append(cur)
        loaded = [b for b in blocks if b]
        assert loaded and min(loaded) >= n_wait, (head, n_wait, blocks)
        checked += 1
    assert checked >= 60, checked   # every direct-load variant of the fused kernel (with / without epilogue, bands, mel modes)


def test_winograd_kernel_hand_set_waits_match_its_requests(device_asm):
    """k_conv3x3_wino stages its operands by LDS-DMA from inline asm and waits with hand-set counters (csrc/k_conv_wino.h): in
    every steady-state chunk body the wave requests 7 rows of input, then 8 rows of U, and `s_waitcnt vmcnt(8)` in front of the
    patch reads relies on exactly that order - a wave's vector-memory operations return in order, so at most the 8 YOUNGER U
    requests may be outstanding once the input has landed.  Checked on the assembly of all twelve variants (pooled or not x
    tile columns x input layout, + the six BatchNorm-statistics forms): in each loop body with the 64 MFMAs of a chunk and the hand-set wait, the vector-memory
    instructions in front of the wait are 15 LDS-DMA requests and nothing else, and the loop has no scratch access.  (The
    unpooled variants sit at the 256 + 256 register limit of a one-wave-per-SIMD kernel and keep up to 31 dwords of per-work-item
    geometry in scratch OUTSIDE the chunk loop - stored once, reloaded once per 64 x 64 block; the pooled ones use none.)"""
    import re
    text = open(device_asm).read()
    fns = re.split(r"\n(?=_Z14k_conv3x3_winoILb[01]ELi\d+ELb[01]ELb[01]EE[^\n]*:\s)", text)
    # preamble + 2 (pooled or not) x 3 (tile columns) x 2 (chunked / channels-last input) + the 6 unpooled forms that also accumulate
    # the BatchNorm statistics in their epilogue (template parameter BN)
    assert len(fns) == 19, len(fns)
    checked = 0
    for fn in fns[1:]:
        head = fn.split(":", 1)[0]
        body = fn.split("s_endpgm")[0]
        blocks, cur = [], []
        for ln in body.split("\n"):
            t = ln.strip()
            if re.match(r"\.LBB\d+_\d+:", t):
                blocks.append(cur)
                cur = []
            elif t and not t.startswith(";"):
                cur.append(t)
        blocks.append(cur)
        loops = [b for b in blocks if sum(1 for t in b if t.startswith("v_mfma_f32_32x32x2")) == 64 and "s_waitcnt vmcnt(8)" in b]
        assert len(loops) == 2, (head, len(loops))   # one copy of the loop per transform half (wave-uniform branch)
        for b in loops:
            upto = b[:b.index("s_waitcnt vmcnt(8)")]
            vmem = [t.split()[0] for t in upto if re.match(r"(global|buffer|flat|scratch)_", t)]
            assert vmem == ["global_load_lds_dwordx4"] * 15, (head, vmem)
            assert not any(t.startswith("scratch_") for t in b), head
            checked += 1
        scratch = int(re.search(r"\.amdhsa_kernel " + re.escape(head) + r"\s.*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S).group(1))
        pooled = head.startswith("_Z14k_conv3x3_winoILb1")
        # (unpooled forms: a few dozen bytes of spilled epilogue / prologue state outside the K loop - 120-132 bytes since round 6,
        # when the epilogue also accumulates the BatchNorm statistics; the loop itself is checked scratch-free above)
        assert scratch == 0 if pooled else scratch <= 160, (head, scratch)
    assert checked == 36


def test_winograd_weight_gradient_kernel_fits_two_waves_per_simd(device_asm):
    """k_wino_wrw (csrc/k_conv_wino_wrw.h) hides memory latency with TWO waves per SIMD: workgroups of 512 threads need at most
    256 registers per lane (vector + accumulation), no scratch; its transform is written as packed adds (11 v_pk_add_f32 per
    tile and position half) and a tile costs 8 MFMAs and 10 loads."""
    import re
    text = open(device_asm).read()
    m = re.search(r"\.amdhsa_kernel _Z10k_wino_wrwILi2ELi2EEvPKfS1_Pfiiiiii\s(.*?)\.end_amdhsa_kernel", text, re.S)
    assert m
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1)) == 0
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(1)).group(1)) <= 256
    body = text.split("\n_Z10k_wino_wrwILi2ELi2EEvPKfS1_Pfiiiiii:", 1)[1].split("s_endpgm")[0]
    assert not re.search(r"\bscratch_", body)
    blocks, cur = [], []
    for ln in body.split("\n"):
        t = ln.strip()
        if re.match(r"\.LBB\d+_\d+:", t):
            blocks.append(cur)
            cur = []
        elif t and not t.startswith(";"):
            cur.append(t)
    blocks.append(cur)
    n_mfma = [sum(t.startswith("v_mfma_f32_32x32x2") for t in b) for b in blocks]
    n_load = [sum(t.startswith("buffer_load_dword ") for t in b) for b in blocks]
    # both position halves x the four slots of the unrolled load ring: a tile = 8 MFMAs, and 6 + 4 loads (a lane keeps the
    # column transform of the two patch columns it shares with its next tile; only the first tile of a row loads 6 more)
    assert sum(n == 8 for n in n_mfma) >= 8 and set(n_mfma) <= {0, 8}, sorted(set(n_mfma))
    assert sum(n == 10 for n in n_load) >= 8 and sum(n == 6 for n in n_load) >= 8, sorted(set(n_load))
    assert body.count("v_pk_add_f32") >= 2 * 9


def test_winograd_weight_gradient_argument_checks():
    """iris_conv3x3_wino_wrw refuses what the kernel does not cover before touching the device."""
    lib = N.lib()
    import ctypes as C
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert lib.iris_wino_wrw_workspace_len(4, 8, 8, 64, 128) in (0, 16 * 64 * 128 * 16) or lib.iris_wino_wrw_workspace_len(4, 8, 8, 64, 128) % (16 * 64 * 128) == 0
    assert lib.iris_wino_wrw_workspace_len(4, 8, 8, 16, 128) == 0
    assert lib.iris_conv3x3_wino_wrw(None, p, p, 1, 1, 1, 1, 1, 4, 4, 64, 64, 0, p, 16, None) == -1
    assert lib.iris_conv3x3_wino_wrw(p, p, p, 1, 1, 1, 1, 0, 4, 4, 64, 64, 0, p, 16, None) == -1
    assert lib.iris_conv3x3_wino_wrw(p, p, p, 1, 1, 1, 1, 1, 4, 4, 16, 64, 0, p, 16, None) == -2
    assert lib.iris_conv3x3_wino_wrw(p, p, p, 1, 1, 1, 1, 1, 4, 4, 64, 48, 0, p, 16, None) == -2
    assert lib.iris_conv3x3_wino_wrw(p, p, p, 1, 1, 1, 1, 4096, 64, 64, 64, 64, 0, p, 16, None) == -2   # 2^32 bytes


def test_winograd_weight_packing_on_the_host():
    """iris_wino_pack_weights (host code, no GPU): U = G g G^T per (cout, cin), stored in the kernel's LDS order
    [cout block][chunk of 8 cin][position 16][pair 2][hl 2][cout 64][2] with channel 4 pair + 2 hl + j of the chunk at (pair, hl, j)."""
    import numpy as np
    lib = N.lib()
    rng = np.random.default_rng(0)
    cin, cout = 16, 128
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    out = np.empty(lib.iris_wino_packed_len(cin, cout), np.float32)
    assert out.size == 16 * cin * cout
    assert lib.iris_wino_pack_weights(w.ctypes.data, cin, cout, out.ctypes.data) == 0
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
    U = np.einsum("xi,ocij,yj->ocxy", G, w.astype(np.float64), G)          # [cout, cin, 4, 4]
    packed = out.reshape(cout // 64, cin // 8, 16, 2, 2, 64, 2)
    for o, c in [(0, 0), (5, 3), (63, 7), (64, 8), (127, 15), (70, 10)]:
        k = c % 8
        got = packed[o // 64, c // 8, :, k >> 2, (k >> 1) & 1, o % 64, k & 1]
        assert np.allclose(got, U[o, c].reshape(16).astype(np.float32), rtol=0, atol=1e-7), (o, c)
    # every element is used exactly once: the packed tensor is a permutation of U
    assert np.allclose(np.sort(out), np.sort(U.astype(np.float32).ravel()), atol=1e-7)
