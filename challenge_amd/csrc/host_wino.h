// host_wino.h -- host side of the Winograd convolutions: the device packers' entry points and one launch path for both kernel
// families, k_conv_wino.h (fp32 matrix cores, traits WinoF32) and k_conv_wino_b3.h (split-bf16 matrix cores, traits WinoB3).
// Part of the single translation unit iris_frontend.hip (and of scripts/microbench/wino_conv.hip), included after both.
#pragma once

// The argument checks of every device packing: `kc` input channels per chunk of the kernel family; `job` >= 0: the job of
// iris_wino_pack_weights_device_multi the message names
static int wino_pack_check(const char* name, int job, int kc, const void* weight, const void* packed, int cin, int cout) {
    char why[96];
    int code = IRIS_E_INVALID;
    if (!weight || !packed) {
        snprintf(why, sizeof(why), "%s", job < 0 ? "NULL argument" : "NULL pointer");
    } else if (cin <= 0 || cout <= 0 || (cin % kc) || (cout % 64)) {
        code = IRIS_E_UNSUPPORTED;
        snprintf(why, sizeof(why), "cin %d must be a multiple of %d, cout %d of 64", cin, kc, cout);
    } else if (reinterpret_cast<uintptr_t>(packed) & 15) {
        snprintf(why, sizeof(why), "packed must be 16-byte aligned");
    } else {
        return IRIS_OK;
    }
    return job < 0 ? fail(code, "%s: %s", name, why) : fail(code, "%s: job %d: %s", name, job, why);
}

extern "C" int iris_wino_pack_weights_device(const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, int cin,
                                             int cout, int transposed, float* packed, void* stream) {
    if (const int rc = wino_pack_check("iris_wino_pack_weights_device", -1, kWinoKC, weight, packed, cin, cout)) return rc;
    k_wino_pack<<<(unsigned)((cout / kWinoTN) * (cin / kWinoKC)), 512, 0, (hipStream_t)stream>>>(weight, stride_o, stride_i, stride_h, stride_w,
                                                                                                 cin, cout, transposed, packed);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_wino_b3_pack_weights_device(const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, int cin,
                                                int cout, int transposed, float* packed, void* stream) {
    if (const int rc = wino_pack_check("iris_wino_b3_pack_weights_device", -1, kB3KC, weight, packed, cin, cout)) return rc;
    k_wino_pack_b3<<<(unsigned)((cout / 64) * (cin / kB3KC)), 128, 0, (hipStream_t)stream>>>(weight, stride_o, stride_i, stride_h, stride_w, cin,
                                                                                             cout, transposed, reinterpret_cast<uint4*>(packed));
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_wino_pack_weights_device_multi(iris_pack_job* jobs_host, int n_jobs, int split_bf16, void* stream) {
    if (!jobs_host || n_jobs <= 0) return fail(IRIS_E_INVALID, "iris_wino_pack_weights_device_multi: no jobs");
    const int kc = split_bf16 ? kB3KC : kWinoKC;
    for (int i = 0; i < n_jobs; ++i) {
        const iris_pack_job& jb = jobs_host[i];
        if (const int rc = wino_pack_check("iris_wino_pack_weights_device_multi", i, kc, jb.weight, jb.packed, jb.cin, jb.cout)) return rc;
    }
    for (int base = 0; base < n_jobs; base += kWinoPackMaxJobs) {
        WinoPackJobs jobs;
        jobs.n = std::min(kWinoPackMaxJobs, n_jobs - base);
        jobs.pad = 0;
        long long blocks = 0;
        for (int i = 0; i < jobs.n; ++i) {
            iris_pack_job& jb = jobs_host[base + i];
            jb.first_block = (int)blocks;
            jobs.j[i] = jb;
            blocks += (long long)(jb.cout / 64) * (jb.cin / kc);
        }
        if (blocks >= 2147483647LL) return fail(IRIS_E_UNSUPPORTED, "iris_wino_pack_weights_device_multi: too many blocks");
        if (split_bf16) k_wino_pack_b3_multi<<<(unsigned)blocks, 128, 0, (hipStream_t)stream>>>(jobs);
        else k_wino_pack_multi<<<(unsigned)blocks, 512, 0, (hipStream_t)stream>>>(jobs);
        HIP_TRY(hipGetLastError());
    }
    return IRIS_OK;
}

// one form (POOL, IN_NHWC, BN) of kernel family K at the tile columns `tc` of the geometry
template <typename K, bool POOL, bool IN_NHWC, bool BN, typename... Args>
static hipError_t wino_launch(int tc, unsigned grid, hipStream_t s, Args... args) {
    if (tc >= 64) K::template kernel<POOL, 64, IN_NHWC, BN><<<grid, 256, K::kLdsBytes, s>>>(args...);
    else if (tc >= 32) K::template kernel<POOL, 32, IN_NHWC, BN><<<grid, 256, K::kLdsBytes, s>>>(args...);
    else K::template kernel<POOL, 16, IN_NHWC, BN><<<grid, 256, K::kLdsBytes, s>>>(args...);
    return hipGetLastError();
}

// The convolution of either family (K: its traits; `name`: the entry point, for the messages).  Both kernels work on blocks of
// 64 tiles x 64 output channels; the grid is persistent, one workgroup (4 waves, one per SIMD) per CU.
// x: channel-chunked [B][cin / 8][H][W][8] (IRIS_WINO_IN_NHWC: channels-last [B][H][W][cin]); packed: the family's packer; bias:
// nullable; y: chunked [B][cout / 8][Ho][Wo][8] (IRIS_WINO_OUT_NHWC: channels-last [B][Ho][Wo][cout]); flags = IRIS_WINO_*;
// bn_sums: the `_bn` forms' statistics (nullptr otherwise)
template <typename K>
static int conv3x3_wino_run(const char* name, const float* x, const float* packed, const float* bias, float* y, int batch, int height,
                            int width, int cin, int cout, int flags, double* bn_sums, void* stream) {
    if (!x || !packed || !y) return fail(IRIS_E_INVALID, "%s: NULL argument", name);
    if (bn_sums && (bias || (flags & (IRIS_WINO_POOL | IRIS_WINO_RELU)) || !(flags & IRIS_WINO_OUT_NHWC)))
        return fail(IRIS_E_INVALID, "%s_bn: the statistics are those of the bare convolution, channels-last out (no bias / ReLU / pooling)", name);
    if (batch <= 0 || height <= 0 || width <= 0) return fail(IRIS_E_INVALID, "%s: empty tensor", name);
    if (flags & ~(IRIS_WINO_POOL | IRIS_WINO_OUT_NHWC | IRIS_WINO_IN_NHWC | IRIS_WINO_RELU)) return fail(IRIS_E_INVALID, "%s: flags 0x%x", name, flags);
    if (cin <= 0 || cout <= 0 || (cin % K::kKC) || (cout % 64))
        return fail(IRIS_E_UNSUPPORTED, "%s: cin %d must be a multiple of %d, cout %d of 64", name, cin, K::kKC, cout);
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(packed)) & 15)
        return fail(IRIS_E_INVALID, "%s: x and the packed weights must be 16-byte aligned", name);
    if ((long long)batch * height * width * cin >= 1073741824LL)
        return fail(IRIS_E_UNSUPPORTED, "%s: tensor too large for 32-bit byte offsets (>= 2^30 elements)", name);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::atomic<unsigned> lds_set[64];   // one per family
#define WINO_TCS(P, I, B) K::template kernel<P, 64, I, B>, K::template kernel<P, 32, I, B>, K::template kernel<P, 16, I, B>
    HIP_TRY(set_max_lds_once(lds_set, dev, K::kLdsBytes, WINO_TCS(false, false, false), WINO_TCS(false, true, false), WINO_TCS(true, false, false),
                             WINO_TCS(true, true, false), WINO_TCS(false, false, true), WINO_TCS(false, true, true)));
#undef WINO_TCS
    const int pool = (flags & IRIS_WINO_POOL) != 0, out_nhwc = (flags & IRIS_WINO_OUT_NHWC) != 0;
    const int in_nhwc = (flags & IRIS_WINO_IN_NHWC) != 0, relu = (flags & IRIS_WINO_RELU) != 0;
    const int th = (height + 1) / 2, tw = (width + 1) / 2;
    const int tc = tw > 32 ? 64 : (tw > 16 ? 32 : 16), tr = 64 / tc;
    const long long n_work = (((long long)batch * th + tr - 1) / tr) * ((tw + tc - 1) / tc) * (cout / 64);
    if (n_work >= 2147483647LL) return fail(IRIS_E_UNSUPPORTED, "%s: too many tiles", name);
    const unsigned grid = (unsigned)std::min<long long>(n_work, device_cu_count(dev));
    const hipStream_t st = (hipStream_t)stream;
    const typename K::Packed pk = reinterpret_cast<typename K::Packed>(packed);
    hipError_t e;   // (bn_sums is nullptr unless BN: the statistics go with neither pooling nor bias)
    if (pool) e = in_nhwc ? wino_launch<K, true, true, false>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums)
                          : wino_launch<K, true, false, false>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums);
    else if (bn_sums) e = in_nhwc ? wino_launch<K, false, true, true>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums)
                                  : wino_launch<K, false, false, true>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums);
    else e = in_nhwc ? wino_launch<K, false, true, false>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums)
                     : wino_launch<K, false, false, false>(tc, grid, st, x, pk, bias, y, batch, height, width, cin, cout, out_nhwc, relu, bn_sums);
    HIP_TRY(e);
    return IRIS_OK;
}

// packed: iris_wino_pack_weights[_device]
extern "C" int iris_conv3x3_wino(const float* x, const float* packed, const float* bias, float* y, int batch, int height, int width,
                                 int cin, int cout, int flags, void* stream) {
    return conv3x3_wino_run<WinoF32>("iris_conv3x3_wino", x, packed, bias, y, batch, height, width, cin, cout, flags, nullptr, stream);
}
// The training form (bare convolution, flags = IRIS_WINO_OUT_NHWC [| IRIS_WINO_IN_NHWC]) that ALSO accumulates the statistics of
// the BatchNorm behind it: bn_sums_zeroed = DEVICE double [iris_bn_sums_len(cout)], zero on entry, consumed by
// iris_bn_relu_apply_sums0 / iris_bn_relu_pool_apply_sums0 (no iris_bn_stats pass over z)
extern "C" int iris_conv3x3_wino_bn(const float* x, const float* packed, float* y, int batch, int height, int width, int cin, int cout,
                                    int flags, double* bn_sums_zeroed, void* stream) {
    if (!bn_sums_zeroed) return fail(IRIS_E_INVALID, "iris_conv3x3_wino_bn: NULL argument");
    return conv3x3_wino_run<WinoF32>("iris_conv3x3_wino", x, packed, nullptr, y, batch, height, width, cin, cout, flags, bn_sums_zeroed, stream);
}

// packed: iris_wino_b3_pack_weights_device; cin % 16 == 0
extern "C" int iris_conv3x3_wino_b3(const float* x, const float* packed, const float* bias, float* y, int batch, int height, int width,
                                    int cin, int cout, int flags, void* stream) {
    return conv3x3_wino_run<WinoB3>("iris_conv3x3_wino_b3", x, packed, bias, y, batch, height, width, cin, cout, flags, nullptr, stream);
}
// as iris_conv3x3_wino_bn: the bare convolution + the statistics of the BatchNorm behind it
extern "C" int iris_conv3x3_wino_b3_bn(const float* x, const float* packed, float* y, int batch, int height, int width, int cin, int cout,
                                       int flags, double* bn_sums_zeroed, void* stream) {
    if (!bn_sums_zeroed) return fail(IRIS_E_INVALID, "iris_conv3x3_wino_b3_bn: NULL argument");
    return conv3x3_wino_run<WinoB3>("iris_conv3x3_wino_b3", x, packed, nullptr, y, batch, height, width, cin, cout, flags, bn_sums_zeroed, stream);
}
