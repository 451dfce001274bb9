// k_pcen.h -- per-channel energy normalisation (PCEN) of mel magnitudes: a first-order IIR smoother along time, then
// adaptive gain control and root compression (Wang et al. 2017; Lostanlen et al. 2019).
// Part of the single translation unit iris_frontend.hip.
//
// x is viewed as [n_rows, n_time, n_inner]; every (row, inner) sequence runs
//     M[0] = E[0],  M[t] = (1 - s) M[t-1] + s E[t]
//     out  = d^r expm1(r log1p(E exp(-a (log eps + log1p(M / eps))) / d))
// A workgroup owns one row (and up to 256 of its inner columns) and walks it in tiles:
//   1. the tile's frames x columns are loaded into LDS, coalesced (float4 where aligned);
//   2. thread (c, seg) owns column c and R consecutive frames of the tile: it runs the recurrence from zero over its
//      run, which gives the affine map M_out = A M_in + B of the run (A = (1 - s)^len, B = the zero-start result);
//   3. the maps of one column are composed across the runs of a wave with __shfl_up (stride = columns), across the
//      waves through LDS, and onto the carry of the previous tile: each thread gets the exact M entering its run;
//   4. the thread re-runs its frames sequentially from that M (the same op order as a per-frame loop), writes the
//      output back into the LDS tile, and the tile is stored coalesced.  The run holding frame 0 of the row starts
//      from M = E[0] with A = 0, so no carry reaches it.
// Every value is a fixed sequence of fp32 operations: bitwise reproducible, no atomics, no host synchronisation;
// in place (y == x) is safe because a tile is entirely in LDS before any of it is stored.
// k_pcen<false, true> (iris_pcen_banded) is the same kernel with s, a, d, r of band = row % n_bands read from a device array: the
// forward of the trainable layer; its gradient kernel (k_pcen_grad.h) shares the tile, map and scan functions below.
#pragma once

constexpr int kPcenThreads = 256;
constexpr int kPcenMaxRun = 16;                                   // frames per thread per tile (R)
constexpr int kPcenTile = kPcenThreads * kPcenMaxRun;             // floats per tile, at most
constexpr int kPcenLds = kPcenTile + kPcenTile / 32;              // + one pad dword per 32

struct PcenArgs {
    const float* x;
    float* y;
    int n_time, n_inner;
    int cols;            // inner columns per workgroup: min(n_inner, 256)
    int run;             // R: frames per thread per tile
    int nseg;            // runs per column per tile: 256 / cols
    float s, om;         // s, 1 - s
    float gain, power;   // a, r
    float inv_eps, log_eps, log_bias, bias_pow;  // 1 / eps, ln eps, ln d, d^r
    float eps;           // (banded forms only)
    // the banded forms (iris_pcen_banded, iris_pcen_banded_grad): s, a, d, r of band = row % n_bands come from the device
    // array params[4][n_bands] and the constants above are formed by the workgroup (pcen_band_constants)
    const float* params;
    int n_bands;
    float bias;          // d (banded forms only)
};

__device__ __forceinline__ int pcen_pad(int e) { return e + (e >> 5); }

__device__ __forceinline__ float pcen_log_m(float m, const PcenArgs& a) { return a.log_eps + log1pf(m * a.inv_eps); }   // ln(eps + M)

// E (eps + M)^-a / d from l = ln(eps + M); where exp(arg) would overflow fp32 (gain above ~6) the product is formed in the
// log domain.  Either way E == 0 gives exactly 0 and a NaN in E or M gives NaN.
__device__ __forceinline__ float pcen_qd(float e, float l, const PcenArgs& a) {
    const float arg = fmaf(-a.gain, l, -a.log_bias);    // ln((eps + M)^-a / d)
    return arg < 80.f ? e * expf(arg) : expf(logf(e) + arg);
}

__device__ __forceinline__ float pcen_value(float e, float m, const PcenArgs& a) {
    return a.bias_pow * expm1f(a.power * log1pf(pcen_qd(e, pcen_log_m(m, a), a)));
}

// the per-band constants of a row, formed on the device from params[4][n_bands] (s, a, d, r)
__device__ __forceinline__ void pcen_band_constants(PcenArgs& a, int row) {
    const int band = row % a.n_bands;
    a.s = a.params[band];
    a.om = 1.f - a.s;
    a.gain = a.params[a.n_bands + band];
    a.bias = a.params[2 * a.n_bands + band];
    a.power = a.params[3 * a.n_bands + band];
    a.log_bias = logf(a.bias);
    a.bias_pow = powf(a.bias, a.power);
}

// what a thread owns of its workgroup's row: column c and the run `seg` of every tile
struct PcenGeom {
    int tid, lane, wave;
    int cols, ncol;      // columns per workgroup; columns of this workgroup
    int c0, c, seg;
    bool active, contiguous;   // contiguous: the tile is one contiguous span of the row
    int last_active, tile_frames;
    size_t row_off;
};

__device__ __forceinline__ PcenGeom pcen_geom(const PcenArgs& a) {
    PcenGeom g;
    g.tid = threadIdx.x, g.lane = g.tid & 63, g.wave = g.tid >> 6;
    g.cols = a.cols, g.c0 = blockIdx.y * kPcenThreads;
    g.ncol = min(g.cols, a.n_inner - g.c0);
    g.c = g.tid % g.cols, g.seg = g.tid / g.cols;
    g.active = g.seg < a.nseg && g.c < g.ncol;
    g.last_active = a.nseg * g.cols - 1;
    g.row_off = (size_t)blockIdx.x * a.n_time * a.n_inner;
    g.contiguous = g.ncol == a.n_inner;
    g.tile_frames = a.nseg * a.run;
    return g;
}

// step 1: frames t0 .. t0 + len - 1, columns c0 .. c0 + ncol - 1 of a row into an LDS tile, coalesced
__device__ __forceinline__ void pcen_load_tile(float* tile, const float* src_row, const PcenArgs& a, const PcenGeom& g, int t0, int len) {
    const int tid = g.tid, ncol = g.ncol, n_el = len * ncol;
    if (g.contiguous) {
        const float* src = src_row + (size_t)t0 * a.n_inner;
        int head = 0;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            head = n_el & ~3;
            for (int i = 4 * tid; i < head; i += 4 * kPcenThreads) {
                const float4 v = *reinterpret_cast<const float4*>(src + i);
                tile[pcen_pad(i)] = v.x;
                tile[pcen_pad(i + 1)] = v.y;
                tile[pcen_pad(i + 2)] = v.z;
                tile[pcen_pad(i + 3)] = v.w;
            }
        }
        for (int i = head + tid; i < n_el; i += kPcenThreads) tile[pcen_pad(i)] = src[i];
    } else {
        for (int i = tid; i < n_el; i += kPcenThreads) {
            const int f = i / ncol, cc = i - f * ncol;
            tile[pcen_pad(i)] = src_row[(size_t)(t0 + f) * a.n_inner + g.c0 + cc];
        }
    }
}

// the same tile back to a row
__device__ __forceinline__ void pcen_store_tile(const float* tile, float* dst_row, const PcenArgs& a, const PcenGeom& g, int t0, int len) {
    const int tid = g.tid, ncol = g.ncol, n_el = len * ncol;
    if (g.contiguous) {
        float* dst = dst_row + (size_t)t0 * a.n_inner;
        int head = 0;
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            head = n_el & ~3;
            for (int i = 4 * tid; i < head; i += 4 * kPcenThreads)
                *reinterpret_cast<float4*>(dst + i) =
                    make_float4(tile[pcen_pad(i)], tile[pcen_pad(i + 1)], tile[pcen_pad(i + 2)], tile[pcen_pad(i + 3)]);
        }
        for (int i = head + tid; i < n_el; i += kPcenThreads) dst[i] = tile[pcen_pad(i)];
    } else {
        for (int i = tid; i < n_el; i += kPcenThreads) {
            const int f = i / ncol, cc = i - f * ncol;
            dst_row[(size_t)(t0 + f) * a.n_inner + g.c0 + cc] = tile[pcen_pad(i)];
        }
    }
}

// The affine map of the smoother over a run of frames, M_out = A M_in + B.  A Map has kN floats v[], `compose_after`
// (this map after an earlier one) and a State that `apply` carries through a map; k_pcen_grad.h scans the
// (M, dM / ds) pair with a four-float map through the same pcen_scan_exclusive.
struct PcenMapM {
    static constexpr int kN = 2;
    float v[2];          // A, B
    struct State {
        float m;
        __device__ __forceinline__ void load(const float (*carry)[kPcenThreads], int c) { m = carry[0][c]; }
        __device__ __forceinline__ void apply(const float* w) { m = fmaf(w[0], m, w[1]); }
    };
    __device__ __forceinline__ void compose_after(const float* p) {
        v[1] = fmaf(v[0], p[1], v[1]);
        v[0] *= p[0];
    }
};

// step 3: the maps of one column are composed across the runs of a wave (inclusive scan, __shfl_up with stride = columns)
// and across the waves through LDS, onto the carry of the previous tile: returns the exact state entering this thread's run.
// Holds one __syncthreads: every thread of the workgroup calls it.
template <class Map>
__device__ __forceinline__ typename Map::State pcen_scan_exclusive(Map m, const float (*carry)[kPcenThreads],
                                                                   float (*s_map)[kPcenThreads], const PcenGeom& g) {
    const int cols = g.cols, tid = g.tid;
    for (int d = cols; d < 64; d <<= 1) {
        float p[Map::kN];
#pragma unroll
        for (int k = 0; k < Map::kN; ++k) p[k] = __shfl_up(m.v[k], d);
        if (g.lane >= d) m.compose_after(p);
    }
#pragma unroll
    for (int k = 0; k < Map::kN; ++k) s_map[k][tid] = m.v[k];
    __syncthreads();
    // exclusive value: the carry of the previous tile, through the earlier waves' runs of column c, through this
    // wave's earlier runs of column c
    typename Map::State st;
    st.load(carry, g.c);
    float w[Map::kN];
    for (int wv = 0; wv < g.wave; ++wv) {
        const int hi = min(64 * wv + 63, g.last_active);
        const int t = hi - (((hi - g.c) % cols) + cols) % cols;    // last thread <= hi holding column c
        if (t >= 64 * wv) {
#pragma unroll
            for (int k = 0; k < Map::kN; ++k) w[k] = s_map[k][t];
            st.apply(w);
        }
    }
    if (g.lane >= cols) {
#pragma unroll
        for (int k = 0; k < Map::kN; ++k) w[k] = s_map[k][tid - cols];
        st.apply(w);
    }
    return st;
}

// kSmoother: write M instead of the PCEN output (iris_pcen_smoother); kBanded: per-band parameters from a.params
template <bool kSmoother, bool kBanded = false>
__global__ __launch_bounds__(kPcenThreads) void k_pcen(PcenArgs a) {
    __shared__ float tile[kPcenLds];
    __shared__ float s_map[PcenMapM::kN][kPcenThreads];
    __shared__ float carry[1][kPcenThreads];
    if (kBanded) pcen_band_constants(a, blockIdx.x);
    const PcenGeom g = pcen_geom(a);
    const int ncol = g.ncol, c = g.c;
    const float* src_row = a.x + g.row_off;
    float* dst_row = a.y + g.row_off;
    if (g.tid < g.cols) carry[0][g.tid] = 0.f;

    for (int t0 = 0; t0 < a.n_time; t0 += g.tile_frames) {
        const int len = min(g.tile_frames, a.n_time - t0);
        pcen_load_tile(tile, src_row, a, g, t0, len);
        __syncthreads();

        // ---- pass 1: the affine map of this thread's run, from zero ----
        const int f_beg = g.seg * a.run, f_end = g.active ? min(f_beg + a.run, len) : f_beg;
        float mA = 1.f, mB = 0.f;
        for (int f = f_beg; f < f_end; ++f) {
            const float e = tile[pcen_pad(f * ncol + c)];
            if (t0 + f == 0) {
                mB = e;
                mA = 0.f;
            } else {
                mB = fmaf(a.s, e, a.om * mB);
                mA *= a.om;
            }
        }
        const float m_in = pcen_scan_exclusive<PcenMapM>(PcenMapM{{mA, mB}}, carry, s_map, g).m;

        // ---- pass 2: the run again from its exact start; output into the tile ----
        float m = m_in;
        for (int f = f_beg; f < f_end; ++f) {
            const int li = pcen_pad(f * ncol + c);
            const float e = tile[li];
            m = (t0 + f == 0) ? e : fmaf(a.s, e, a.om * m);
            tile[li] = kSmoother ? m : pcen_value(e, m, a);
        }
        __syncthreads();   // every thread has read its carry and written its outputs
        if (g.active && g.seg == a.nseg - 1) carry[0][c] = m;     // state after the tile's last frame of column c

        pcen_store_tile(tile, dst_row, a, g, t0, len);
        __syncthreads();   // the tile buffer and the carries are reused by the next tile
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int pcen_check(const char* who, const float* x, const float* y, int n_rows, int n_time, int n_inner) {
    if (!x || !y) return fail(IRIS_E_INVALID, "%s: %s is NULL", who, !x ? "mel" : "out");
    if (n_rows <= 0 || n_time <= 0 || n_inner <= 0)
        return fail(IRIS_E_INVALID, "%s: shape [%d, %d, %d] must be positive", who, n_rows, n_time, n_inner);
    if ((size_t)n_time * (size_t)n_inner > (size_t)INT_MAX)
        return fail(IRIS_E_UNSUPPORTED, "%s: a row of %d x %d floats exceeds 2^31 - 1", who, n_time, n_inner);
    if ((n_inner + kPcenThreads - 1) / kPcenThreads > 65535)
        return fail(IRIS_E_UNSUPPORTED, "%s: n_inner %d > %d", who, n_inner, 65535 * kPcenThreads);
    const size_t bytes = (size_t)n_rows * n_time * n_inner * sizeof(float);
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), yb = reinterpret_cast<uintptr_t>(y);
    if (xb != yb && xb < yb + bytes && yb < xb + bytes)
        return fail(IRIS_E_INVALID, "%s: out overlaps mel without being the same tensor (in place means out == mel)", who);
    return IRIS_OK;
}

static int pcen_check_smooth(const char* who, float smooth) {
    if (!std::isfinite(smooth) || !(smooth > 0.f) || smooth > 1.f)
        return fail(IRIS_E_INVALID, "%s: smooth = %g is outside 0 < s <= 1", who, (double)smooth);
    return IRIS_OK;
}

// the tile geometry of a shape; returns the grid
static dim3 pcen_plan(PcenArgs& a, int n_rows, int n_time, int n_inner) {
    a.n_time = n_time;
    a.n_inner = n_inner;
    a.cols = std::min(n_inner, kPcenThreads);
    a.nseg = kPcenThreads / a.cols;
    a.run = (int)std::min<long long>(std::max<long long>(((long long)n_time + a.nseg - 1) / a.nseg, 1), kPcenMaxRun);
    return dim3((unsigned)n_rows, (unsigned)((n_inner + kPcenThreads - 1) / kPcenThreads));
}

template <bool kSmoother, bool kBanded = false>
static int pcen_launch(PcenArgs& a, int n_rows, int n_time, int n_inner, float smooth, void* stream) {
    const dim3 grid = pcen_plan(a, n_rows, n_time, n_inner);
    a.s = smooth;
    a.om = 1.f - smooth;
    k_pcen<kSmoother, kBanded><<<grid, kPcenThreads, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

static int pcen_eps_constants(const char* who, PcenArgs& a, float eps) {
    if (!std::isfinite(eps) || !(eps > 0.f)) return fail(IRIS_E_INVALID, "%s: eps = %g is outside eps > 0", who, (double)eps);
    a.eps = eps;
    a.inv_eps = (float)(1.0 / (double)eps);
    a.log_eps = (float)std::log((double)eps);
    if (!std::isfinite(a.inv_eps)) return fail(IRIS_E_INVALID, "%s: 1 / eps = %g is not a finite float", who, 1.0 / (double)eps);
    return IRIS_OK;
}

// the banded forms' own arguments: the device array params[4][n_bands] and how the rows map onto the bands.  (The values
// live on the device: their ranges are the caller's to guarantee, a check here would need a synchronisation.)
static int pcen_banded_args(const char* who, PcenArgs& a, const float* params, int n_bands, int n_rows, float eps) {
    if (!params) return fail(IRIS_E_INVALID, "%s: params is NULL", who);
    if (n_bands <= 0) return fail(IRIS_E_INVALID, "%s: n_bands = %d must be positive", who, n_bands);
    if (n_rows % n_bands) return fail(IRIS_E_INVALID, "%s: n_rows = %d is not a multiple of n_bands = %d", who, n_rows, n_bands);
    a.params = params;
    a.n_bands = n_bands;
    return pcen_eps_constants(who, a, eps);
}

extern "C" int iris_pcen(const float* mel, float* out, int n_rows, int n_time, int n_inner, float smooth, float gain,
                         float bias, float power, float eps, void* stream) {
    int rc = pcen_check("iris_pcen", mel, out, n_rows, n_time, n_inner);
    if (rc) return rc;
    if ((rc = pcen_check_smooth("iris_pcen", smooth))) return rc;
    if (!std::isfinite(gain) || !(gain >= 0.f)) return fail(IRIS_E_INVALID, "iris_pcen: gain = %g is outside a >= 0", (double)gain);
    if (!std::isfinite(bias) || !(bias > 0.f)) return fail(IRIS_E_INVALID, "iris_pcen: bias = %g is outside d > 0", (double)bias);
    if (!std::isfinite(power) || !(power > 0.f) || power > 1.f)
        return fail(IRIS_E_INVALID, "iris_pcen: power = %g is outside 0 < r <= 1", (double)power);
    if (!std::isfinite(eps) || !(eps > 0.f)) return fail(IRIS_E_INVALID, "iris_pcen: eps = %g is outside eps > 0", (double)eps);
    PcenArgs a{};
    a.x = mel;
    a.y = out;
    a.gain = gain;
    a.power = power;
    // the constants of the output formula, each rounded once from double
    a.inv_eps = (float)(1.0 / (double)eps);
    a.log_eps = (float)std::log((double)eps);
    a.log_bias = (float)std::log((double)bias);
    a.bias_pow = (float)std::pow((double)bias, (double)power);
    if (!std::isfinite(a.inv_eps) || !std::isfinite(a.bias_pow))
        return fail(IRIS_E_INVALID, "iris_pcen: 1 / eps = %g or bias^power = %g is not a finite float", 1.0 / (double)eps,
                    std::pow((double)bias, (double)power));
    return pcen_launch<false>(a, n_rows, n_time, n_inner, smooth, stream);
}

extern "C" int iris_pcen_smoother(const float* mel, float* m_out, int n_rows, int n_time, int n_inner, float smooth,
                                  void* stream) {
    int rc = pcen_check("iris_pcen_smoother", mel, m_out, n_rows, n_time, n_inner);
    if (rc) return rc;
    if ((rc = pcen_check_smooth("iris_pcen_smoother", smooth))) return rc;
    PcenArgs a{};
    a.x = mel;
    a.y = m_out;
    return pcen_launch<true>(a, n_rows, n_time, n_inner, smooth, stream);
}

extern "C" int iris_pcen_banded(const float* mel, float* out, int n_rows, int n_time, int n_inner, const float* params,
                                int n_bands, float eps, void* stream) {
    int rc = pcen_check("iris_pcen_banded", mel, out, n_rows, n_time, n_inner);
    if (rc) return rc;
    PcenArgs a{};
    if ((rc = pcen_banded_args("iris_pcen_banded", a, params, n_bands, n_rows, eps))) return rc;
    a.x = mel;
    a.y = out;
    return pcen_launch<false, true>(a, n_rows, n_time, n_inner, 0.f, stream);
}
