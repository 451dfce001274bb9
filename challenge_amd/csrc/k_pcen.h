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
};

__device__ __forceinline__ int pcen_pad(int e) { return e + (e >> 5); }

__device__ __forceinline__ float pcen_value(float e, float m, const PcenArgs& a) {
    const float l = a.log_eps + log1pf(m * a.inv_eps);   // ln(eps + M)
    const float arg = fmaf(-a.gain, l, -a.log_bias);    // ln((eps + M)^-a / d)
    // E (eps + M)^-a / d; where exp(arg) would overflow fp32 (gain above ~6) the product is formed in the log domain.
    // Either way E == 0 gives exactly 0 and a NaN in E or M gives NaN.
    const float q = arg < 80.f ? e * expf(arg) : expf(logf(e) + arg);
    return a.bias_pow * expm1f(a.power * log1pf(q));
}

// kSmoother: write M instead of the PCEN output (iris_pcen_smoother)
template <bool kSmoother>
__global__ __launch_bounds__(kPcenThreads) void k_pcen(PcenArgs a) {
    __shared__ float tile[kPcenLds];
    __shared__ float s_a[kPcenThreads], s_b[kPcenThreads];
    __shared__ float carry[kPcenThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cols = a.cols, c0 = blockIdx.y * kPcenThreads;
    const int ncol = min(cols, a.n_inner - c0);                   // columns of this workgroup
    const int c = tid % cols, seg = tid / cols;
    const bool active = seg < a.nseg && c < ncol;
    const int last_active = a.nseg * cols - 1;
    const size_t row_off = (size_t)blockIdx.x * a.n_time * a.n_inner;
    const float* src_row = a.x + row_off;
    float* dst_row = a.y + row_off;
    const bool contiguous = ncol == a.n_inner;                    // the tile is one contiguous span of the row
    const int tile_frames = a.nseg * a.run;
    if (tid < cols) carry[tid] = 0.f;

    for (int t0 = 0; t0 < a.n_time; t0 += tile_frames) {
        const int len = min(tile_frames, a.n_time - t0);
        const int n_el = len * ncol;
        // ---- load the tile (frames t0 .. t0 + len - 1, columns c0 .. c0 + ncol - 1) ----
        if (contiguous) {
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
                tile[pcen_pad(i)] = src_row[(size_t)(t0 + f) * a.n_inner + c0 + cc];
            }
        }
        __syncthreads();

        // ---- pass 1: the affine map of this thread's run, from zero ----
        const int f_beg = seg * a.run, f_end = active ? min(f_beg + a.run, len) : f_beg;
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
        // ---- compose the maps of column c: inclusive scan over the runs within the wave ----
        for (int d = cols; d < 64; d <<= 1) {
            const float pA = __shfl_up(mA, d), pB = __shfl_up(mB, d);
            if (lane >= d) {
                mB = fmaf(mA, pB, mB);
                mA *= pA;
            }
        }
        s_a[tid] = mA;
        s_b[tid] = mB;
        __syncthreads();
        // exclusive value: the carry of the previous tile, through the earlier waves' runs of column c, through this
        // wave's earlier runs of column c
        float m_in = carry[c];
        for (int w = 0; w < wave; ++w) {
            const int hi = min(64 * w + 63, last_active);
            const int t = hi - (((hi - c) % cols) + cols) % cols;    // last thread <= hi holding column c
            if (t >= 64 * w) m_in = fmaf(s_a[t], m_in, s_b[t]);
        }
        if (lane >= cols) m_in = fmaf(s_a[tid - cols], m_in, s_b[tid - cols]);

        // ---- pass 2: the run again from its exact start; output into the tile ----
        float m = m_in;
        for (int f = f_beg; f < f_end; ++f) {
            const int li = pcen_pad(f * ncol + c);
            const float e = tile[li];
            m = (t0 + f == 0) ? e : fmaf(a.s, e, a.om * m);
            tile[li] = kSmoother ? m : pcen_value(e, m, a);
        }
        __syncthreads();   // every thread has read its carry and written its outputs
        if (active && seg == a.nseg - 1) carry[c] = m;            // state after the tile's last frame of column c

        // ---- store the tile ----
        if (contiguous) {
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
                dst_row[(size_t)(t0 + f) * a.n_inner + c0 + cc] = tile[pcen_pad(i)];
            }
        }
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

template <bool kSmoother>
static int pcen_launch(PcenArgs& a, int n_rows, int n_time, int n_inner, float smooth, void* stream) {
    a.n_time = n_time;
    a.n_inner = n_inner;
    a.cols = std::min(n_inner, kPcenThreads);
    a.nseg = kPcenThreads / a.cols;
    a.run = (int)std::min<long long>(std::max<long long>(((long long)n_time + a.nseg - 1) / a.nseg, 1), kPcenMaxRun);
    a.s = smooth;
    a.om = 1.f - smooth;
    const dim3 grid((unsigned)n_rows, (unsigned)((n_inner + kPcenThreads - 1) / kPcenThreads));
    k_pcen<kSmoother><<<grid, kPcenThreads, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
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
