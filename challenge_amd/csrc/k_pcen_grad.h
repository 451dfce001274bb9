// k_pcen_grad.h -- gradient of a scalar loss with respect to the per-band PCEN parameters (iris_pcen_banded_grad): the
// backward half of iris_pcen_banded (k_pcen.h), for the trainable PCEN layer.  Part of the single translation unit
// iris_frontend.hip.
//
// mel is data, so no gradient with respect to it is produced and no reverse scan is needed: the smoother's sensitivity
// G = dM / ds is itself a forward recurrence beside M,
//     M[0] = E[0], G[0] = 0;   M[t] = (1 - s) M[t-1] + s E[t],   G[t] = (1 - s) G[t-1] + (E[t] - M[t-1])
// and a run of frames is the affine map  M_out = A M_in + B,  G_out = A G_in + C M_in + D  of the pair, composed by the
// same chunked scan as k_pcen's (A, B) map (pcen_scan_exclusive).  With qd = E (eps + M)^-a / d (the forward's log1p
// argument), L = log1p(qd), P = r d^(r-1) exp((r - 1) L) = r (q + d)^(r-1):
//     d out / d s = -a P (qd d) G / (eps + M)          d out / d a = -P (qd d) ln(eps + M)
//     d out / d d =  r d^(r-1) expm1((r - 1) L)        d out / d r =  d^r (ln d expm1(r L) + exp(r L) L)
// (the last two in the expm1 / log1p form: their textbook differences cancel for small q).  E == 0 gives exactly zero terms.
//
// k_pcen_grad: a workgroup owns one row (and up to 256 of its inner columns) as in k_pcen, keeps a second LDS tile for
// dout, and every thread adds its dout * d out / d theta products in frame order; the workgroup reduces them in a fixed
// order (wave shuffles, then the four waves through LDS) to four partial sums in the workspace.  k_pcen_grad_reduce: one
// wave per (theta, band) adds that band's partials over batch and column chunks, in a fixed order.  No atomics: the same
// inputs give the same bits.  Nothing is allocated and nothing synchronises; both launches go to the caller's stream.
#pragma once

struct PcenGradArgs {
    PcenArgs p;          // x = mel; y unused
    const float* dout;
    float* partial;      // [n_rows][gridDim.y][4]
};

// the (M, G) pair's map over a run of frames: M_out = A M_in + B, G_out = A G_in + C M_in + D
struct PcenMapMG {
    static constexpr int kN = 4;
    float v[4];          // A, B, C, D
    struct State {
        float m, g;
        __device__ __forceinline__ void load(const float (*carry)[kPcenThreads], int c) { m = carry[0][c], g = carry[1][c]; }
        __device__ __forceinline__ void apply(const float* w) {
            g = fmaf(w[0], g, fmaf(w[2], m, w[3]));
            m = fmaf(w[0], m, w[1]);
        }
        // one frame: e = E[t]
        __device__ __forceinline__ void step(float e, bool first, float s, float om) {
            g = first ? 0.f : fmaf(om, g, e - m);
            m = first ? e : fmaf(s, e, om * m);
        }
    };
    __device__ __forceinline__ void identity() { v[0] = 1.f, v[1] = 0.f, v[2] = 0.f, v[3] = 0.f; }
    __device__ __forceinline__ void step(float e, bool first, float s, float om) {
        if (first) {
            v[0] = 0.f, v[1] = e, v[2] = 0.f, v[3] = 0.f;
        } else {
            v[3] = fmaf(om, v[3], e - v[1]);
            v[2] = fmaf(om, v[2], -v[0]);
            v[1] = fmaf(s, e, om * v[1]);
            v[0] *= om;
        }
    }
    // this map after the earlier map p
    __device__ __forceinline__ void compose_after(const float* p) {
        v[3] = fmaf(v[0], p[3], fmaf(v[2], p[1], v[3]));
        v[2] = fmaf(v[0], p[2], v[2] * p[0]);
        v[1] = fmaf(v[0], p[1], v[1]);
        v[0] *= p[0];
    }
};

__global__ __launch_bounds__(kPcenThreads) void k_pcen_grad(PcenGradArgs ga) {
    __shared__ float tile[kPcenLds], dtile[kPcenLds];
    __shared__ float s_map[PcenMapMG::kN][kPcenThreads];
    __shared__ float carry[2][kPcenThreads];
    __shared__ float s_red[kPcenThreads / 64][4];
    PcenArgs& a = ga.p;
    pcen_band_constants(a, blockIdx.x);
    const PcenGeom g = pcen_geom(a);
    const float* src_row = a.x + g.row_off;
    const float* dsrc_row = ga.dout + g.row_off;
    const float bias = a.bias;
    const float bias_pow_m1 = a.bias_pow / bias;                  // d^(r-1)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                          // s, a, d, r
    if (g.tid < g.cols) carry[0][g.tid] = 0.f, carry[1][g.tid] = 0.f;

    for (int t0 = 0; t0 < a.n_time; t0 += g.tile_frames) {
        const int len = min(g.tile_frames, a.n_time - t0);
        pcen_load_tile(tile, src_row, a, g, t0, len);
        pcen_load_tile(dtile, dsrc_row, a, g, t0, len);
        __syncthreads();

        const int f_beg = g.seg * a.run, f_end = g.active ? min(f_beg + a.run, len) : f_beg;
        PcenMapMG map;
        map.identity();
        for (int f = f_beg; f < f_end; ++f) map.step(tile[pcen_pad(f * g.ncol + g.c)], t0 + f == 0, a.s, a.om);
        PcenMapMG::State st = pcen_scan_exclusive<PcenMapMG>(map, carry, s_map, g);

        for (int f = f_beg; f < f_end; ++f) {
            const int li = pcen_pad(f * g.ncol + g.c);
            const float e = tile[li], dy = dtile[li];
            st.step(e, t0 + f == 0, a.s, a.om);
            const float l = pcen_log_m(st.m, a);                  // ln(eps + M)
            const float qd = pcen_qd(e, l, a);                    // q / d
            const float L = log1pf(qd);
            const float q = qd * bias;
            const float P = a.power * bias_pow_m1 * expf((a.power - 1.f) * L);
            const float t_a = -(P * q) * l;
            const float t_s = -(a.gain * (P * q)) * (st.g / (a.eps + st.m));
            const float t_d = a.power * bias_pow_m1 * expm1f((a.power - 1.f) * L);
            const float t_r = a.bias_pow * fmaf(a.log_bias, expm1f(a.power * L), expf(a.power * L) * L);
            acc[0] = fmaf(dy, t_s, acc[0]);
            acc[1] = fmaf(dy, t_a, acc[1]);
            acc[2] = fmaf(dy, t_d, acc[2]);
            acc[3] = fmaf(dy, t_r, acc[3]);
        }
        __syncthreads();   // every thread has read its carry
        if (g.active && g.seg == a.nseg - 1) carry[0][g.c] = st.m, carry[1][g.c] = st.g;
        __syncthreads();   // the tiles and the carries are reused by the next tile
    }

    // ---- the workgroup's four sums, in a fixed order: lanes of a wave, then the waves ----
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (g.lane == 0) s_red[g.wave][k] = v;
    }
    __syncthreads();
    if (g.tid < 4) {
        float v = s_red[0][g.tid];
        for (int w = 1; w < kPcenThreads / 64; ++w) v += s_red[w][g.tid];
        ga.partial[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 4 + g.tid] = v;
    }
}

// dparams[theta][band] = sum over the rows of the band (row = rep * n_bands + band) and their column chunks.  One wave per
// output: lane l adds entries l, l + 64, ... of the band's list in index order, then a fixed shuffle tree - the same bits
// every run, and the loads of a wave go out together instead of one thread walking the list.
__global__ __launch_bounds__(256) void k_pcen_grad_reduce(const float* partial, float* dparams, int n_rows, int n_bands, int n_chunks) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= 4 * n_bands) return;                                 // (wave-uniform)
    const int theta = i / n_bands, band = i - theta * n_bands;
    const long n = (long)(n_rows / n_bands) * n_chunks;
    float v = 0.f;
    for (long e = lane; e < n; e += 64) {
        const long rep = e / n_chunks, y = e - rep * n_chunks;
        v += partial[((size_t)(rep * n_bands + band) * n_chunks + y) * 4 + theta];
    }
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) dparams[i] = v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" size_t iris_pcen_banded_grad_workspace(int n_rows, int n_time, int n_inner) {
    if (n_rows <= 0 || n_time <= 0 || n_inner <= 0) return 0;
    return 4 * (size_t)n_rows * (size_t)((n_inner + kPcenThreads - 1) / kPcenThreads);
}

extern "C" int iris_pcen_banded_grad(const float* mel, const float* dout, int n_rows, int n_time, int n_inner, const float* params,
                                     int n_bands, float eps, float* dparams, float* workspace, size_t workspace_floats,
                                     void* stream) {
    const char* who = "iris_pcen_banded_grad";
    if (!dout || !dparams) return fail(IRIS_E_INVALID, "%s: %s is NULL", who, !dout ? "dout" : "dparams");
    int rc = pcen_check(who, mel, mel, n_rows, n_time, n_inner);
    if (rc) return rc;
    PcenGradArgs ga{};
    if ((rc = pcen_banded_args(who, ga.p, params, n_bands, n_rows, eps))) return rc;
    const size_t need = iris_pcen_banded_grad_workspace(n_rows, n_time, n_inner);
    if (!workspace || workspace_floats < need)
        return fail(IRIS_E_CAPACITY, "%s: workspace %zu floats < %zu", who, workspace ? workspace_floats : (size_t)0, need);
    ga.p.x = mel;
    ga.dout = dout;
    ga.partial = workspace;
    const dim3 grid = pcen_plan(ga.p, n_rows, n_time, n_inner);
    k_pcen_grad<<<grid, kPcenThreads, 0, (hipStream_t)stream>>>(ga);
    k_pcen_grad_reduce<<<(unsigned)n_bands, 256, 0, (hipStream_t)stream>>>(workspace, dparams, n_rows, n_bands, (int)grid.y);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
