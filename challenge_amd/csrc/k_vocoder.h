// k_vocoder.h -- time stretching of complex spectrograms: a batched phase vocoder (the reference's
// transforms.phase_vocoder, transforms.py:137-195) over a ragged set of sources, each with its own rate, in one launch.
// Part of the single translation unit iris_frontend.hip (after k_pcen.h, whose tile and scan functions it uses).
//
// Per source: X [F, T, 2C] (re block, im block), rate r > 0, output Y [F, n, 2C] with n = ceil(T / r).  Output frame i
// sits at ts = (double)i * r: i0 = floor(ts), alpha = (float)(ts - i0); frames >= T read as zeros.
//     mag[i]   = alpha |X[i0 + 1]| + (1 - alpha) |X[i0]|
//     step[0]  = angle(X[0]);  step[i] = wrap(angle(X[j0 + 1]) - angle(X[j0]) - adv) + adv,  j0 = i0 of frame i - 1
//     phase[i] = step[0] + ... + step[i]   (mod 2 pi),   Y[i] = mag[i] (cos, sin)(phase[i])
// with adv = pi * bin (only adv mod 2 pi matters: pi * (bin & 1)).  The reference accumulates the phase unreduced - it
// reaches pi * bin * i, ~4e5 rad, and fp32 then loses 1e-2 of the peak; here the running phase is kept in [-pi, pi]
// wherever it is stored or carried, so every addition rounds a value of at most ~pi.  Addition modulo 2 pi composes: the
// prefix sum is the chunked scan of k_pcen with an additive map.
//   blockIdx.y = source, blockIdx.x = frequency row; the 256-thread workgroup walks the row's output frames in tiles:
//   1. the input frames a tile needs are one contiguous span of the row ([i0 of the frame before the tile, i0 of its last
//      frame + 1]): loaded into LDS, coalesced (a span too long for the buffer - a very large rate - is read from
//      global memory instead);
//   2. thread (c, seg) owns channel c and R consecutive output frames: it forms their phase steps (kept in registers)
//      and their sum from zero;
//   3. pcen_scan_exclusive composes the sums across runs, waves and the carry of the previous tile;
//   4. the thread walks its frames again from that exact start, writes mag (cos, sin) into the LDS output tile, and the
//      tile is stored coalesced.
// A fixed sequence of fp32 operations per value (the time grid alone is fp64): bitwise reproducible; no atomics, no
// workspace, no synchronisation; every loop bound comes from the descriptor.  r == 1 copies the source bit for bit.
#pragma once

constexpr int kVocMaxRun = 4;                                     // output frames per thread per tile (R)
constexpr int kVocOut = kPcenThreads * kVocMaxRun * 2;            // floats of an output tile (re + im), at most
constexpr int kVocIn = 2 * kVocOut + 1024;                        // floats of an input span held in LDS (rates up to ~2 at full R)
constexpr int kVocOutLds = kVocOut + kVocOut / 32;                // + one pad dword per 32 (pcen_pad)
constexpr int kVocInLds = kVocIn + kVocIn / 32;

static_assert(sizeof(iris_voc_src) == 32, "iris_voc_src is 32 bytes: two pointers, two ints, one double");

// x - 2 pi rint(x / 2 pi) for |x| of a few pi; 2 pi as a float pair, so a reduction adds no error of its own
__device__ __forceinline__ float voc_wrap(float x) {
    const float n = rintf(x * 0.15915494309189533577f);
    return fmaf(-n, -1.7484555e-7f, fmaf(-n, 6.2831854820251465f, x));
}

// running phase: the sum of a run of steps, reduced after every addition
struct VocMapPhase {
    static constexpr int kN = 1;
    float v[1];
    struct State {
        float m;
        __device__ __forceinline__ void load(const float (*carry)[kPcenThreads], int c) { m = carry[0][c]; }
        __device__ __forceinline__ void apply(const float* w) { m = voc_wrap(m + w[0]); }
    };
    __device__ __forceinline__ void compose_after(const float* p) { v[0] = voc_wrap(v[0] + p[0]); }
};

// frames of the row from the LDS span that starts at frame in0 or (span too long) from global memory; frames >= T are zeros
struct VocFrames {
    const float* tile;
    const float* row;
    int in0, n_in, chan2;
    bool staged;
    __device__ __forceinline__ float at(int frame, int comp) const {
        if (frame >= n_in) return 0.f;
        return staged ? tile[pcen_pad((frame - in0) * chan2 + comp)] : row[(size_t)frame * chan2 + comp];
    }
};

__global__ __launch_bounds__(kPcenThreads) void k_phase_vocoder(const iris_voc_src* __restrict__ table, int chan, int max_out_frames) {
    __shared__ float in_tile[kVocInLds];
    __shared__ float out_tile[kVocOutLds];
    __shared__ float s_map[VocMapPhase::kN][kPcenThreads];
    __shared__ float carry[1][kPcenThreads];
    const iris_voc_src d = table[blockIdx.y];
    const int T = d.n_in, n = d.n_out, chan2 = 2 * chan, tid = threadIdx.x;
    const double r = d.rate;
    if (T <= 0 || n <= 0 || n > max_out_frames || !(r > 0.0)) return;   // nothing (or nothing safe) to write
    const float* src_row = static_cast<const float*>(d.src) + (size_t)blockIdx.x * T * chan2;
    float* dst_row = static_cast<float*>(d.dst) + (size_t)blockIdx.x * n * chan2;
    if (r == 1.0) {   // the reference returns its input: a copy (n == T)
        const int n_el = min(n, T) * chan2;
        for (int i = tid; i < n_el; i += kPcenThreads) dst_row[i] = src_row[i];
        return;
    }

    // the row as pcen's tile functions see it: n_inner = 2C floats per frame, all of them this workgroup's
    PcenArgs a{};
    a.n_inner = chan2;
    a.cols = chan;
    a.nseg = kPcenThreads / chan;
    a.run = min(max((n + a.nseg - 1) / a.nseg, 1), kVocMaxRun);
    while (a.run > 1 && (ceil((double)(a.nseg * a.run) * r) + 2.0) * chan2 > (double)kVocIn) --a.run;
    PcenGeom g;        // scan geometry: `chan` columns
    g.tid = tid, g.lane = tid & 63, g.wave = tid >> 6;
    g.cols = chan, g.ncol = chan, g.c0 = 0;
    g.c = tid % chan, g.seg = tid / chan;
    g.active = g.seg < a.nseg;
    g.last_active = a.nseg * chan - 1;
    g.row_off = 0;
    g.contiguous = true;
    g.tile_frames = a.nseg * a.run;
    PcenGeom gt = g;   // tile geometry: 2C floats per frame, one contiguous span
    gt.cols = gt.ncol = chan2;
    const int c = g.c;
    const float adv = (blockIdx.x & 1) ? 3.14159274101257324f : 0.f;
    if (tid < chan) carry[0][tid] = 0.f;

    for (int t0 = 0; t0 < n; t0 += g.tile_frames) {
        const int len = min(g.tile_frames, n - t0);
        // ---- the input span of the tile: frames in0 .. in1 (below T: frames from T on are the zero padding) ----
        VocFrames x;
        x.tile = in_tile, x.row = src_row, x.n_in = T, x.chan2 = chan2;
        x.in0 = (int)floor((double)max(t0 - 1, 0) * r);
        const int in1 = min((int)floor((double)(t0 + len - 1) * r) + 1, T - 1);
        const int n_ld = max(in1 - x.in0 + 1, 0);
        x.staged = (long long)n_ld * chan2 <= (long long)kVocIn;
        if (x.staged) pcen_load_tile(in_tile, src_row, a, gt, x.in0, n_ld);
        __syncthreads();

        // ---- pass 1: the phase steps of this thread's run and their sum from zero ----
        const int f_beg = g.seg * a.run, f_end = g.active ? min(f_beg + a.run, len) : f_beg;
        float step[kVocMaxRun];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kVocMaxRun; ++j) {
            step[j] = 0.f;
            if (f_beg + j < f_end) {
                const int i = t0 + f_beg + j;
                if (i == 0) {
                    step[j] = atan2f(x.at(0, chan + c), x.at(0, c));
                } else {
                    const int j0 = (int)floor((double)(i - 1) * r);
                    const float a0 = atan2f(x.at(j0, chan + c), x.at(j0, c));
                    const float a1 = atan2f(x.at(j0 + 1, chan + c), x.at(j0 + 1, c));
                    step[j] = voc_wrap(a1 - a0 - adv) + adv;
                }
                sum = voc_wrap(sum + step[j]);
            }
        }
        float phase = pcen_scan_exclusive<VocMapPhase>(VocMapPhase{{sum}}, carry, s_map, g).m;

        // ---- pass 2: the run again from its exact start; output into the tile ----
#pragma unroll
        for (int j = 0; j < kVocMaxRun; ++j) {
            if (f_beg + j < f_end) {
                const int f = f_beg + j;
                const double ts = (double)(t0 + f) * r;
                const double fl = floor(ts);
                const int i0 = (int)fl;
                const float alpha = (float)(ts - fl);
                const float re0 = x.at(i0, c), im0 = x.at(i0, chan + c);
                const float re1 = x.at(i0 + 1, c), im1 = x.at(i0 + 1, chan + c);
                const float n0 = sqrtf(re0 * re0 + im0 * im0), n1 = sqrtf(re1 * re1 + im1 * im1);
                const float mag = alpha * n1 + (1.f - alpha) * n0;
                phase = voc_wrap(phase + step[j]);
                float sn, cs;
                sincosf(phase, &sn, &cs);
                out_tile[pcen_pad(f * chan2 + c)] = mag * cs;
                out_tile[pcen_pad(f * chan2 + chan + c)] = mag * sn;
            }
        }
        __syncthreads();   // every thread has read its carry and written its outputs
        if (g.active && g.seg == a.nseg - 1) carry[0][c] = phase;   // phase after the tile's last frame of channel c

        pcen_store_tile(out_tile, dst_row, a, gt, t0, len);
        __syncthreads();   // the tile buffers and the carries are reused by the next tile
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int iris_phase_vocoder(const void* table_dev, int n_src, int n_bins, int chan2, int max_out_frames, void* stream) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_phase_vocoder: n_src = %d is negative", n_src);
    if (n_bins < 2) return fail(IRIS_E_INVALID, "iris_phase_vocoder: n_bins = %d (hop = n_bins - 1 must be positive)", n_bins);
    if (chan2 <= 0 || (chan2 & 1))
        return fail(IRIS_E_INVALID, "iris_phase_vocoder: chan2 = %d must be positive and even (re block, im block)", chan2);
    if (n_src == 0) return IRIS_OK;
    if (!table_dev) return fail(IRIS_E_INVALID, "iris_phase_vocoder: table is NULL");
    if (max_out_frames <= 0) return fail(IRIS_E_INVALID, "iris_phase_vocoder: max_out_frames = %d must be positive", max_out_frames);
    if (chan2 / 2 > kPcenThreads)
        return fail(IRIS_E_UNSUPPORTED, "iris_phase_vocoder: %d channels > %d", chan2 / 2, kPcenThreads);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_phase_vocoder: n_src = %d > 65535", n_src);
    if ((size_t)max_out_frames * (size_t)chan2 > (size_t)INT_MAX)
        return fail(IRIS_E_UNSUPPORTED, "iris_phase_vocoder: a row of %d x %d floats exceeds 2^31 - 1", max_out_frames, chan2);
    k_phase_vocoder<<<dim3((unsigned)n_bins, (unsigned)n_src), kPcenThreads, 0, (hipStream_t)stream>>>(
        static_cast<const iris_voc_src*>(table_dev), chan2 / 2, max_out_frames);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
