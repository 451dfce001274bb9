// k_sedeval.h -- segment- and event-based detection counts (Mesaros, Heittola & Virtanen 2016, the measures sed_eval reports) of one
// batch at up to 16 thresholds, in two launches; ratios are host arithmetic on the counts (metrics.sed_metrics).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// Definition (include/iris_frontend.h has it in full): label activity y_true >= 0.5f, predicted activity at threshold h
// y_pred >= h (fp32, NaN inactive).  The thresholds increase strictly, so the thresholds a score passes are a PREFIX h_0 .. h_{c-1}:
// a frame is summed up by its count c, and a (row, segment) by the largest count of its frames.
//   k_sed_extract: one wave per (clip, class) row, 64 frames per step.  __ballot gives the 64-bit activity mask of the labels
//     and of every threshold; run starts are m & ~prev and the frames after a run's end ~m & prev with prev = (m << 1) | carry,
//     the carry being the previous step's bit 63.  The walk goes one frame past the row (frame T is inactive), so a run open at
//     the end closes at T - 1.  A start's slot in its list is the count before the step + the set bits below the lane; the list
//     counters live one per lane (lane i: mask i) and are read with readlane.  Frame f lies in segment (f * hop) / seg_samples;
//     the lane of a segment's last frame writes (label active, largest count) of the segment as one 16-bit word, from the ballot
//     bits between the segment's first lane of the step and itself, joined with what the segment gathered in earlier steps.
//   k_sed_score: the first `ev_blocks` workgroups match - one lane per (row, threshold), reference events in time order, each
//     taking the earliest free prediction within both collars (a taken prediction is marked by complementing its start in the
//     workspace); the others take one (clip, segment) per lane and combine its classes into tp / fp / fn and S / D / I.
//     Sums go to 64-bit LDS counters and the non-zero ones to the int64 counts, with vector atomics.
// Workspace, int32 unless noted, R = B * K rows, M = n_thr + 1 lists per row, cap = T / 2 + 1 >= ceil(T / 2) events per list:
//   n_events [R][M] | start [R][M][cap] | end + 1 [R][M][cap] | segment words, uint16 [R][n_seg]
// ---------------------------------------------------------------------------

constexpr int kSedMaxK = 16;
constexpr int kSedMaxThr = 16;
constexpr int kSedMaxT = 1 << 20;
constexpr int kSedThreads = 256;
constexpr int kSedWaves = kSedThreads / 64;
constexpr int kSedMaxBlocks = 1 << 16;
constexpr int kSedFields = 6;

struct SedThresholds {
    float h[kSedMaxThr];
};

struct SedLayout {
    long long rows, n_seg, cap, lists;
    size_t off_start, off_end, off_seg, bytes;   // byte offsets behind n_events
};

static SedLayout sed_layout(long long batch, long long n_time, long long n_classes, long long n_thr, long long hop, long long seg_samples) {
    SedLayout l;
    l.rows = batch * n_classes;
    l.n_seg = ((n_time - 1) * hop) / seg_samples + 1;
    l.cap = n_time / 2 + 1;
    l.lists = l.rows * (n_thr + 1);
    l.off_start = (size_t)l.lists * sizeof(int);
    l.off_end = l.off_start + (size_t)l.lists * (size_t)l.cap * sizeof(int);
    l.off_seg = l.off_end + (size_t)l.lists * (size_t)l.cap * sizeof(int);
    l.bytes = l.off_seg + (size_t)l.rows * (size_t)l.n_seg * sizeof(unsigned short);
    return l;
}

__global__ __launch_bounds__(kSedThreads) void k_sed_extract(const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                                             long long rows, int T, int K, SedThresholds thr, int n_thr, int hop,
                                                             int seg_samples, int n_seg, int cap, int* __restrict__ n_events,
                                                             int* __restrict__ ev_start, int* __restrict__ ev_end,
                                                             unsigned short* __restrict__ seg_words) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lists = n_thr + 1;
    const unsigned long long below = (1ull << lane) - 1ull;
    float h_lane = 0.f;   // lane j: threshold j (static indices: the argument stays in scalar registers)
#pragma unroll
    for (int j = 0; j < kSedMaxThr; ++j) h_lane = lane == j ? thr.h[j] : h_lane;
    const int n_steps = T / 64 + 1;   // frames 0 .. T: the frame after the row closes an open run
    for (long long r = (long long)blockIdx.x * kSedWaves + wave; r < rows; r += (long long)gridDim.x * kSedWaves) {
        const long long b = r / K;
        const int k = (int)(r - b * K);
        const float* const yt = y_true + (size_t)b * T * K + k;
        const float* const yp = y_pred + (size_t)b * T * K + k;
        int* const st = ev_start + (size_t)r * lists * cap;
        int* const en = ev_end + (size_t)r * lists * cap;
        unsigned short* const sg = seg_words + (size_t)r * n_seg;
        int n_mine = 0;            // lane i: events of list i so far
        unsigned carry = 0u;       // bit i: list i was active in the previous frame
        bool open_ref = false;     // the segment still open at the previous step's end: label active, largest count
        int open_cnt = 0;
        long long prev_seg = -1;   // ... and its index
        float t_next = lane < T ? yt[(size_t)lane * K] : 0.f, p_next = lane < T ? yp[(size_t)lane * K] : 0.f;
        for (int c = 0; c < n_steps; ++c) {
            const int f = c * 64 + lane;
            const bool valid = f < T;
            const float t = t_next, p = p_next;
            if (f + 64 < T) {
                t_next = yt[(size_t)(f + 64) * K];
                p_next = yp[(size_t)(f + 64) * K];
            }
            // this lane's segment, the lanes [s, lane] of it inside the step, and whether it began in an earlier step
            const long long seg = valid ? ((long long)f * hop) / seg_samples : -2;
            const long long seg_after = ((long long)(f + 1) * hop) / seg_samples;
            long long seg_before = __shfl_up(seg, 1, 64);
            const bool first = valid && (lane == 0 || seg != seg_before);
            const bool last = valid && (f == T - 1 || seg_after != seg);
            const unsigned long long firsts = __ballot(first);
            const int s = valid ? 63 - __clzll((long long)(firsts & (below | (1ull << lane)))) : 0;
            const unsigned long long seg_mask = valid ? (((2ull << lane) - 1ull) & ~((1ull << s) - 1ull)) : 0ull;
            const bool joins0 = __shfl(seg, 0, 64) == prev_seg;   // the step's first segment continues the open one
            const bool joins = joins0 && s == 0;
            const int s_top = firsts ? 63 - __clzll((long long)firsts) : 0;
            const unsigned long long top_mask = ~((1ull << s_top) - 1ull);
            const bool top_joins = joins0 && s_top == 0;

            auto events = [&](int list, unsigned long long m) {
                const unsigned cbit = (carry >> list) & 1u;
                const unsigned long long prev = (m << 1) | cbit;
                const unsigned long long starts = m & ~prev, ends = ~m & prev;
                const int base = __builtin_amdgcn_readlane(n_mine, list);
                if ((starts >> lane) & 1ull) st[(size_t)list * cap + base + __popcll(starts & below)] = f;
                if ((ends >> lane) & 1ull) en[(size_t)list * cap + base - (int)cbit + __popcll(ends & below)] = f;   // (= last frame + 1)
                if (lane == list) n_mine += __popcll(starts);
                carry = (carry & ~(1u << list)) | ((unsigned)(m >> 63) << list);
            };

            const unsigned long long m_ref = __ballot(valid && t >= 0.5f);   // (NaN: false)
            const bool seg_ref = (m_ref & seg_mask) != 0ull || (joins && open_ref);
            const bool top_ref = (m_ref & top_mask) != 0ull || (top_joins && open_ref);
            events(0, m_ref);
            int cnt = 0, top_cnt = 0;
            for (int j = 0; j < n_thr; ++j) {
                const float h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h_lane), j));
                const unsigned long long m = __ballot(valid && p >= h);
                cnt += (m & seg_mask) != 0ull ? 1 : 0;
                top_cnt += (m & top_mask) != 0ull ? 1 : 0;
                events(1 + j, m);
            }
            if (joins) cnt = max(cnt, open_cnt);
            if (last) sg[seg] = (unsigned short)((seg_ref ? 1 : 0) | (cnt << 8));
            if (firsts) {
                open_ref = top_ref;
                open_cnt = top_joins ? max(top_cnt, open_cnt) : top_cnt;
                prev_seg = __shfl(seg, 63, 64);
            }
        }
        if (lane < lists) n_events[(size_t)r * lists + lane] = n_mine;
    }
}

__global__ __launch_bounds__(kSedThreads) void k_sed_score(long long rows, long long batch, int K, int n_thr, int hop,
                                                           int collar_samples, int offset_pct, int n_seg, int cap, int ev_blocks,
                                                           const int* __restrict__ n_events, int* ev_start,
                                                           const int* __restrict__ ev_end, const unsigned short* __restrict__ seg_words,
                                                           unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long acc[kSedMaxThr * (kSedMaxK + 1) * kSedFields];   // (64-bit: no bound on a workgroup's share needed)
    const int n_acc = n_thr * (K + 1) * kSedFields;
    for (int i = threadIdx.x; i < n_acc; i += blockDim.x) acc[i] = 0ull;
    __syncthreads();
    const int lists = n_thr + 1;
    if ((int)blockIdx.x < ev_blocks) {
        const long long items = rows * n_thr;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long long)ev_blocks * blockDim.x) {
            const long long r = i / n_thr;
            const int j = (int)(i - r * n_thr), k = (int)(r % K);
            const int n_ref = n_events[(size_t)r * lists], n_pred = n_events[(size_t)r * lists + 1 + j];
            const int* const rs = ev_start + (size_t)r * lists * cap;
            const int* const re = ev_end + (size_t)r * lists * cap;
            int* const ps = ev_start + ((size_t)r * lists + 1 + j) * cap;   // this lane's alone: a taken start is stored as ~start
            const int* const pe = ev_end + ((size_t)r * lists + 1 + j) * cap;
            int tp = 0, lo = 0;
            for (int e = 0; e < n_ref && lo < n_pred; ++e) {
                const long long on_r = (long long)rs[e] * hop, off_r = (long long)re[e] * hop;
                const long long tol = max(100ll * collar_samples, (long long)offset_pct * (off_r - on_r));
                // onsets increase along both lists: what lies before this window, or is taken, is out for every later event too
                while (lo < n_pred) {
                    const int v = ps[lo];
                    if (v >= 0 && (long long)v * hop >= on_r - collar_samples) break;
                    ++lo;
                }
                for (int q = lo; q < n_pred; ++q) {
                    const int v = ps[q];
                    const long long on_p = (long long)(v < 0 ? ~v : v) * hop;
                    if (on_p > on_r + collar_samples) break;
                    if (v < 0) continue;
                    const long long d = (long long)pe[q] * hop - off_r;
                    if (100ll * (d < 0 ? -d : d) <= tol) {
                        ps[q] = ~v;
                        ++tp;
                        break;
                    }
                }
            }
            unsigned long long* const a = acc + (j * (K + 1) + k) * kSedFields;
            if (tp) atomicAdd(&a[3], (unsigned long long)tp);
            if (n_pred - tp) atomicAdd(&a[4], (unsigned long long)(n_pred - tp));
            if (n_ref - tp) atomicAdd(&a[5], (unsigned long long)(n_ref - tp));
        }
    } else {
        const long long items = batch * n_seg;
        const long long stride = (long long)(gridDim.x - ev_blocks) * blockDim.x;
        for (long long i = (long long)(blockIdx.x - ev_blocks) * blockDim.x + threadIdx.x; i < items; i += stride) {
            const long long b = i / n_seg;
            const int s = (int)(i - b * n_seg);
            const unsigned short* const w = seg_words + (size_t)b * K * n_seg + s;
            for (int j = 0; j < n_thr; ++j) {
                int n_fn = 0, n_fp = 0;
                for (int k = 0; k < K; ++k) {
                    const unsigned v = w[(size_t)k * n_seg];
                    const bool ref = (v & 1u) != 0u, pred = (int)(v >> 8) > j;
                    if (ref || pred) atomicAdd(&acc[(j * (K + 1) + k) * kSedFields + (ref && pred ? 0 : pred ? 1 : 2)], 1ull);
                    n_fn += ref && !pred ? 1 : 0;
                    n_fp += pred && !ref ? 1 : 0;
                }
                unsigned long long* const a = acc + (j * (K + 1) + K) * kSedFields;
                const int sub = min(n_fn, n_fp);
                if (sub) atomicAdd(&a[0], (unsigned long long)sub);
                if (n_fn > n_fp) atomicAdd(&a[1], (unsigned long long)(n_fn - n_fp));
                if (n_fp > n_fn) atomicAdd(&a[2], (unsigned long long)(n_fp - n_fn));
                atomicAdd(&a[3], 1ull);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_acc; i += blockDim.x) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&counts[i], v);
    }
}

static int sed_check_shape(const char* who, int batch, int n_time, int n_classes, int n_thr, int hop, int seg_samples) {
    if (batch < 1 || n_time < 1 || n_classes < 1) return fail(IRIS_E_INVALID, "%s: batch %d, T %d, K %d", who, batch, n_time, n_classes);
    if (n_thr < 1 || n_thr > kSedMaxThr) return fail(IRIS_E_INVALID, "%s: %d thresholds (1 .. %d)", who, n_thr, kSedMaxThr);
    if (hop < 1 || seg_samples < hop) return fail(IRIS_E_INVALID, "%s: hop %d (>= 1), seg_samples %d (>= hop)", who, hop, seg_samples);
    if (n_classes > kSedMaxK) return fail(IRIS_E_UNSUPPORTED, "%s: K %d (<= %d)", who, n_classes, kSedMaxK);
    if (n_time > kSedMaxT) return fail(IRIS_E_UNSUPPORTED, "%s: T %d (<= 2^20)", who, n_time);
    if ((long long)batch * (long long)n_time > 2147483647LL)
        return fail(IRIS_E_UNSUPPORTED, "%s: batch %d x T %d frames (<= 2^31 - 1)", who, batch, n_time);
    return IRIS_OK;
}

extern "C" long long iris_sed_workspace_bytes(int batch, int n_time, int n_classes, int n_thr, int hop, int seg_samples) {
    if (sed_check_shape("iris_sed_workspace_bytes", batch, n_time, n_classes, n_thr, hop, seg_samples) != IRIS_OK) return 0;
    return (long long)sed_layout(batch, n_time, n_classes, n_thr, hop, seg_samples).bytes;
}

extern "C" int iris_sed_counts(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes,
                               const float* thresholds, int n_thr, int hop, int seg_samples, int collar_samples, int offset_pct,
                               void* workspace, size_t workspace_bytes, long long* counts, void* stream) {
    if (!y_true || !y_pred || !thresholds || !workspace || !counts)
        return fail(IRIS_E_INVALID, "iris_sed_counts: NULL y_true / y_pred / thresholds / workspace / counts");
    const int shape = sed_check_shape("iris_sed_counts", batch, n_time, n_classes, n_thr, hop, seg_samples);
    if (shape != IRIS_OK) return shape;
    if (collar_samples < 0 || offset_pct < 0 || offset_pct > 100)
        return fail(IRIS_E_INVALID, "iris_sed_counts: collar_samples %d (>= 0), offset_pct %d (0 .. 100)", collar_samples, offset_pct);
    SedThresholds thr;
    for (int j = 0; j < kSedMaxThr; ++j) thr.h[j] = 0.f;
    for (int j = 0; j < n_thr; ++j) {
        const float h = thresholds[j];
        if (!std::isfinite(h) || (j > 0 && !(h > thresholds[j - 1])))
            return fail(IRIS_E_INVALID, "iris_sed_counts: thresholds must be finite and strictly increasing (entry %d)", j);
        thr.h[j] = h;
    }
    const SedLayout l = sed_layout(batch, n_time, n_classes, n_thr, hop, seg_samples);
    if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0u) return fail(IRIS_E_INVALID, "iris_sed_counts: workspace must be 4-byte aligned");
    if (workspace_bytes < l.bytes)
        return fail(IRIS_E_INVALID, "iris_sed_counts: workspace of %zu bytes, %zu needed (iris_sed_workspace_bytes)", workspace_bytes, l.bytes);
    char* const ws = static_cast<char*>(workspace);
    int* const n_events = reinterpret_cast<int*>(ws);
    int* const ev_start = reinterpret_cast<int*>(ws + l.off_start);
    int* const ev_end = reinterpret_cast<int*>(ws + l.off_end);
    unsigned short* const seg_words = reinterpret_cast<unsigned short*>(ws + l.off_seg);
    const hipStream_t s = (hipStream_t)stream;
    const int g1 = (int)std::min<long long>((l.rows + kSedWaves - 1) / kSedWaves, kSedMaxBlocks);
    k_sed_extract<<<g1, kSedThreads, 0, s>>>(y_true, y_pred, l.rows, n_time, n_classes, thr, n_thr, hop, seg_samples, (int)l.n_seg,
                                             (int)l.cap, n_events, ev_start, ev_end, seg_words);
    HIP_TRY(hipGetLastError());
    const int ev_blocks = (int)std::min<long long>((l.rows * n_thr + kSedThreads - 1) / kSedThreads, kSedMaxBlocks);
    const int seg_blocks = (int)std::min<long long>(((long long)batch * l.n_seg + kSedThreads - 1) / kSedThreads, kSedMaxBlocks);
    k_sed_score<<<ev_blocks + seg_blocks, kSedThreads, 0, s>>>(l.rows, batch, n_classes, n_thr, hop, collar_samples, offset_pct,
                                                               (int)l.n_seg, (int)l.cap, ev_blocks, n_events, ev_start, ev_end,
                                                               seg_words, reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
