// k_psds.h -- intersection-based detection counts behind the polyphonic sound detection score (Bilen et al., ICASSP 2020) of one
// batch at up to 64 thresholds, in two launches; the ratios, the curves and the area are host arithmetic (metrics.psds_metrics).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// Definition (include/iris_frontend.h has it in full): label activity y_true >= 0.5f, predicted activity at threshold h
// y_pred >= h (fp32, NaN inactive); events are maximal runs [s, e) of one (clip, class) row.  With I_k(d) the frames of a detection
// d in which label k is active: d PASSES if 100 I_c(d) >= dtc_pct len(d), else it is a false positive and a cross-trigger on every
// k != c with 100 I_k(d) >= cttc_pct len(d); a ground-truth event g is a true positive if 100 cov(g) >= gtc_pct len(g), cov(g)
// the frames of g inside passing detections of its class.
//   k_psds_prep:  one wave per (clip, class) row, 64 frames per step, frames 0 .. T (frame T is inactive and closes an open run).
//     __ballot gives the label mask; lane f writes P[f] = active label frames before f (the count before the step + the set bits
//     below the lane), so I_k([s, e)) = P_k[e] - P_k[s]; run starts m & ~prev and the frames after a run's end ~m & prev go to the
//     row's ground-truth list as in k_sed_extract.  The totals n_gt, gt_frames (and n_frames, once) are added to the last plane.
//   k_psds_score: one wave per (row, threshold).  The forward walk finds every detection's end at the lane of the frame after it;
//     that lane knows the start (the highest start bit below it, or the start carried from an earlier step), loads P_k[e] and
//     P_k[s] and decides.  Counters are wave sums of ballots: FP and n_det in every lane alike, CT[c][k] in lane k.  The mask
//     "frame lies in a passing detection" of a step is a ballot over the frames whose run ends inside the step; a run that crosses
//     a step boundary is the only one open there, so when it ends and passes, the words it crossed are rewritten by the wave (the
//     first word from a copy kept in a register, the others all ones).  Then an exclusive scan of the words' popcounts gives
//     C(x) = passing frames before x as cum[x / 64] + popcount(word[x / 64] below x % 64), and one lane per ground-truth event
//     takes cov = C(e) - C(s).  The sums of one (row, threshold) go to the int64 counts with vector atomics, zeros left out.
// Workspace, R = B * K rows, cap = T / 2 + 1 events per list, W = T / 64 + 1 words per (row, threshold):
//   pass words, uint64 [R][n_thr][W] | P, int32 [R][T + 1] | n_gt events [R] | start [R][cap] | end [R][cap] | cum [R][n_thr][W]
// ---------------------------------------------------------------------------

constexpr int kPsdsMaxK = 16;
constexpr int kPsdsMaxThr = 64;
constexpr int kPsdsMaxT = 1 << 20;
constexpr int kPsdsThreads = 256;
constexpr int kPsdsWaves = kPsdsThreads / 64;
constexpr int kPsdsMaxBlocks = 1 << 12;   // 16,384 waves fill the device about twice; further rows / items take the grid-stride loops

struct PsdsThresholds {
    float h[kPsdsMaxThr];
};

struct PsdsLayout {
    long long rows, cap, words, items;
    size_t off_prefix, off_n, off_start, off_end, off_cum, bytes;   // byte offsets behind the pass words
};

static PsdsLayout psds_layout(long long batch, long long n_time, long long n_classes, long long n_thr) {
    PsdsLayout l;
    l.rows = batch * n_classes;
    l.cap = n_time / 2 + 1;
    l.words = n_time / 64 + 1;
    l.items = l.rows * n_thr;
    l.off_prefix = (size_t)l.items * (size_t)l.words * sizeof(unsigned long long);
    l.off_n = l.off_prefix + (size_t)l.rows * (size_t)(n_time + 1) * sizeof(int);
    l.off_start = l.off_n + (size_t)l.rows * sizeof(int);
    l.off_end = l.off_start + (size_t)l.rows * (size_t)l.cap * sizeof(int);
    l.off_cum = l.off_end + (size_t)l.rows * (size_t)l.cap * sizeof(int);
    l.bytes = l.off_cum + (size_t)l.items * (size_t)l.words * sizeof(int);
    return l;
}

__global__ __launch_bounds__(kPsdsThreads) void k_psds_prep(const float* __restrict__ y_true, long long rows, long long batch, int T,
                                                            int K, int n_thr, int cap, int* __restrict__ prefix,
                                                            int* __restrict__ n_events, int* __restrict__ ev_start,
                                                            int* __restrict__ ev_end, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n_steps = T / 64 + 1;   // frames 0 .. T
    unsigned long long* const totals = counts + (size_t)n_thr * K * (K + 2);
    for (long long r = (long long)blockIdx.x * kPsdsWaves + wave; r < rows; r += (long long)gridDim.x * kPsdsWaves) {
        const long long b = r / K;
        const int k = (int)(r - b * K);
        const float* const yt = y_true + (size_t)b * T * K + k;
        int* const P = prefix + (size_t)r * (T + 1);
        int* const st = ev_start + (size_t)r * cap;
        int* const en = ev_end + (size_t)r * cap;
        int n_ev = 0, n_act = 0;   // (wave-uniform)
        unsigned carry = 0u;
        float t_next = lane < T ? yt[(size_t)lane * K] : 0.f;
        for (int c = 0; c < n_steps; ++c) {
            const int f = c * 64 + lane;
            const float t = t_next;
            if (f + 64 < T) t_next = yt[(size_t)(f + 64) * K];
            const unsigned long long m = __ballot(f < T && t >= 0.5f);   // (NaN: false)
            const unsigned long long prev = (m << 1) | carry;
            const unsigned long long starts = m & ~prev, ends = ~m & prev;
            if (f <= T) P[f] = n_act + __popcll(m & below);
            if ((starts >> lane) & 1ull) st[n_ev + __popcll(starts & below)] = f;
            if ((ends >> lane) & 1ull) en[n_ev - (int)carry + __popcll(ends & below)] = f;   // (= last frame + 1)
            n_ev += __popcll(starts);
            n_act += __popcll(m);
            carry = (unsigned)(m >> 63);
        }
        if (lane == 0) {
            n_events[r] = n_ev;
            if (n_ev) atomicAdd(&totals[(size_t)k * (K + 2)], (unsigned long long)n_ev);
            if (n_act) atomicAdd(&totals[(size_t)k * (K + 2) + 1], (unsigned long long)n_act);
            if (r == 0) atomicAdd(&totals[K > 1 ? K : 2], (unsigned long long)(batch * T));   // (K = 1: column 1 is gt_frames)
        }
    }
}

__global__ __launch_bounds__(kPsdsThreads) void k_psds_score(const float* __restrict__ y_pred, long long items, int T, int K,
                                                             PsdsThresholds thr, int n_thr, int dtc_pct, int gtc_pct, int cttc_pct,
                                                             int cap, const int* __restrict__ prefix,
                                                             const int* __restrict__ n_events, const int* __restrict__ ev_start,
                                                             const int* __restrict__ ev_end, unsigned long long* pass_words,
                                                             int* cum_words, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    float h_lane = 0.f;   // lane j: threshold j (static indices: the argument stays in scalar registers)
#pragma unroll
    for (int j = 0; j < kPsdsMaxThr; ++j) h_lane = lane == j ? thr.h[j] : h_lane;
    const int n_steps = T / 64 + 1;   // frames 0 .. T: the frame after the row closes an open run
    for (long long i = (long long)blockIdx.x * kPsdsWaves + wave; i < items; i += (long long)gridDim.x * kPsdsWaves) {
        const long long r = i / n_thr;
        const int j = __builtin_amdgcn_readfirstlane((int)(i - r * n_thr));
        const long long b = r / K;
        const int c = (int)(r - b * K);
        const float h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h_lane), j));
        const float* const yp = y_pred + (size_t)b * T * K + c;
        const int* const P0 = prefix + (size_t)b * K * (T + 1);   // class k of this clip: P0 + k * (T + 1)
        const int* const Pc = P0 + (size_t)c * (T + 1);
        unsigned long long* const pw = pass_words + (size_t)i * n_steps;
        int* const cw = cum_words + (size_t)i * n_steps;
        int n_det = 0, n_fp = 0;       // wave-uniform
        int ct_mine = 0;               // lane k: cross-triggers on class k
        unsigned carry = 0u;           // the previous frame was active
        int open_start = 0;            // the start of the run open at the step boundary ...
        unsigned long long open_word = 0ull;   // ... and the pass bits known of the word it starts in
        float p_next = lane < T ? yp[(size_t)lane * K] : 0.f;
        for (int s = 0; s < n_steps; ++s) {
            const int f = s * 64 + lane;
            const float p = p_next;
            if (f + 64 < T) p_next = yp[(size_t)(f + 64) * K];
            const unsigned long long m = __ballot(f < T && p >= h);   // (NaN: false)
            const unsigned long long prev = (m << 1) | carry;
            const unsigned long long starts = m & ~prev, ends = ~m & prev;
            unsigned long long pass_ends = 0ull;   // bit e: the detection that ends in front of lane e passes
            if (ends) {
                const bool is_end = (ends >> lane) & 1ull;
                const unsigned long long sb = starts & below;
                const int d_start = sb ? s * 64 + 63 - __clzll((long long)sb) : open_start;
                const long long len = f - d_start;
                bool passes = false;
                if (is_end) passes = 100ll * (long long)(Pc[f] - Pc[d_start]) >= (long long)dtc_pct * len;
                pass_ends = __ballot(is_end && passes);
                const unsigned long long failed = ends & ~pass_ends;
                n_det += __popcll(ends);
                n_fp += __popcll(failed);
                if (failed && cttc_pct > 0) {
                    for (int k = 0; k < K; ++k) {
                        if (k == c) continue;
                        const int* const Pk = P0 + (size_t)k * (T + 1);
                        bool ct = false;
                        if ((failed >> lane) & 1ull) ct = 100ll * (long long)(Pk[f] - Pk[d_start]) >= (long long)cttc_pct * len;
                        const int n = __popcll(__ballot(ct));
                        if (lane == k) ct_mine += n;
                    }
                }
                // a passing detection that began in an earlier step: the words [open_start / 64, s) it crossed
                if (carry && (pass_ends & ends & (0ull - ends))) {   // (the lowest end bit is the carried run's)
                    const int w0 = open_start >> 6;
                    for (int w = w0 + lane; w < s; w += 64)
                        pw[w] = w == w0 ? (open_word | (~0ull << (open_start & 63))) : ~0ull;
                }
            }
            // frames whose run ends inside this step
            const unsigned long long above = ends & ~below & ~(1ull << lane);
            const bool in_pass = ((m >> lane) & 1ull) && above && ((pass_ends >> (__ffsll((long long)above) - 1)) & 1ull);
            const unsigned long long known = __ballot(in_pass);
            if (lane == 0) pw[s] = known;
            if (m >> 63) {   // the run of frame 63 stays open: where it began
                const unsigned long long zeros = ~m;
                if (zeros) {
                    open_start = s * 64 + 64 - __clzll((long long)zeros);
                    open_word = known;
                } else if (!carry) {
                    open_start = s * 64;
                    open_word = 0ull;
                }
            }
            carry = (unsigned)(m >> 63);
        }
        __threadfence_block();   // the words above are read by other lanes below
        int running = 0;
        for (int base = 0; base < n_steps; base += 64) {
            const int w = base + lane;
            const int cnt = w < n_steps ? __popcll(pw[w]) : 0;
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (w < n_steps) cw[w] = running + incl - cnt;
            running += __shfl(incl, 63, 64);
        }
        __threadfence_block();
        const int n_gt = n_events[r];
        const int* const gs = ev_start + (size_t)r * cap;
        const int* const ge = ev_end + (size_t)r * cap;
        int n_tp = 0;
        for (int base = 0; base < n_gt; base += 64) {
            const int e = base + lane;
            bool tp = false;
            if (e < n_gt) {
                const int a = gs[e], z = ge[e];
                const int ca = cw[a >> 6] + __popcll(pw[a >> 6] & ((1ull << (a & 63)) - 1ull));
                const int cz = cw[z >> 6] + __popcll(pw[z >> 6] & ((1ull << (z & 63)) - 1ull));
                tp = 100ll * (long long)(cz - ca) >= (long long)gtc_pct * (long long)(z - a);
            }
            n_tp += __popcll(__ballot(tp));
        }
        unsigned long long* const row = counts + ((size_t)j * K + c) * (K + 2);
        if (lane == c) {
            if (n_tp) atomicAdd(&row[c], (unsigned long long)n_tp);
            if (n_fp) atomicAdd(&row[K], (unsigned long long)n_fp);
            if (n_det) atomicAdd(&row[K + 1], (unsigned long long)n_det);
        } else if (lane < K && ct_mine) {
            atomicAdd(&row[lane], (unsigned long long)ct_mine);
        }
    }
}

static int psds_check_shape(const char* who, int batch, int n_time, int n_classes, int n_thr) {
    if (batch < 1 || n_time < 1 || n_classes < 1 || n_thr < 1)
        return fail(IRIS_E_INVALID, "%s: batch %d, T %d, K %d, %d thresholds (all >= 1)", who, batch, n_time, n_classes, n_thr);
    if (n_classes > kPsdsMaxK) return fail(IRIS_E_UNSUPPORTED, "%s: K %d (<= %d)", who, n_classes, kPsdsMaxK);
    if (n_thr > kPsdsMaxThr) return fail(IRIS_E_UNSUPPORTED, "%s: %d thresholds (<= %d)", who, n_thr, kPsdsMaxThr);
    if (n_time > kPsdsMaxT) return fail(IRIS_E_UNSUPPORTED, "%s: T %d (<= 2^20)", who, n_time);
    if ((long long)batch * (long long)n_time > 2147483647LL)
        return fail(IRIS_E_UNSUPPORTED, "%s: batch %d x T %d frames (<= 2^31 - 1)", who, batch, n_time);
    return IRIS_OK;
}

extern "C" long long iris_psds_workspace_bytes(int batch, int n_time, int n_classes, int n_thr) {
    if (psds_check_shape("iris_psds_workspace_bytes", batch, n_time, n_classes, n_thr) != IRIS_OK) return 0;
    return (long long)psds_layout(batch, n_time, n_classes, n_thr).bytes;
}

extern "C" int iris_psds_counts(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes,
                                const float* thresholds, int n_thr, int dtc_pct, int gtc_pct, int cttc_pct, void* workspace,
                                size_t workspace_bytes, long long* counts, void* stream) {
    if (!y_true || !y_pred || !thresholds || !workspace || !counts)
        return fail(IRIS_E_INVALID, "iris_psds_counts: NULL y_true / y_pred / thresholds / workspace / counts");
    const int shape = psds_check_shape("iris_psds_counts", batch, n_time, n_classes, n_thr);
    if (shape != IRIS_OK) return shape;
    if (dtc_pct < 1 || dtc_pct > 100 || gtc_pct < 1 || gtc_pct > 100 || cttc_pct < 0 || cttc_pct > 100)
        return fail(IRIS_E_INVALID, "iris_psds_counts: dtc_pct %d, gtc_pct %d (1 .. 100), cttc_pct %d (1 .. 100, or 0 for none)", dtc_pct,
                    gtc_pct, cttc_pct);
    PsdsThresholds thr;
    for (int j = 0; j < kPsdsMaxThr; ++j) thr.h[j] = 0.f;
    for (int j = 0; j < n_thr; ++j) {
        const float h = thresholds[j];
        if (!std::isfinite(h) || (j > 0 && !(h > thresholds[j - 1])))
            return fail(IRIS_E_INVALID, "iris_psds_counts: thresholds must be finite and strictly increasing (entry %d)", j);
        thr.h[j] = h;
    }
    const PsdsLayout l = psds_layout(batch, n_time, n_classes, n_thr);
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0u) return fail(IRIS_E_INVALID, "iris_psds_counts: workspace must be 8-byte aligned");
    if (workspace_bytes < l.bytes)
        return fail(IRIS_E_INVALID, "iris_psds_counts: workspace of %zu bytes, %zu needed (iris_psds_workspace_bytes)", workspace_bytes, l.bytes);
    char* const ws = static_cast<char*>(workspace);
    unsigned long long* const pass_words = reinterpret_cast<unsigned long long*>(ws);
    int* const prefix = reinterpret_cast<int*>(ws + l.off_prefix);
    int* const n_events = reinterpret_cast<int*>(ws + l.off_n);
    int* const ev_start = reinterpret_cast<int*>(ws + l.off_start);
    int* const ev_end = reinterpret_cast<int*>(ws + l.off_end);
    int* const cum_words = reinterpret_cast<int*>(ws + l.off_cum);
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(counts);
    const hipStream_t s = (hipStream_t)stream;
    const int g1 = (int)std::min<long long>((l.rows + kPsdsWaves - 1) / kPsdsWaves, kPsdsMaxBlocks);
    k_psds_prep<<<g1, kPsdsThreads, 0, s>>>(y_true, l.rows, batch, n_time, n_classes, n_thr, (int)l.cap, prefix, n_events, ev_start,
                                            ev_end, out);
    HIP_TRY(hipGetLastError());
    const int g2 = (int)std::min<long long>((l.items + kPsdsWaves - 1) / kPsdsWaves, kPsdsMaxBlocks);
    k_psds_score<<<g2, kPsdsThreads, 0, s>>>(y_pred, l.items, n_time, n_classes, thr, n_thr, dtc_pct, gtc_pct, cttc_pct, (int)l.cap,
                                             prefix, n_events, ev_start, ev_end, pass_words, cum_words, out);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
