// k_detect.h -- window predictions of F files -> event lists (metrics.py:56-81 + :111-137) in two launches, no host sync.
// Part of the single translation unit iris_frontend.hip (after decode_core.h).
#pragma once
// ---------------------------------------------------------------------------
// The arithmetic is decode_core.h's steps 1-4, called and not restated: dec_overlap_avg (1), dec_smooth with dec_is_on /
// dec_is_nan (2), dec_dilate (3), dec_run_starts / dec_run_ends (4), pads from dec_pad.  Here is how one setting's work is laid
// out over two launches, and the checks of the arguments that k_tune.h's entry point shares (dec_check_files).
// Launch 1 (k_decode_bits): one workgroup per tile of kDecTile frames of one file, every class in turn.  The tile's p (with a
// halo of 64 MW + avg.l / avg.r frames) goes to LDS; a is computed per frame from LDS and turned by __ballot into two bit words per
// 64 frames (a >= thr, a is NaN) over the tile plus MW words each side; d of a frame is "any on-bit and no NaN-bit in the
// window", a masked OR over <= 2 MW + 1 words.  d goes out as bit words, file by file, class by class.
// Launch 2 (k_decode_runs): one wave per (file, class) walks its bit words 64 at a time: run starts / ends are word
// operations, a wave prefix sum of their popcounts gives each event its slot, so the i-th start and the i-th end land in
// pair i.  Plain stores only, no atomics: the output is bitwise reproducible.
// Offsets (tiles, bit words, event pairs) are prefix sums over frame_len, recomputed on the device by each block.
// ---------------------------------------------------------------------------

constexpr int kDecTile = 512;                          // output frames per workgroup (a multiple of 64)
constexpr int kDecThreads = 256;
constexpr int kDecMaxK = 16;
constexpr int kDecMaxAvg = 127;                        // avg pool width: al, ar <= 63
constexpr int kDecMaxMax = 256;                        // max pool width: ml, mr <= 128, so MW <= 2 halo words
constexpr int kDecMaxMW = 2;
constexpr int kDecMaxWords = kDecTile / 64 + 2 * kDecMaxMW;
constexpr int kDecMaxP = kDecTile + 128 * kDecMaxMW + (kDecMaxAvg - 1);

struct DecLds {
    float p[kDecMaxP];
    uint64_t on[kDecMaxWords];
    uint64_t nan[kDecMaxWords];
    int scan_t[kDecThreads];
    int scan_w[kDecThreads];
    int file, tile, wbase;
};

__global__ __launch_bounds__(kDecThreads) void k_decode_bits(const float* __restrict__ preds, const int* __restrict__ win_off,
                                                             const int* __restrict__ frame_len, int F, int n_frame, int hop,
                                                             int n_out, int up, int K, DecPad avg, DecPad mx, int mw, float thr,
                                                             uint64_t* __restrict__ bits) {
    __shared__ DecLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwv = kDecThreads / 64;
    const int bid = blockIdx.x;
    // ---- which file / tile: block-wide prefix sums of tiles and bit words over frame_len, 256 files at a time
    if (tid == 0) L.file = -1;
    int base_t = 0, base_w = 0;
    for (int c0 = 0; c0 < F; c0 += kDecThreads) {
        const int g = c0 + tid;
        const int tl = g < F ? frame_len[g] : 0;
        const int nt = (tl + kDecTile - 1) / kDecTile, nw = dec_words(tl);
        L.scan_t[tid] = nt;
        L.scan_w[tid] = nw;
        __syncthreads();
        for (int o = 1; o < kDecThreads; o <<= 1) {   // Hillis-Steele inclusive scan
            const int xt = tid >= o ? L.scan_t[tid - o] : 0, xw = tid >= o ? L.scan_w[tid - o] : 0;
            __syncthreads();
            L.scan_t[tid] += xt;
            L.scan_w[tid] += xw;
            __syncthreads();
        }
        const int ex_t = base_t + L.scan_t[tid] - nt;
        if (g < F && bid >= ex_t && bid < ex_t + nt) {   // exactly one thread of the grid's files owns this block
            L.file = g;
            L.tile = bid - ex_t;
            L.wbase = (base_w + L.scan_w[tid] - nw) * K;
        }
        base_t += L.scan_t[kDecThreads - 1];
        base_w += L.scan_w[kDecThreads - 1];
        __syncthreads();
        if (L.file >= 0) break;   // (uniform: read after the barrier)
    }
    if (L.file < 0) return;
    const int f = L.file, T = frame_len[f], nw = dec_words(T);
    const int t0 = L.tile * kDecTile;
    const int w0 = win_off[f], W = win_off[f + 1] - w0;
    const int bbase = t0 - 64 * mw;        // frame of bit 0 of on / nan
    const int pbase = bbase - avg.l;       // frame of p[0]
    const int np = kDecTile + 128 * mw + avg.l + avg.r;
    const int nwb = kDecTile / 64 + 2 * mw;
    uint64_t* out = bits + L.wbase;
    for (int k = 0; k < K; ++k) {
        // 1. overlap-add average over the tile and its halo
        for (int i = tid; i < np; i += kDecThreads) {
            const int v = pbase + i;
            L.p[i] = v >= 0 && v < T ? dec_overlap_avg(preds, w0, W, n_frame, hop, n_out, up, K, v, k) : 0.f;
        }
        __syncthreads();
        // 2. average smoothing -> bit words (a >= thr, a NaN); frames outside [0, T) are neither
        for (int j = wv; j < nwb; j += nwv) {
            const int u = bbase + 64 * j + lane;
            bool on = false, isn = false;
            if (u >= 0 && u < T) {
                const float a = dec_smooth(L.p, -pbase, u, avg, T);
                on = dec_is_on(a, thr);
                isn = dec_is_nan(a);
            }
            const uint64_t b_on = __ballot(on), b_nan = __ballot(isn);
            if (lane == 0) {
                L.on[j] = b_on;
                L.nan[j] = b_nan;
            }
        }
        __syncthreads();
        // 3. max smoothing + threshold as a bit dilation; frames >= T stay 0 (launch 2 relies on it)
        for (int jj = wv; jj < kDecTile / 64; jj += nwv) {
            const int t = t0 + 64 * jj + lane;
            const int i = 64 * mw + 64 * jj + lane;   // the frame's bit in on / nan
            const uint64_t b = __ballot(t < T && dec_dilate(L.on, L.nan, i - mx.l, i + mx.r));
            const int word = (t0 >> 6) + jj;
            if (lane == 0 && word < nw) out[(size_t)k * nw + word] = b;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_decode_runs(const int* __restrict__ frame_len, int F, int K,
                                                     const uint64_t* __restrict__ bits, int* __restrict__ ev,
                                                     int* __restrict__ n_ev) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // (file, class), uniform per wave
    if (q >= F * K) return;
    const int f = q / K, k = q - f * K;
    int sw = 0, sp = 0;   // bit words and event pairs of the files before f
    for (int g = lane; g < f; g += 64) {
        const int tl = frame_len[g];
        sw += dec_words(tl);
        sp += dec_pairs(tl);
    }
    sw = dec_wave_sum(sw);
    sp = dec_wave_sum(sp);
    const int T = frame_len[f], nw = dec_words(T);
    const uint64_t* w = bits + (size_t)sw * K + (size_t)k * nw;
    int* e = ev + 2 * ((size_t)sp * K + (size_t)k * dec_pairs(T));
    int base_s = 0, base_e = 0;
    for (int c0 = 0; c0 < nw; c0 += 64) {
        const int j = c0 + lane;
        const uint64_t cur = j < nw ? w[j] : 0ull;
        const uint64_t prev = (j > 0 && j - 1 < nw) ? w[j - 1] : 0ull;
        const uint64_t next = j + 1 < nw ? w[j + 1] : 0ull;
        uint64_t s = dec_run_starts(cur, prev >> 63), en = dec_run_ends(cur, next);
        const int cs = __popcll(s), ce = __popcll(en);
        const int is = dec_wave_incl_scan(cs, lane), ie = dec_wave_incl_scan(ce, lane);
        int xs = base_s + is - cs, xe = base_e + ie - ce;
        while (s) {
            e[2 * (size_t)xs++] = (j << 6) + __builtin_ctzll(s);
            s &= s - 1;
        }
        while (en) {
            e[2 * (size_t)xe++ + 1] = (j << 6) + __builtin_ctzll(en);
            en &= en - 1;
        }
        base_s += __shfl(is, 63, 64);
        base_e += __shfl(ie, 63, 64);
    }
    if (lane == 0) n_ev[q] = base_s;
}

// What both decoder entry points (`who`: the name, for the message) ask of the window geometry and of the per-file tables,
// on the host copies; the totals are what the two need to size their launches and bound their indices.
struct DecTotals { long long tiles, words, pairs, frames, t_max; };   // sums over the files, and the longest file's frames
static int dec_check_files(const char* who, const int* win_off_host, const int* frame_len_host, int n_files, int n_frame,
                           int overlap_hop, int n_out, DecTotals* tot) {
    if (overlap_hop > n_frame)
        return fail(IRIS_E_INVALID, "%s: overlap_hop %d > n_frame %d leaves frames no window covers", who, overlap_hop, n_frame);
    if (n_frame % n_out != 0)
        return fail(IRIS_E_INVALID, "%s: n_frame %d is not a multiple of the model's %d output frames", who, n_frame, n_out);
    if (win_off_host[0] < 0) return fail(IRIS_E_INVALID, "%s: win_off[0] = %d < 0", who, win_off_host[0]);
    *tot = DecTotals{};
    for (int f = 0; f < n_files; ++f) {
        const long long tl = frame_len_host[f], nwin = (long long)win_off_host[f + 1] - win_off_host[f];
        if (tl < 0 || nwin < 0) return fail(IRIS_E_INVALID, "%s: file %d: frame_len %lld, windows %lld", who, f, tl, nwin);
        if (tl > 0 && (nwin < 1 || tl > (nwin - 1) * overlap_hop + n_frame))
            return fail(IRIS_E_INVALID, "%s: file %d: frame_len %lld > (%lld - 1) * %d + %d: frames no window covers", who, f, tl,
                        nwin, overlap_hop, n_frame);
        tot->tiles += (tl + kDecTile - 1) / kDecTile;
        tot->words += dec_words(tl);
        tot->pairs += dec_pairs(tl);
        tot->frames += tl;
        tot->t_max = std::max(tot->t_max, tl);
    }
    return IRIS_OK;
}

extern "C" int iris_decode_events(const float* preds, const int* win_off, const int* frame_len, const int* win_off_host,
                                  const int* frame_len_host, int n_files, int n_frame, int overlap_hop, int n_out, int n_classes,
                                  int avg_pool, int max_pool, float threshold, unsigned long long* bits, int* ev, int* n_ev,
                                  void* stream) {
    if (!preds || !win_off || !frame_len || !win_off_host || !frame_len_host || !bits || !ev || !n_ev)
        return fail(IRIS_E_INVALID, "iris_decode_events: NULL pointer argument");
    if (n_files < 1 || n_frame < 1 || overlap_hop < 1 || n_out < 1 || n_classes < 1 || avg_pool < 1 || max_pool < 1)
        return fail(IRIS_E_INVALID, "iris_decode_events: files %d, n_frame %d, overlap_hop %d, n_out %d, K %d, pools %d / %d",
                    n_files, n_frame, overlap_hop, n_out, n_classes, avg_pool, max_pool);
    if (n_classes > kDecMaxK || avg_pool > kDecMaxAvg || max_pool > kDecMaxMax)
        return fail(IRIS_E_UNSUPPORTED, "iris_decode_events: K %d (<= %d), avg_pool %d (<= %d), max_pool %d (<= %d)", n_classes,
                    kDecMaxK, avg_pool, kDecMaxAvg, max_pool, kDecMaxMax);
    DecTotals tot;
    const int rc = dec_check_files("iris_decode_events", win_off_host, frame_len_host, n_files, n_frame, overlap_hop, n_out, &tot);
    if (rc != IRIS_OK) return rc;
    if (tot.tiles > INT_MAX || tot.words * n_classes > INT_MAX || 2 * tot.pairs * n_classes > INT_MAX)
        return fail(IRIS_E_UNSUPPORTED, "iris_decode_events: %lld frames in one call is too many", tot.words * 64);
    const DecPad avg = dec_pad(avg_pool), mx = dec_pad(max_pool);
    const int mw = (std::max(mx.l, mx.r) + 63) / 64;
    hipStream_t s = (hipStream_t)stream;
    if (tot.tiles > 0) {
        k_decode_bits<<<(unsigned)tot.tiles, kDecThreads, 0, s>>>(preds, win_off, frame_len, n_files, n_frame, overlap_hop, n_out,
                                                                  n_frame / n_out, n_classes, avg, mx, mw, threshold,
                                                                  reinterpret_cast<uint64_t*>(bits));
        HIP_TRY(hipGetLastError());
    }
    const int q = n_files * n_classes;
    k_decode_runs<<<(q + 3) / 4, 256, 0, s>>>(frame_len, n_files, n_classes, reinterpret_cast<const uint64_t*>(bits), ev, n_ev);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
