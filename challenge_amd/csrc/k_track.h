// k_track.h -- tracking the delay of a moving event: the steered response of K16 per STEP of frames, and the best path through
// its lags.  Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K19.  Frames are grouped into steps of `step` frames counted from frame 0, block % step == 0, so a step lies in one block of
// whitening factors.  An event (sample, first, last) is cut into the steps u = first / step .. last / step (the first and the
// last may be short); step r of the call is one ROW, events[e][3] the running count of the rows of the events before e.
//
// Step response (iris_locate_steps, two launches): R [rows, L] double and n_terms [rows] int64, L = 2 N + 1.  R[row, n] is
// K16's term sum (k_locate.h) with "segment" read as "step": the moments p00, p11, p10 over the step's frames, the factors
// (a, b, c) of the step's block, the same lag grid and bins; n_terms[row] = the step's frames x its contributing bins.
//   1. k_locate_moments<true> (k_locate.h): K16's wave per (row, bin) with the rows cut at `step`, the factor index t0 / block.
//   2. k_track_scan: one wave per (ROW, lag) - not per (event, lag).  A lane sums the terms of the bins k_lo + l, k_lo + l + 64,
//      ... in that order with K16's statements, one xor tree, lane 0 writes; the lag-0 wave also counts n_terms.  Why per row: a
//      wave per (event, lag) that keeps its lanes' phases across the steps needs either a register array sized for the widest
//      bin range at compile time or a partial sum per step in LDS; a wave per row needs neither, has steps-per-event times the
//      waves (events are short: 64 frames in steps of 16 give 4) and pays for it with one sincospi per (row, bin, lag) instead
//      of one per (event, bin, lag).  A row depends on its own event's record, spectrum and factors only; no atomics.
//   Error, as K16's with one segment per row: |R - exact| <= (n_l + n_s + 72) u sum A, u = 2^-53, n_l = ceil(step frames / 64)
//   (= 1 for steps up to 64 frames), n_s = ceil((k_hi - k_lo) / 64), A as in k_locate.h.
//
// Path (iris_track_lags, one launch): given pen >= 0 as the table P[d] = d pen (double, formed on the host, d = 0 .. Jc, Jc =
// min(J, L - 1)) and the jump limit J, per event over its rows u = 0 .. n - 1:
//     D_0[n] = R[0, n];   D_u[n] = max over n' in [max(0, n - J), min(L - 1, n + J)] of (D_{u-1}[n'] - P[|n - n'|]) + R[u, n]
//     the maximiser is the SMALLEST such n'; path[n - 1] = the smallest argmax of D_{n-1}; earlier rows follow the back-pointers.
//   k_track_viterbi: one workgroup of 256 threads per event.  D is double-buffered in LDS as doubles: 2 x 2049 x 8 = 32.8 KB,
//   which caps tracking at kTrackMaxLags = 2049 lags (N <= 1024); the host refuses more.  Lags are strided over the threads; a
//   thread scans its n' ASCENDING with a strict > (the tie rule), one subtraction and one comparison per candidate, one
//   addition per lag: no product anywhere, so nothing can be contracted into an fma and a host loop that does the same
//   operations gives the same bits.  One barrier per step.  Back-pointers are int32 [rows, L] in a workspace; after the last
//   barrier thread 0 takes the first argmax and walks them back into path [rows] int32.
// ---------------------------------------------------------------------------
constexpr int kTrackMaxLags = 2049;  // 2 N + 1 <= 2049: two rows of doubles in LDS (32.8 KB)

__global__ __launch_bounds__(256) void k_track_scan(const LocateArgs a) {  // a.S rows, a.curve = R [S, L], a.n_terms [S]
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (long long)a.S * a.L) return;  // wave-uniform
    const int s = (int)(wave / a.L), li = (int)(wave % a.L);
    const long long n = (long long)li - a.N;
    int lo = 0, hi = a.E - 1;  // the last event whose first row is <= s (uniform)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.events[4 * mid + 3] <= s) lo = mid; else hi = mid - 1;
    }
    const int b = a.events[4 * lo], first = a.events[4 * lo + 1], last = a.events[4 * lo + 2];
    const int r = first / a.cut + (s - a.events[4 * lo + 3]);
    const int t0 = max(first, r * a.cut), t1 = min(last, (r + 1) * a.cut - 1);  // inclusive
    const int j = t0 / a.block, frames = t1 - t0 + 1;
    // (the host checked every record; a record that does not fit reads nothing and writes zeros)
    const bool fits = b >= 0 && b < a.B && first >= 0 && last < a.T && j >= 0 && j < a.J && t0 <= t1;
    const double period = (double)a.period;
    const double* mom = a.mom + (size_t)s * a.nk * 4;
    double sum = 0.;
    long long count = 0;
    for (int ki = lane; fits && ki < a.nk; ki += 64) {
        const int k = a.k_lo + ki;
        double fa = 1., fb = 1., cr = 0., ci = 0.;
        if (a.fac) {
            const vec4 g = reinterpret_cast<const vec4*>(a.fac)[((size_t)b * a.F + k) * a.J + j];
            fa = g[0], fb = g[1], cr = g[2], ci = g[3];
        }
        if (fa == 0.) continue;  // a silent block contributes nothing
        count += frames;
        const double p00 = mom[4 * ki], p11 = mom[4 * ki + 1], pre = mom[4 * ki + 2], pim = mom[4 * ki + 3];
        long long m = ((long long)k * n) % a.period;  // exact: |k n| < 2^31 2^11
        if (m < 0) m += a.period;
        if (2 * m > a.period) m -= a.period;  // |m| <= period / 2
        double sn, cs;
        sincospi((double)(2 * m) / period, &sn, &cs);  // e = cs - i sn (one rounding in the argument)
        const double s1r = fb * (cs - cr), s1i = fb * (-sn - ci);
        const double s1sq = fma(s1i, s1i, s1r * s1r), a2 = fa * fa;
        const double cross = fma(s1i, pim, s1r * pre);  // Re(conj(s1) p10)
        const double num = a2 * p00 + s1sq * p11 + (2.0 * fa) * cross;
        sum += num / (a2 + s1sq);
    }
    sum = locate_wave_sum(sum);
    if (li == 0) count = locate_wave_sum(count);
    if (lane != 0) return;
    a.curve[wave] = sum;
    if (li == 0) a.n_terms[s] = count;
}

struct TrackArgs {
    const double* R;      // [rows, L]
    const int* offsets;   // [E + 1]: event e owns the rows offsets[e] .. offsets[e + 1] - 1
    const double* pen;    // [Jc + 1]: P[d] = d pen
    int* back;            // [rows, L] workspace
    int* path;            // [rows]
    int E, rows, L, J;    // J already clipped to L - 1
};

__global__ __launch_bounds__(256) void k_track_viterbi(const TrackArgs a) {
    __shared__ double d[2][kTrackMaxLags];
    const int e = blockIdx.x;
    if (e >= a.E) return;
    const int row0 = a.offsets[e], n_rows = a.offsets[e + 1] - row0;
    // (the host checked the offsets and L; a record that does not fit reads nothing and writes nothing: uniform)
    if (row0 < 0 || n_rows < 1 || (long long)row0 + n_rows > a.rows || a.L < 1 || a.L > kTrackMaxLags) return;
    const int L = a.L, J = a.J;
    for (int n = threadIdx.x; n < L; n += 256) d[0][n] = a.R[(size_t)row0 * L + n];
    __syncthreads();
    for (int u = 1; u < n_rows; ++u) {
        const double* prev = d[(u - 1) & 1];
        double* cur = d[u & 1];
        const double* r = a.R + (size_t)(row0 + u) * L;
        int* back = a.back + (size_t)(row0 + u) * L;
        for (int n = threadIdx.x; n < L; n += 256) {
            const int lo = max(0, n - J), hi = min(L - 1, n + J);
            double best = prev[lo] - a.pen[n - lo];
            int arg = lo;
            for (int m = lo + 1; m <= hi; ++m) {  // ascending, strict: the smallest maximiser
                const double v = prev[m] - a.pen[m < n ? n - m : m - n];
                if (v > best) best = v, arg = m;
            }
            cur[n] = best + r[n];
            back[n] = arg;
        }
        __threadfence_block();  // (thread 0 reads the back-pointers of every thread below)
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double* fin = d[(n_rows - 1) & 1];
    int i = 0;
    for (int n = 1; n < L; ++n)
        if (fin[n] > fin[i]) i = n;
    a.path[row0 + n_rows - 1] = i;
    for (int u = n_rows - 1; u >= 1; --u) {
        i = a.back[(size_t)(row0 + u) * L + i];
        a.path[row0 + u - 1] = i;
    }
}
