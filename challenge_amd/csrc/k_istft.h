// k_istft.h -- inverse STFT of a ragged set of complex spectrograms in the reference layout [F, T, 2C] (re block | im block
// last), one launch: torch.istft(n_fft, hop, window = periodic Hann, center = True, onesided, normalized = False, length),
// the inverse of load_wav's Spectrogram(n_fft, power = None).  Part of the single translation unit iris_frontend.hip.
//
// Per record: S [F, T, 2C] -> y [C, len_out], len_out <= (T - 1) hop, with N = n_fft, p = n + N / 2:
//     x_t[i]  = irfft(S[:, t])[i]                                  (the imaginary parts of bins 0 and N / 2 are ignored)
//     y[c, n] = (sum_t w[p - t hop] x_t[p - t hop]) / (sum_t w[p - t hop]^2)     over the frames with 0 <= p - t hop < N,
//                                                                                  in ascending t
//   blockIdx.y = record, blockIdx.x = a tile of `tile` consecutive output samples, all channels.  The frames that cover
//   the tile (its own and the ceil(N / hop) - 1 halo frames on each side: recomputed, never exchanged) are walked in groups
//   of `group` frames:
//   1. stage: a frame's bins sit a row pitch (T 2C floats) apart, so the group's spectra are read as one contiguous run of
//      group * 2C floats per bin into an LDS tile [F][group * 2C | 1] - the mirror image of k_stft's write-out tile;
//   2. transform: one wave per (frame, channel).  The N-point real inverse is ONE NC = N / 2 point complex FFT of the
//      wave-per-frame core (iris_fft.h): Z[k] = E[k] + i O[k] with 2 E[k] = X[k] + conj X[NC - k],
//      2 O[k] = (X[k] - conj X[NC - k]) w^-k packs the even samples into the real and the odd samples into the imaginary
//      part, and the inverse is conj(FFT(conj Z)) - the forward core and its host-built twiddles, unchanged.  Every lane
//      forms the conj Z[k] of its own points from the column of the tile (odd row stride: conflict-free), so there is no
//      exchange before the transform.  w^-k comes from the plan's untangle twiddles (w^-(k + NC / 2) = i w^-k), the window
//      from its window table: both built on the host in double.  The windowed frame goes to an LDS frame buffer;
//   3. overlap-add: thread s owns output sample n0 + s of every channel and adds the group's covering frames to its LDS
//      accumulator in ascending t.
//   After the last group the sample is divided by its envelope (the covering w^2 summed in ascending t from the LDS copy of
//   the window) and stored coalesced.
// The fp32 operation sequence of a sample is 0 + f_t0 + f_t1 + ... over ALL its covering frames in ascending t, then one
// division: it depends neither on the tile nor on the group nor on the batch.  Bitwise reproducible, a batch equals the
// single calls.  A sample whose covering frames are all zero is 0 / envelope = 0 exactly; a NaN stays inside its frame.
// No atomics, no workspace, no synchronisation with the host; every loop bound comes from the descriptor.
#pragma once

constexpr int istft_waves(int log2n) { return log2n >= 11 ? 4 : 8; }
constexpr int kIstftTileMax = 4096, kIstftTileMin = 1024;   // output samples per workgroup
constexpr size_t kIstftLdsMax = 160 * 1024;

static_assert(sizeof(iris_istft_src) == 24, "iris_istft_src is 24 bytes: two pointers, two ints");

struct IstftArgs {
    const iris_istft_src* table;
    const float* consts;
    int C, hop, max_frames;
    int tile;    // output samples per workgroup (even)
    int group;   // frames per pass
};

// a record the kernel leaves alone (the table lives on the device and cannot be checked on the host without a synchronisation)
__device__ __forceinline__ bool istft_skip(const iris_istft_src& d, int hop, int max_frames) {
    return d.n_frames < 2 || d.n_frames > max_frames || d.len_out <= 0 ||
           (long long)d.len_out > (long long)(d.n_frames - 1) * hop || !d.src || !d.dst;
}

// first frame that covers position p (frames t with 0 <= p - t hop < N), before clipping to the record
__device__ __forceinline__ int istft_first_frame(int p, int N, int hop) { return p < N ? 0 : (p - N + hop) / hop; }

template <int LOG2N>
__global__ __launch_bounds__(64 * istft_waves(LOG2N)) void k_istft(const IstftArgs a) {
    constexpr int W = istft_waves(LOG2N), NT = 64 * W;
    constexpr int N = 1 << LOG2N, NC = N / 2, P = FftCfg<LOG2N>::P, NTW = FftCfg<LOG2N>::NTW, F = NC + 1;
    constexpr int kWaveBufBytes = (lds_padded(NC, FftCfg<LOG2N>::PMMAX) * 8 + 15) & ~15;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const iris_istft_src d = a.table[blockIdx.y];
    if (istft_skip(d, a.hop, a.max_frames)) return;
    const int n0 = (int)blockIdx.x * a.tile;
    if (n0 >= d.len_out) return;
    const int n1 = min(n0 + a.tile, d.len_out);   // one past the tile's last output sample
    const int T = d.n_frames, h = a.hop, C = a.C, C2 = 2 * C, G = a.group;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* __restrict__ src = d.src;
    float* __restrict__ dst = d.dst;

    const int row = (G * C2) | 1;   // odd stride: a frame's column is read conflict-free
    cf* lds = reinterpret_cast<cf*>(smem + wv * kWaveBufBytes);
    float* wtab = reinterpret_cast<float*>(smem + W * kWaveBufBytes);   // [N] the window
    float* acc = wtab + N;                                              // [C][tile] overlap-add accumulator
    float* fr = acc + (size_t)C * a.tile;                               // [G * C][N] windowed frames of the group
    float* spec = fr + (size_t)G * C * N;                               // [F][row] spectra of the group

    cf tw[NTW], post[P / 2], win[P];
    {
        float wreg_unused[kMelRegs];
        int lo_unused;
        load_consts<LOG2N>(a.consts, lane, tw, post, win, wreg_unused, lo_unused);
    }
    if (wv == 0) {
#pragma unroll
        for (int q = 0; q < P; ++q) reinterpret_cast<cf*>(wtab)[lane + kWave * q] = win[q];
    }
    for (int i = tid; i < C * a.tile; i += NT) acc[i] = 0.f;

    // frames that cover the tile's positions [p0, p1]
    const int p0 = n0 + N / 2, p1 = n1 - 1 + N / 2;
    const int ta = istft_first_frame(p0, N, h), tb = min(T - 1, p1 / h);
    constexpr float inv_n = 1.0f / (float)N;

    for (int tg0 = ta; tg0 <= tb; tg0 += G) {
        const int g = min(G, tb - tg0 + 1);
        // ---- 1. the group's spectra: per bin one contiguous run of g * 2C floats ----
        {
            const int run = g * C2, total = F * run;
            const float* s0 = src + (size_t)tg0 * C2;
            const size_t pitch = (size_t)T * C2;
            for (int idx = tid; idx < total; idx += NT) {
                const int f = idx / run, r = idx - f * run;
                spec[f * row + r] = s0[(size_t)f * pitch + r];
            }
        }
        __syncthreads();
        // ---- 2. one wave per (frame, channel): conj Z from the tile, forward FFT, conj, scale, window ----
        for (int fc = wv; fc < g * C; fc += W) {
            const int tl = (C == 1) ? fc : fc / C, c = fc - tl * C;
            const float* col = spec + tl * C2 + c;
            cf x[P];
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int k = lane + kWave * q;
                const float ar = col[k * row], br = col[(NC - k) * row];   // X[k], conj X[NC - k]
                float ai = col[k * row + C], bi = -col[(NC - k) * row + C];
                if (q == 0 && lane == 0) ai = bi = 0.f;   // bins 0 and N / 2 are real by definition
                const float ex = ar + br, ey = ai + bi, dx = ar - br, dy = ai - bi;
                // w^-k: conj(post) below NC / 2, i conj(post) above
                const float twr = q < P / 2 ? post[q % (P / 2)].x : post[q % (P / 2)].y;
                const float twi = q < P / 2 ? -post[q % (P / 2)].y : post[q % (P / 2)].x;
                const float ox = dx * twr - dy * twi, oy = dx * twi + dy * twr;   // 2 O
                x[q] = mk(ex - oy, -(ey + ox));                                   // conj(2 E + 2 i O)
            }
            fft_frame<LOG2N>(x, tw, lds, lane);
            cf* out = reinterpret_cast<cf*>(fr + (size_t)fc * N);
#pragma unroll
            for (int q = 0; q < P; ++q)   // samples 2 m, 2 m + 1 of the frame, m = lane + 64 q
                out[lane + kWave * q] = mk((x[q].x * inv_n) * win[q].x, (-x[q].y * inv_n) * win[q].y);
        }
        __syncthreads();
        // ---- 3. overlap-add in ascending t (the next group's staging does not touch fr or acc) ----
        for (int s = tid; s < n1 - n0; s += NT) {
            const int p = n0 + s + N / 2;
            const int t_lo = max(tg0, istft_first_frame(p, N, h)), t_hi = min(tg0 + g - 1, p / h);
            for (int c = 0; c < C; ++c) {
                float v = acc[c * a.tile + s];
                for (int t = t_lo; t <= t_hi; ++t) v += fr[(size_t)((t - tg0) * C + c) * N + (p - t * h)];
                acc[c * a.tile + s] = v;
            }
        }
    }
    __syncthreads();
    // ---- the envelope and the store ----
    for (int s = tid; s < n1 - n0; s += NT) {
        const int p = n0 + s + N / 2;
        const int t_lo = istft_first_frame(p, N, h), t_hi = min(T - 1, p / h);
        float den = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const float w = wtab[p - t * h];
            den += w * w;
        }
        for (int c = 0; c < C; ++c) dst[(size_t)c * d.len_out + n0 + s] = acc[c * a.tile + s] / den;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static const void* istft_kernel(int log2n) {
    switch (log2n) {
        case 11: return (const void*)k_istft<11>;
        case 10: return (const void*)k_istft<10>;
        case 9: return (const void*)k_istft<9>;
        default: return (const void*)k_istft<8>;
    }
}

// frames per pass: 16 (frame, channel) pairs at n_fft 512, scaled so that spectra + frames stay near 96 KiB
static int istft_group(int log2n, int channels) { return std::max(1, ((16 * 512) >> log2n) / channels); }

static size_t istft_lds_bytes(int log2n, int channels, int tile, int group) {
    const int N = 1 << log2n, NC = N / 2, F = NC + 1;
    int pmmax;
    switch (log2n) {
        case 11: pmmax = FftCfg<11>::PMMAX; break;
        case 10: pmmax = FftCfg<10>::PMMAX; break;
        case 9: pmmax = FftCfg<9>::PMMAX; break;
        default: pmmax = FftCfg<8>::PMMAX; break;
    }
    const size_t xbuf = ((size_t)lds_padded(NC, pmmax) * 8 + 15) & ~(size_t)15;
    const size_t row = (size_t)(group * 2 * channels) | 1;
    return (size_t)istft_waves(log2n) * xbuf +
           ((size_t)N + (size_t)channels * tile + (size_t)group * channels * N + (size_t)F * row) * 4;
}

// largest tile whose LDS fits (0: none - too many channels)
static int istft_tile(int log2n, int channels) {
    const int group = istft_group(log2n, channels);
    for (int tile = kIstftTileMax; tile >= kIstftTileMin; tile >>= 1)
        if (istft_lds_bytes(log2n, channels, tile, group) <= kIstftLdsMax) return tile;
    return 0;
}

extern "C" long long iris_istft_len(long long n_frames, int hop) {
    if (n_frames < 2 || hop <= 0) return 0;
    return (n_frames - 1) * (long long)hop;
}

extern "C" int iris_istft(iris_plan* plan, const void* table_dev, int n_src, int max_frames, void* stream) {
    if (!plan) return fail(IRIS_E_INVALID, "iris_istft: plan is NULL");
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_istft: n_src = %d is negative", n_src);
    if (n_src > 0 && !table_dev) return fail(IRIS_E_INVALID, "iris_istft: table is NULL");
    if (max_frames < 2) return fail(IRIS_E_INVALID, "iris_istft: max_frames = %d must be at least 2", max_frames);
    if (plan->mel_only) return fail(IRIS_E_UNSUPPORTED, "iris_istft: plan was created mel-only (n_fft = 0)");
    if (plan->log2n < 8 || plan->log2n > 11) return fail(IRIS_E_UNSUPPORTED, "iris_istft: n_fft = %d is not supported", plan->n_fft);
    if (plan->hop > plan->n_fft / 2)
        return fail(IRIS_E_UNSUPPORTED, "iris_istft: hop = %d exceeds n_fft / 2 = %d (the envelope could vanish)", plan->hop,
                    plan->n_fft / 2);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_istft: n_src = %d > 65535", n_src);
    const int tile = istft_tile(plan->log2n, plan->channels);
    if (tile == 0)
        return fail(IRIS_E_UNSUPPORTED, "iris_istft: %d channels at n_fft %d do not fit the LDS", plan->channels, plan->n_fft);
    const long long max_len = (long long)(max_frames - 1) * plan->hop;
    if (max_len + 2LL * plan->n_fft + kIstftTileMax > (long long)INT_MAX)
        return fail(IRIS_E_UNSUPPORTED, "iris_istft: max_frames = %d at hop %d is more than 2^31 samples", max_frames, plan->hop);
    if (n_src == 0) return IRIS_OK;
    IstftArgs a;
    a.table = static_cast<const iris_istft_src*>(table_dev);
    a.consts = plan->d_consts;
    a.C = plan->channels;
    a.hop = plan->hop;
    a.max_frames = max_frames;
    a.tile = tile;
    a.group = istft_group(plan->log2n, plan->channels);
    const size_t lds = istft_lds_bytes(plan->log2n, plan->channels, tile, a.group);
    const dim3 grid((unsigned)((max_len + tile - 1) / tile), (unsigned)n_src);
    void* params[] = {&a};
    HIP_TRY(hipLaunchKernel(istft_kernel(plan->log2n), grid, dim3(64 * istft_waves(plan->log2n)), params, lds,
                            (hipStream_t)stream));
    return IRIS_OK;
}
