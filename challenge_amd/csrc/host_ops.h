// host_ops.h -- host side: the C-ABI entry points of the operators (argument checks, geometry, launches).
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// host: ops
// ---------------------------------------------------------------------------
static size_t n_chunks_of(size_t row_len) { return (row_len + kChunk - 1) / kChunk; }

extern "C" size_t iris_normalize_workspace(int n_rows, size_t row_len) {
    return n_rows > 0 ? (size_t)n_rows * n_chunks_of(row_len) : 0;
}

extern "C" int iris_normalize(const float* wav, float* out, int n_rows, size_t row_len, float* workspace,
                              size_t workspace_floats, void* stream) {
    if (!wav || !out || !workspace) return fail(IRIS_E_INVALID, "iris_normalize: NULL argument");
    if (n_rows <= 0 || row_len == 0) return fail(IRIS_E_INVALID, "iris_normalize: empty tensor");
    if (n_rows > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_normalize: n_rows %d > 65535", n_rows);
    const size_t n_part = n_chunks_of(row_len);
    if (workspace_floats < iris_normalize_workspace(n_rows, row_len))
        return fail(IRIS_E_CAPACITY, "iris_normalize: workspace %zu floats < %zu", workspace_floats,
                    iris_normalize_workspace(n_rows, row_len));
    hipStream_t s = (hipStream_t)stream;
    k_sumsq_partial<<<dim3((unsigned)n_part, n_rows), 256, 0, s>>>(wav, workspace, row_len, (int)n_part);
    k_normalize_apply<<<dim3((unsigned)n_part, n_rows), 256, 0, s>>>(wav, out, workspace, (int)n_part, row_len);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

static void fused_geometry(const iris_plan* p, int batch, int T, int per_cu, int* chunk_frames, int* chunks_per_clip);

template <int LOG2N>
static hipError_t launch_stft(const StftArgs& a, int grid, size_t lds, hipStream_t s) {
    k_stft<LOG2N><<<grid, 64 * stft_waves(LOG2N), lds, s>>>(a);
    return hipGetLastError();
}

// Geometry of iris_stft for (plan, batch, len): the LDS tile, K1's balanced chunks and the grid.  Host arithmetic only - iris_stft
// launches with exactly these numbers, iris_stft_geometry reports them.
struct StftGeom {
    int tile_frames, chunks_per_clip, n_chunks, grid, waves;
    size_t lds;
};
static int stft_geometry(const iris_plan* p, int batch, int len, StftGeom* g, const char* who) {
    const int T = 1 + len / p->hop;
    const int NC = p->n_fft / 2, F = NC + 1, waves = stft_waves(p->log2n), C2 = 2 * p->channels;
    // tile = as many frames as the LDS left by the waves' exchange buffers holds (one workgroup per
    // CU owns the whole 160 KiB); at least the constant block must fit (it is staged through the tile)
    const size_t xbufs = (size_t)waves * ((wave_buf_bytes(p->log2n) + 15) & ~(size_t)15);
    const int wgs = stft_wgs(p->log2n);  // workgroups per CU
    const size_t room = (160 * 1024 - 1024) / wgs - xbufs;
    auto tile_bytes = [&](int t) { return (size_t)F * ((size_t)t * C2 + 1) * 4; };
    int tf = 1;
    while (tf < 256 && tile_bytes(tf + 1) <= room) ++tf;
    if (tile_bytes(tf) > room) return fail(IRIS_E_UNSUPPORTED, "%s: channels=%d too large", who, p->channels);
    // a whole number of rounds of the workgroup's waves
    const int per_round = std::max(1, waves / std::max(1, p->channels));
    if (tf > per_round) tf -= tf % per_round;
    g->tile_frames = tf;
    g->waves = waves;
    int chunk_frames = 0;
    fused_geometry(p, batch, T, wgs, &chunk_frames, &g->chunks_per_clip);  // K1's balanced chunks, one per workgroup
    g->n_chunks = batch * g->chunks_per_clip;
    g->lds = xbufs + std::max(tile_bytes(tf), (size_t)const_nv4(p->log2n) * 64 * 16);
    if (g->lds > 160 * 1024) return fail(IRIS_E_UNSUPPORTED, "%s: %zu B of LDS", who, g->lds);
    g->grid = std::min(g->n_chunks, p->num_cu * wgs);
    return IRIS_OK;
}

extern "C" int iris_stft_geometry(const iris_plan* p, int batch, int len, int out[5]) {
    const char* who = "iris_stft_geometry";
    if (!p || !out) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (p->mel_only) return fail(IRIS_E_UNSUPPORTED, "%s: plan was created mel-only (n_fft = 0)", who);
    if (batch <= 0 || len <= 0) return fail(IRIS_E_INVALID, "%s: batch=%d len=%d must be positive", who, batch, len);
    if (batch > p->max_batch || len > p->max_len)
        return fail(IRIS_E_CAPACITY, "%s: batch=%d len=%d exceed plan capacity (%d, %d)", who, batch, len, p->max_batch, p->max_len);
    if (len <= p->n_fft / 2) return fail(IRIS_E_INVALID, "%s: len=%d must exceed n_fft/2=%d (reflect padding)", who, len, p->n_fft / 2);
    StftGeom g;
    const int rc = stft_geometry(p, batch, len, &g, who);
    if (rc) return rc;
    out[0] = g.tile_frames;
    out[1] = g.chunks_per_clip;
    out[2] = g.n_chunks;
    out[3] = g.grid;
    out[4] = g.waves;
    return IRIS_OK;
}

extern "C" int iris_stft(iris_plan* p, const float* wav, float* spec, int batch, int len, int flags, void* stream) {
    int rc = check_wav_args(p, wav, spec, batch, len, "iris_stft");
    if (rc) return rc;
    if (flags & ~IRIS_F_NORMALIZE) return fail(IRIS_E_INVALID, "iris_stft: flags 0x%x (only IRIS_F_NORMALIZE applies)", flags);
    StftGeom g;
    if ((rc = stft_geometry(p, batch, len, &g, "iris_stft"))) return rc;
    DeviceGuard guard(p->device);
    StftArgs a;
    a.wav = wav;
    a.spec = spec;
    a.consts = p->d_consts;
    a.B = batch;
    a.C = p->channels;
    a.L = len;
    a.T = 1 + len / p->hop;
    a.hop = p->hop;
    a.tile_frames = g.tile_frames;
    a.chunks_per_clip = g.chunks_per_clip;
    a.chunk_base = a.T / a.chunks_per_clip;
    a.chunk_rem = a.T % a.chunks_per_clip;
    a.n_chunks = g.n_chunks;
    const size_t lds = g.lds;
    const int grid = g.grid;
    hipStream_t s = (hipStream_t)stream;
    a.sumsq = nullptr;
    a.n_sq = 0;
    if (flags & IRIS_F_NORMALIZE) {  // the clip's sum of squares as partial sums in the plan's workspace, folded by the kernel
        const size_t row = (size_t)p->channels * len;
        a.n_sq = (int)((row + kChunk - 1) / kChunk);
        if ((size_t)batch * a.n_sq > p->ws_floats) return fail(IRIS_E_CAPACITY, "iris_stft: workspace too small");
        k_sumsq_partial<<<dim3(a.n_sq, batch), 256, 0, s>>>(wav, p->d_ws, row, a.n_sq);
        a.sumsq = p->d_ws;
    }
    hipError_t e;
    switch (p->log2n) {
        case 11: e = launch_stft<11>(a, grid, lds, s); break;
        case 10: e = launch_stft<10>(a, grid, lds, s); break;
        case 9: e = launch_stft<9>(a, grid, lds, s); break;
        default: e = launch_stft<8>(a, grid, lds, s); break;
    }
    HIP_TRY(e);
    return IRIS_OK;
}

static int grid_for(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 2048 * 4); }

extern "C" int iris_complex_to_magphase(const float* in, float* out, size_t n_outer, int channels, void* stream) {
    if (!in || !out || channels <= 0) return fail(IRIS_E_INVALID, "iris_complex_to_magphase: bad argument");
    if (n_outer == 0) return IRIS_OK;
    k_complex_to_magphase<<<grid_for(n_outer * channels), 256, 0, (hipStream_t)stream>>>(in, out, n_outer, channels);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_magphase_to_complex(const float* in, float* out, size_t n_outer, int channels, void* stream) {
    if (!in || !out || channels <= 0) return fail(IRIS_E_INVALID, "iris_magphase_to_complex: bad argument");
    if (n_outer == 0) return IRIS_OK;
    k_magphase_to_complex<<<grid_for(n_outer * channels), 256, 0, (hipStream_t)stream>>>(in, out, n_outer, channels);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// iris_magmel and its FilterAugment sibling iris_magmel_gain (`gain`: the sibling's kernels, which multiply the finished mel
// values by mel_gain[b, m]); every check happens before the first HIP call
static int magmel_impl(iris_plan* p, const float* spec, float* mel, int batch, int n_frames, int is_magphase, const int32_t* t_bands,
                       int n_tb, const int32_t* f_bands, int n_fb, const float* mel_gain, bool gain, void* stream, const char* who) {
    if (!p || !spec || !mel) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0) return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d", who, batch, n_frames);
    if (gain && !mel_gain) return fail(IRIS_E_INVALID, "%s: mel_gain is NULL", who);
    if (batch > 65535) return fail(IRIS_E_UNSUPPORTED, "%s: batch %d > 65535", who, batch);
    int rc;
    if ((rc = check_bands(t_bands, n_tb, who)) || (rc = check_bands(f_bands, n_fb, who))) return rc;
    DeviceGuard guard(p->device);
    MagmelArgs a;
    a.spec = spec;
    a.mel = mel;
    a.w = p->d_mel;
    a.band_lo = p->d_band_lo;
    a.band_len = p->d_band_len;
    a.t_bands = n_tb ? t_bands : nullptr;
    a.n_tb = n_tb;
    a.f_bands = n_fb ? f_bands : nullptr;
    a.n_fb = n_fb;
    a.B = batch;
    a.C = p->channels;
    a.F = p->n_bins;
    a.T = n_frames;
    a.M = p->n_mel;
    a.is_magphase = is_magphase;
    const bool aligned = (reinterpret_cast<uintptr_t>(spec) & (8 * p->channels - 1)) == 0;
    if (p->tri_ok && (p->channels == 1 || p->channels == 2) && aligned &&
        (size_t)p->n_mel * 64 * p->channels * sizeof(float) <= 64 * 1024 && !p->magmel_generic) {
        MagmelTriArgs t;
        t.spec = spec;
        t.mel = mel;
        t.bin_band = p->d_bin_band;
        t.bin_w = p->d_bin_w;
        t.t_bands = a.t_bands;
        t.n_tb = n_tb;
        t.f_bands = a.f_bands;
        t.n_fb = n_fb;
        t.B = batch;
        t.F = p->n_bins;
        t.T = n_frames;
        t.M = p->n_mel;
        t.is_magphase = is_magphase;
        t.f_lo = p->tri_f_lo;
        t.f_hi = p->tri_f_hi;
        const dim3 grid((n_frames + 63) / 64, batch);
        // split the bins over 8 waves when the grid alone cannot fill the chip
        const int threads = (size_t)grid.x * grid.y * 4 < (size_t)p->num_cu * 8 ? 512 : 256;
        const size_t lds = (size_t)p->n_mel * 64 * p->channels * sizeof(float);
        if (gain) {
            const MagmelTriGainArgs g = {t, mel_gain};
            if (p->channels == 1) k_magmel_tri_gain<1><<<grid, threads, lds, (hipStream_t)stream>>>(g);
            else k_magmel_tri_gain<2><<<grid, threads, lds, (hipStream_t)stream>>>(g);
        } else {
            if (p->channels == 1) k_magmel_tri<1><<<grid, threads, lds, (hipStream_t)stream>>>(t);
            else k_magmel_tri<2><<<grid, threads, lds, (hipStream_t)stream>>>(t);
        }
    } else {
        const int tc = n_frames * p->channels;
        if (gain) k_magmel_gain<<<dim3((tc + 63) / 64, batch), 256, 0, (hipStream_t)stream>>>(MagmelGainArgs{a, mel_gain});
        else k_magmel<<<dim3((tc + 63) / 64, batch), 256, 0, (hipStream_t)stream>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_magmel(iris_plan* p, const float* spec, float* mel, int batch, int n_frames, int is_magphase,
                           const int32_t* t_bands, int n_tb, const int32_t* f_bands, int n_fb, void* stream) {
    return magmel_impl(p, spec, mel, batch, n_frames, is_magphase, t_bands, n_tb, f_bands, n_fb, nullptr, false, stream, "iris_magmel");
}

extern "C" int iris_magmel_gain(iris_plan* p, const float* spec, float* mel, int batch, int n_frames, int is_magphase,
                                const int32_t* t_bands, int n_tb, const int32_t* f_bands, int n_fb, const float* mel_gain,
                                void* stream) {
    return magmel_impl(p, spec, mel, batch, n_frames, is_magphase, t_bands, n_tb, f_bands, n_fb, mel_gain, true, stream,
                       "iris_magmel_gain");
}

// iris_spec_ipd: the mel-band inter-channel phase difference of a stereo complex spectrum (k_ipd.h); every check happens
// before the first HIP call
extern "C" int iris_spec_ipd(iris_plan* p, const float* spec, float* out, int batch, int n_frames, int is_magphase,
                             const int32_t* t_bands, int n_tb, const int32_t* f_bands, int n_fb, void* stream) {
    const char* who = "iris_spec_ipd";
    if (!p || !spec || !out) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0) return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d", who, batch, n_frames);
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the phase difference is that of a stereo pair", who, p->channels);
    if (is_magphase) return fail(IRIS_E_UNSUPPORTED, "%s: magnitude / phase input; a complex spectrum (re0, re1, im0, im1) is expected", who);
    if (batch > 65535) return fail(IRIS_E_UNSUPPORTED, "%s: batch %d > 65535", who, batch);
    if ((reinterpret_cast<uintptr_t>(spec) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(IRIS_E_INVALID, "%s: spec must be 16-byte and out 8-byte aligned", who);
    int rc;
    if ((rc = check_bands(t_bands, n_tb, who)) || (rc = check_bands(f_bands, n_fb, who))) return rc;
    DeviceGuard guard(p->device);
    IpdArgs a;
    a.spec = spec;
    a.out = out;
    a.w = p->d_mel;
    a.band_lo = p->d_band_lo;
    a.band_len = p->d_band_len;
    a.t_bands = n_tb ? t_bands : nullptr;
    a.n_tb = n_tb;
    a.f_bands = n_fb ? f_bands : nullptr;
    a.n_fb = n_fb;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.M = p->n_mel;
    const dim3 grid((n_frames + 63) / 64, batch);
    // the bands go over 8 waves when the grid alone cannot fill the chip (as iris_magmel's streaming kernel does)
    const int threads = (size_t)grid.x * grid.y * 4 < (size_t)p->num_cu * 8 ? 512 : 256;
    k_spec_ipd<<<grid, threads, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// the checks iris_spec_whiten_factors and iris_spec_whiten share (k_whiten.h); every one happens before the first HIP call
static int check_whiten(const iris_plan* p, const float* spec, const float* factors, int batch, int n_frames, int is_magphase,
                        int block, const char* who) {
    if (!p || !spec || !factors) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0) return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d", who, batch, n_frames);
    if (block < 1) return fail(IRIS_E_INVALID, "%s: block=%d must be at least 1 frame", who, block);
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the covariance is that of a stereo pair", who, p->channels);
    if (is_magphase) return fail(IRIS_E_UNSUPPORTED, "%s: magnitude / phase input; a complex spectrum (re0, re1, im0, im1) is expected", who);
    if (batch > 65535) return fail(IRIS_E_UNSUPPORTED, "%s: batch %d > 65535", who, batch);
    if ((reinterpret_cast<uintptr_t>(spec) & 15) || (reinterpret_cast<uintptr_t>(factors) & 15))
        return fail(IRIS_E_INVALID, "%s: spec and factors must be 16-byte aligned", who);
    return IRIS_OK;
}

// iris_spec_whiten_factors: the per-(sample, bin, block) whitening factors of a stereo complex spectrum (k_whiten.h, pass 1)
extern "C" int iris_spec_whiten_factors(iris_plan* p, const float* spec, float* factors, int batch, int n_frames, int is_magphase,
                                        int block, double loading, void* stream) {
    const char* who = "iris_spec_whiten_factors";
    int rc;
    if ((rc = check_whiten(p, spec, factors, batch, n_frames, is_magphase, block, who))) return rc;
    if (!std::isfinite(loading) || loading <= 0.) return fail(IRIS_E_INVALID, "%s: loading=%g must be finite and positive", who, loading);
    DeviceGuard guard(p->device);
    WhitenFactorArgs a;
    a.spec = spec;
    a.fac = factors;
    a.loading = loading;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.block = std::min(block, n_frames);
    a.J = (n_frames + a.block - 1) / a.block;
    a.log2g = 0;
    while (a.log2g < 6 && (4 << a.log2g) < a.block) ++a.log2g;  // G = a quarter of the power of two >= block, 1 ... 64
    const int per_wave = 64 >> a.log2g;
    a.n_waves = (long long)batch * p->n_bins * ((a.J + per_wave - 1) / per_wave);
    const long long blocks = (a.n_waves + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail(IRIS_E_UNSUPPORTED, "%s: %lld workgroups exceed the grid limit", who, blocks);
    k_whiten_factors<false><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// iris_spec_whiten_factors_ranges: the factors of every (sample, bin, block) from the frames a table names, without the masked
// ones (k_whiten.h, K18).  ranges_host is the host's copy of the device table: what is checked here.  Every check that does not
// read the plan comes first, and all of them before the first HIP call.
extern "C" int iris_spec_whiten_factors_ranges(iris_plan* p, const float* spec, const uint8_t* mask, const int32_t* ranges_dev,
                                               const int32_t* ranges_host, float* factors, int batch, int n_frames, int block,
                                               double loading, void* stream) {
    const char* who = "iris_spec_whiten_factors_ranges";
    if (!p || !spec || !mask || !ranges_dev || !ranges_host || !factors) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0) return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d", who, batch, n_frames);
    if (block < 1) return fail(IRIS_E_INVALID, "%s: block=%d must be at least 1 frame", who, block);
    if (!std::isfinite(loading) || loading <= 0.) return fail(IRIS_E_INVALID, "%s: loading=%g must be finite and positive", who, loading);
    if ((reinterpret_cast<uintptr_t>(spec) & 15) || (reinterpret_cast<uintptr_t>(factors) & 15))
        return fail(IRIS_E_INVALID, "%s: spec and factors must be 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(ranges_dev) & 3) return fail(IRIS_E_INVALID, "%s: the range table must be 4-byte aligned", who);
    if (batch > 65535) return fail(IRIS_E_UNSUPPORTED, "%s: batch %d > 65535", who, batch);
    const int blk = std::min(block, n_frames), n_blocks = (n_frames + blk - 1) / blk;
    for (long long i = 0; i < (long long)batch * n_blocks; ++i) {
        const int32_t* r = ranges_host + 3 * i;
        if (r[0] < 0 || r[0] >= r[1] || r[1] > n_frames || (r[2] != 0 && r[2] != 1))
            return fail(IRIS_E_INVALID, "%s: sample %lld, block %lld: frames [%d, %d) of %d, use_mask=%d", who, i / n_blocks,
                        i % n_blocks, r[0], r[1], n_frames, r[2]);
    }
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the covariance is that of a stereo pair", who, p->channels);
    DeviceGuard guard(p->device);
    WhitenRangeArgs a;
    a.spec = spec;
    a.fac = factors;
    a.loading = loading;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.block = blk;
    a.J = n_blocks;
    a.log2g = 0;
    // G from `block` as passed, not cut to n_frames: a recording shorter than a block sums in the order it would in a longer batch
    while (a.log2g < 6 && (4LL << a.log2g) < block) ++a.log2g;
    const int per_wave = 64 >> a.log2g;
    a.n_waves = (long long)batch * p->n_bins * ((a.J + per_wave - 1) / per_wave);
    a.mask = mask;
    a.ranges = ranges_dev;
    const long long blocks = (a.n_waves + 3) / 4;
    if (blocks > 0x7fffffffLL) return fail(IRIS_E_UNSUPPORTED, "%s: %lld workgroups exceed the grid limit", who, blocks);
    k_whiten_factors<true><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// iris_spec_whiten: the whitened mel-band energy from the spectrum and its factors (k_whiten.h, pass 2)
extern "C" int iris_spec_whiten(iris_plan* p, const float* spec, const float* factors, float* out, int batch, int n_frames,
                                int is_magphase, int block, int log, const int32_t* t_bands, int n_tb, const int32_t* f_bands,
                                int n_fb, void* stream) {
    const char* who = "iris_spec_whiten";
    int rc;
    if (!out) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if ((rc = check_whiten(p, spec, factors, batch, n_frames, is_magphase, block, who))) return rc;
    if (reinterpret_cast<uintptr_t>(out) & 3) return fail(IRIS_E_INVALID, "%s: out must be 4-byte aligned", who);
    if ((rc = check_bands(t_bands, n_tb, who)) || (rc = check_bands(f_bands, n_fb, who))) return rc;
    DeviceGuard guard(p->device);
    WhitenArgs a;
    a.spec = spec;
    a.fac = factors;
    a.out = out;
    a.w = p->d_mel;
    a.wnorm = p->d_wnorm;
    a.band_lo = p->d_band_lo;
    a.band_len = p->d_band_len;
    a.t_bands = n_tb ? t_bands : nullptr;
    a.n_tb = n_tb;
    a.f_bands = n_fb ? f_bands : nullptr;
    a.n_fb = n_fb;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.M = p->n_mel;
    a.block = std::min(block, n_frames);
    a.J = (n_frames + a.block - 1) / a.block;
    a.log = log ? 1 : 0;
    k_spec_whiten<<<dim3((n_frames + 63) / 64, batch), 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// iris_locate_events: the noise-whitened steered response of E events over a lag grid (k_locate.h, two launches); every check
// happens before the first HIP call.  events_host is the host's copy of the device table: what is checked here.
// step == 0: K16, rows are the events' segments and `curve` holds one row per event.  step >= 1: K19 (k_track.h), rows are the
// events' steps of `step` frames and `curve` (= R) and n_terms hold one row per step.
static int locate_impl(const char* who, int step, iris_plan* p, const float* spec, const float* factors, int n_blocks,
                       const int32_t* events_dev, const int32_t* events_host, int n_events, int batch, int n_frames, int block,
                       int k_lo, int k_hi, int max_lag, int q, double* workspace, size_t workspace_bytes, double* curve,
                       int64_t* n_terms, void* stream) {
    const bool steps = step != 0;
    if (!p || !spec) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0 || n_events < 0)
        return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d n_events=%d", who, batch, n_frames, n_events);
    if (n_frames > (1 << 30)) return fail(IRIS_E_UNSUPPORTED, "%s: n_frames=%d > 2^30", who, n_frames);
    if (reinterpret_cast<uintptr_t>(spec) & 15) return fail(IRIS_E_INVALID, "%s: spec must be 16-byte aligned", who);
    if (k_lo < 0 || k_lo >= k_hi) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) must be a non-empty range from 0 up", who, k_lo, k_hi);
    if (q < 1 || max_lag < 0) return fail(IRIS_E_INVALID, "%s: q=%d must be >= 1 and max_lag=%d >= 0", who, q, max_lag);
    if (q > 65536) return fail(IRIS_E_UNSUPPORTED, "%s: q=%d > 65536", who, q);
    if (2LL * max_lag + 1 > kLocateMaxLags)
        return fail(IRIS_E_UNSUPPORTED, "%s: %lld lags exceed the limit of %d", who, 2LL * max_lag + 1, kLocateMaxLags);
    if (factors) {
        if (block < 1) return fail(IRIS_E_INVALID, "%s: block=%d must be at least 1 frame", who, block);
        if (reinterpret_cast<uintptr_t>(factors) & 15) return fail(IRIS_E_INVALID, "%s: factors must be 16-byte aligned", who);
        block = std::min(block, n_frames);
        if (n_blocks != (n_frames + block - 1) / block)
            return fail(IRIS_E_INVALID, "%s: factors of %d block(s), but %d frames in blocks of %d make %d", who, n_blocks, n_frames,
                        block, (n_frames + block - 1) / block);
    } else {
        block = n_frames;  // the identity: one block
        n_blocks = 1;
    }
    if (steps && (step < 1 || (n_blocks > 1 && block % step)))
        return fail(IRIS_E_INVALID, "%s: step=%d must be at least 1 frame and divide block=%d (a step lies in one block)", who, step, block);
    const int cut = steps ? step : block;
    if (n_events > 0 && (!events_dev || !events_host || !workspace || !curve || !n_terms)) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if ((reinterpret_cast<uintptr_t>(events_dev) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 7) ||
        (reinterpret_cast<uintptr_t>(curve) & 7) || (reinterpret_cast<uintptr_t>(n_terms) & 7))
        return fail(IRIS_E_INVALID, "%s: the event table must be 4-byte, workspace, curve and n_terms 8-byte aligned", who);
    long long n_seg = 0;
    for (int e = 0; e < n_events; ++e) {
        const int32_t* r = events_host + 4 * (size_t)e;
        if (r[0] < 0 || r[0] >= batch) return fail(IRIS_E_INVALID, "%s: event %d names sample %d of %d", who, e, r[0], batch);
        if (r[1] < 0 || r[1] > r[2] || r[2] >= n_frames)
            return fail(IRIS_E_INVALID, "%s: event %d spans frames %d .. %d of %d", who, e, r[1], r[2], n_frames);
        if (r[3] != n_seg) return fail(IRIS_E_INVALID, "%s: event %d starts at %s %d, expected %lld", who, e, steps ? "row" : "segment", r[3], n_seg);
        n_seg += r[2] / cut - r[1] / cut + 1;
        if (n_seg > 0x7fffffffLL) return fail(IRIS_E_UNSUPPORTED, "%s: more than 2^31 - 1 %s", who, steps ? "rows" : "segments");
    }
    // (the plan is read only now: everything above is checked without it)
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the delay is that of a stereo pair", who, p->channels);
    if (p->n_bins < 2) return fail(IRIS_E_UNSUPPORTED, "%s: a plan of %d bin(s)", who, p->n_bins);
    if (k_hi > p->n_bins) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) leave [0, %d]", who, k_lo, k_hi, p->n_bins);
    if (n_events == 0) return IRIS_OK;  // nothing to do, no launch
    const int nk = k_hi - k_lo, lags = 2 * max_lag + 1;
    const long long mom_waves = n_seg * nk, scan_waves = (steps ? n_seg : (long long)n_events) * lags;
    if (workspace_bytes / 32 < (size_t)mom_waves)
        return fail(IRIS_E_CAPACITY, "%s: workspace of %zu bytes, %lld needed", who, workspace_bytes, 32 * mom_waves);
    if ((mom_waves + 3) / 4 > 0x7fffffffLL || (scan_waves + 3) / 4 > 0x7fffffffLL)
        return fail(IRIS_E_UNSUPPORTED, "%s: %lld / %lld waves exceed the grid limit", who, mom_waves, scan_waves);
    DeviceGuard guard(p->device);
    LocateArgs a;
    a.spec = spec;
    a.fac = factors;
    a.events = events_dev;
    a.mom = workspace;
    a.curve = curve;
    a.n_terms = reinterpret_cast<long long*>(n_terms);
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.J = n_blocks;
    a.block = block;
    a.E = n_events;
    a.S = (int)n_seg;
    a.k_lo = k_lo;
    a.nk = nk;
    a.N = max_lag;
    a.q = q;
    a.L = lags;
    a.period = 2LL * (p->n_bins - 1) * q;  // n_fft q (a mel-only plan carries no n_fft)
    a.cut = cut;  // (K19's field: K16's kernels do not read it)
    const dim3 mom_grid((unsigned)((mom_waves + 3) / 4)), scan_grid((unsigned)((scan_waves + 3) / 4));
    if (steps) {
        k_locate_moments<true><<<mom_grid, 256, 0, (hipStream_t)stream>>>(a);
        HIP_TRY(hipGetLastError());
        k_track_scan<<<scan_grid, 256, 0, (hipStream_t)stream>>>(a);
    } else {
        k_locate_moments<false><<<mom_grid, 256, 0, (hipStream_t)stream>>>(a);
        HIP_TRY(hipGetLastError());
        k_locate_scan<<<scan_grid, 256, 0, (hipStream_t)stream>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_locate_events(iris_plan* p, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                                  const int32_t* events_host, int n_events, int batch, int n_frames, int block, int k_lo, int k_hi,
                                  int max_lag, int q, double* workspace, size_t workspace_bytes, double* curve, int64_t* n_terms,
                                  void* stream) {
    return locate_impl("iris_locate_events", 0, p, spec, factors, n_blocks, events_dev, events_host, n_events, batch, n_frames, block,
                       k_lo, k_hi, max_lag, q, workspace, workspace_bytes, curve, n_terms, stream);
}

// iris_locate_steps: the steered response of every STEP of `step` frames of E events (k_track.h, two launches): iris_locate_events'
// arguments and checks with rows for segments; `response` [rows, 2 max_lag + 1] and n_terms [rows].
extern "C" int iris_locate_steps(iris_plan* p, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                                 const int32_t* events_host, int n_events, int batch, int n_frames, int block, int step, int k_lo,
                                 int k_hi, int max_lag, int q, double* workspace, size_t workspace_bytes, double* response,
                                 int64_t* n_terms, void* stream) {
    const char* who = "iris_locate_steps";
    if (step < 1) return fail(IRIS_E_INVALID, "%s: step=%d must be at least 1 frame", who, step);
    return locate_impl(who, step, p, spec, factors, n_blocks, events_dev, events_host, n_events, batch, n_frames, block, k_lo, k_hi,
                       max_lag, q, workspace, workspace_bytes, response, n_terms, stream);
}

// iris_track_lags: the best path through the lags of every event's step responses (k_track.h, one launch); every check happens
// before the first HIP call.  offsets_host is the host's copy of the device table: what is checked here.
extern "C" int iris_track_lags(iris_plan* p, const double* response, const int32_t* offsets_dev, const int32_t* offsets_host,
                               int n_events, int n_rows, int max_lag, const double* penalty_dev, int n_penalty, int max_jump,
                               int32_t* workspace, size_t workspace_bytes, int32_t* path, void* stream) {
    const char* who = "iris_track_lags";
    if (!p) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (n_events < 0 || n_rows < 0 || max_lag < 0 || max_jump < 0)
        return fail(IRIS_E_INVALID, "%s: n_events=%d n_rows=%d max_lag=%d max_jump=%d", who, n_events, n_rows, max_lag, max_jump);
    if (2LL * max_lag + 1 > kTrackMaxLags)
        return fail(IRIS_E_UNSUPPORTED, "%s: %lld lags exceed the limit of %d", who, 2LL * max_lag + 1, kTrackMaxLags);
    const int lags = 2 * max_lag + 1, jump = std::min(max_jump, lags - 1);
    if (n_penalty != jump + 1)
        return fail(IRIS_E_INVALID, "%s: a penalty table of %d entries, min(max_jump, lags - 1) + 1 = %d expected", who, n_penalty, jump + 1);
    if (n_events > 0 && (!response || !offsets_dev || !offsets_host || !penalty_dev || !workspace || !path))
        return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if ((reinterpret_cast<uintptr_t>(response) & 7) || (reinterpret_cast<uintptr_t>(penalty_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(offsets_dev) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 3) || (reinterpret_cast<uintptr_t>(path) & 3))
        return fail(IRIS_E_INVALID, "%s: response and the penalty table must be 8-byte, offsets, workspace and path 4-byte aligned", who);
    if (n_events > 0 && offsets_host[0] != 0) return fail(IRIS_E_INVALID, "%s: the offsets start at %d, not 0", who, offsets_host[0]);
    for (int e = 0; e < n_events; ++e)
        if (offsets_host[e + 1] <= offsets_host[e])
            return fail(IRIS_E_INVALID, "%s: event %d owns rows %d .. %d: every event has at least one step", who, e, offsets_host[e],
                        offsets_host[e + 1] - 1);
    if (n_events > 0 && offsets_host[n_events] != n_rows)
        return fail(IRIS_E_INVALID, "%s: the offsets end at %d, but there are %d rows", who, offsets_host[n_events], n_rows);
    if (n_events == 0) {
        if (n_rows != 0) return fail(IRIS_E_INVALID, "%s: %d rows without an event", who, n_rows);
        return IRIS_OK;  // nothing to do, no launch
    }
    if (workspace_bytes / 4 / (size_t)lags < (size_t)n_rows)
        return fail(IRIS_E_CAPACITY, "%s: workspace of %zu bytes, %lld needed", who, workspace_bytes, 4LL * lags * n_rows);
    DeviceGuard guard(p->device);
    TrackArgs a;
    a.R = response;
    a.offsets = offsets_dev;
    a.pen = penalty_dev;
    a.back = workspace;
    a.path = path;
    a.E = n_events;
    a.rows = n_rows;
    a.L = lags;
    a.J = jump;
    k_track_viterbi<<<dim3((unsigned)n_events), 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// iris_beamform_events: the MVDR beamformer of E events, one [F, T_e, 2] slab each (k_beamform.h, one launch); every check
// happens before the first HIP call.  events_host is the host's copy of the device table: what is checked here.
// n_tdoa < 0: K17, one delay per event.  n_tdoa >= 0: K19, one delay per output frame, n_tdoa of them.
static int beamform_impl(const char* who, long long n_tdoa, iris_plan* p, const float* spec, const float* factors, int n_blocks,
                         const int32_t* events_dev, const int32_t* events_host, const double* tdoa_dev, int n_events, int batch,
                         int n_frames, int block, int k_lo, int k_hi, float* out, size_t out_floats, void* stream) {
    const bool per_frame = n_tdoa >= 0;
    if (!p || !spec) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (batch <= 0 || n_frames <= 0 || n_events < 0)
        return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d n_events=%d", who, batch, n_frames, n_events);
    if (n_frames > (1 << 30)) return fail(IRIS_E_UNSUPPORTED, "%s: n_frames=%d > 2^30", who, n_frames);
    if (reinterpret_cast<uintptr_t>(spec) & 15) return fail(IRIS_E_INVALID, "%s: spec must be 16-byte aligned", who);
    if (k_lo < 0 || k_lo >= k_hi) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) must be a non-empty range from 0 up", who, k_lo, k_hi);
    if (factors) {
        if (block < 1) return fail(IRIS_E_INVALID, "%s: block=%d must be at least 1 frame", who, block);
        if (reinterpret_cast<uintptr_t>(factors) & 15) return fail(IRIS_E_INVALID, "%s: factors must be 16-byte aligned", who);
        block = std::min(block, n_frames);
        if (n_blocks != (n_frames + block - 1) / block)
            return fail(IRIS_E_INVALID, "%s: factors of %d block(s), but %d frames in blocks of %d make %d", who, n_blocks, n_frames,
                        block, (n_frames + block - 1) / block);
    } else {
        block = n_frames;  // the identity: one block
        n_blocks = 1;
    }
    if (n_events > 0 && (!events_dev || !events_host || !tdoa_dev || !out)) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if ((reinterpret_cast<uintptr_t>(events_dev) & 3) || (reinterpret_cast<uintptr_t>(tdoa_dev) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(IRIS_E_INVALID, "%s: the event table must be 4-byte, tdoa and out 8-byte aligned", who);
    long long total = 0;
    int longest = 0;
    for (int e = 0; e < n_events; ++e) {
        const int32_t* r = events_host + 4 * (size_t)e;
        if (r[0] < 0 || r[0] >= batch) return fail(IRIS_E_INVALID, "%s: event %d names sample %d of %d", who, e, r[0], batch);
        if (r[1] < 0 || r[1] > r[2] || r[2] >= n_frames)
            return fail(IRIS_E_INVALID, "%s: event %d spans frames %d .. %d of %d", who, e, r[1], r[2], n_frames);
        if (r[3] != total) return fail(IRIS_E_INVALID, "%s: event %d starts at output frame %d, expected %lld", who, e, r[3], total);
        total += r[2] - r[1] + 1;
        longest = std::max(longest, r[2] - r[1] + 1);
        if (total > 0x7fffffffLL) return fail(IRIS_E_UNSUPPORTED, "%s: more than 2^31 - 1 output frames", who);
    }
    if (per_frame && n_tdoa != total) return fail(IRIS_E_INVALID, "%s: %lld delays for %lld output frames", who, n_tdoa, total);
    // (the plan is read only now: everything above is checked without it)
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the delay is that of a stereo pair", who, p->channels);
    if (p->n_bins < 2) return fail(IRIS_E_UNSUPPORTED, "%s: a plan of %d bin(s)", who, p->n_bins);
    if (k_hi > p->n_bins) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) leave [0, %d]", who, k_lo, k_hi, p->n_bins);
    if (n_events == 0) return IRIS_OK;  // nothing to do, no launch
    if (out_floats / 2 / (size_t)p->n_bins < (size_t)total)
        return fail(IRIS_E_CAPACITY, "%s: out of %zu floats, %lld needed", who, out_floats, 2LL * p->n_bins * total);
    const int groups = (p->n_bins + kBeamBins - 1) / kBeamBins, chunks = (longest + 63) / 64;
    const long long waves = per_frame ? (long long)p->n_bins * chunks : (long long)groups * ((longest + kBeamChunk - 1) / kBeamChunk);
    if ((waves + 3) / 4 > 65535 || n_events > (1 << 24))
        return fail(IRIS_E_UNSUPPORTED, "%s: %lld waves per event / %d events exceed the grid limit", who, waves, n_events);
    DeviceGuard guard(p->device);
    BeamformArgs a;
    a.spec = spec;
    a.fac = factors;
    a.events = events_dev;
    a.tdoa = tdoa_dev;
    a.out = out;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.J = n_blocks;
    a.block = block;
    a.E = n_events;
    a.k_lo = k_lo;
    a.k_hi = k_hi;
    a.groups = groups;
    a.total = total;
    a.n_fft = 2.0 * (p->n_bins - 1);  // (a mel-only plan carries no n_fft)
    const dim3 grid((unsigned)n_events, (unsigned)((waves + 3) / 4));
    if (per_frame)
        k_beamform_frames<<<grid, 256, 0, (hipStream_t)stream>>>(a, chunks);
    else
        k_beamform<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_beamform_events(iris_plan* p, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                                    const int32_t* events_host, const double* tdoa_dev, int n_events, int batch, int n_frames,
                                    int block, int k_lo, int k_hi, float* out, size_t out_floats, void* stream) {
    return beamform_impl("iris_beamform_events", -1, p, spec, factors, n_blocks, events_dev, events_host, tdoa_dev, n_events, batch,
                         n_frames, block, k_lo, k_hi, out, out_floats, stream);
}

// iris_beamform_frames: iris_beamform_events with one delay per OUTPUT FRAME (k_beamform.h, k_beamform_frames; one launch):
// tdoa_dev [n_tdoa], n_tdoa the frames of all events.
extern "C" int iris_beamform_frames(iris_plan* p, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                                    const int32_t* events_host, const double* tdoa_dev, size_t n_tdoa, int n_events, int batch,
                                    int n_frames, int block, int k_lo, int k_hi, float* out, size_t out_floats, void* stream) {
    const char* who = "iris_beamform_frames";
    if (n_tdoa > 0x7fffffffULL) return fail(IRIS_E_UNSUPPORTED, "%s: more than 2^31 - 1 delays", who);
    return beamform_impl(who, (long long)n_tdoa, p, spec, factors, n_blocks, events_dev, events_host, tdoa_dev, n_events, batch,
                         n_frames, block, k_lo, k_hi, out, out_floats, stream);
}

// iris_postfilter_events: the decision-directed Wiener post-filter over the slabs of iris_beamform_events / _frames
// (k_postfilter.h, one launch); every check happens before the first HIP call.  events_host and gmin_host are the host's
// copies of the device arrays: what is checked here.  per_frame: n_tdoa delays, one per output frame; else one per event.
extern "C" int iris_postfilter_events(iris_plan* p, const float* slabs, const float* factors, int n_blocks, const int32_t* events_dev,
                                      const int32_t* events_host, const double* tdoa_dev, size_t n_tdoa, int per_frame,
                                      const double* gmin_dev, const double* gmin_host, int n_events, int batch, int n_frames,
                                      int block, double loading, double alpha, int k_lo, int k_hi, float* out, size_t out_floats,
                                      void* stream) {
    const char* who = "iris_postfilter_events";
    if (!p || !factors) return fail(IRIS_E_INVALID, "%s: NULL argument (the factors are the noise model: there is no identity)", who);
    if (batch <= 0 || n_frames <= 0 || n_events < 0)
        return fail(IRIS_E_INVALID, "%s: batch=%d n_frames=%d n_events=%d", who, batch, n_frames, n_events);
    if (n_frames > (1 << 30)) return fail(IRIS_E_UNSUPPORTED, "%s: n_frames=%d > 2^30", who, n_frames);
    if (k_lo < 0 || k_lo >= k_hi) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) must be a non-empty range from 0 up", who, k_lo, k_hi);
    if (!(alpha >= 0.0 && alpha < 1.0)) return fail(IRIS_E_INVALID, "%s: alpha=%g must lie in [0, 1)", who, alpha);
    if (!(loading > 0.0 && std::isfinite(loading))) return fail(IRIS_E_INVALID, "%s: loading=%g must be positive and finite", who, loading);
    if (block < 1) return fail(IRIS_E_INVALID, "%s: block=%d must be at least 1 frame", who, block);
    if (reinterpret_cast<uintptr_t>(factors) & 15) return fail(IRIS_E_INVALID, "%s: factors must be 16-byte aligned", who);
    block = std::min(block, n_frames);
    if (n_blocks != (n_frames + block - 1) / block)
        return fail(IRIS_E_INVALID, "%s: factors of %d block(s), but %d frames in blocks of %d make %d", who, n_blocks, n_frames, block,
                    (n_frames + block - 1) / block);
    if (n_events > 0 && (!slabs || !events_dev || !events_host || !tdoa_dev || !gmin_dev || !gmin_host || !out))
        return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if ((reinterpret_cast<uintptr_t>(events_dev) & 3) || (reinterpret_cast<uintptr_t>(tdoa_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(gmin_dev) & 7) || (reinterpret_cast<uintptr_t>(slabs) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(IRIS_E_INVALID, "%s: the event table must be 4-byte, tdoa, g_min, slabs and out 8-byte aligned", who);
    long long total = 0;
    for (int e = 0; e < n_events; ++e) {
        const int32_t* r = events_host + 4 * (size_t)e;
        if (r[0] < 0 || r[0] >= batch) return fail(IRIS_E_INVALID, "%s: event %d names sample %d of %d", who, e, r[0], batch);
        if (r[1] < 0 || r[1] > r[2] || r[2] >= n_frames)
            return fail(IRIS_E_INVALID, "%s: event %d spans frames %d .. %d of %d", who, e, r[1], r[2], n_frames);
        if (r[3] != total) return fail(IRIS_E_INVALID, "%s: event %d starts at output frame %d, expected %lld", who, e, r[3], total);
        total += r[2] - r[1] + 1;
        if (total > 0x7fffffffLL) return fail(IRIS_E_UNSUPPORTED, "%s: more than 2^31 - 1 output frames", who);
        if (!(gmin_host[e] > 0.0 && gmin_host[e] <= 1.0))
            return fail(IRIS_E_INVALID, "%s: event %d has the gain floor %g outside (0, 1]", who, e, gmin_host[e]);
    }
    if (n_tdoa != (per_frame ? (size_t)total : (size_t)n_events))
        return fail(IRIS_E_INVALID, "%s: %zu delays for %lld output frames of %d events (per_frame=%d)", who, n_tdoa, total, n_events,
                    per_frame);
    // (the plan is read only now: everything above is checked without it)
    if (p->channels != 2) return fail(IRIS_E_UNSUPPORTED, "%s: the plan has %d channel(s); the delay is that of a stereo pair", who, p->channels);
    if (p->n_bins < 2) return fail(IRIS_E_UNSUPPORTED, "%s: a plan of %d bin(s)", who, p->n_bins);
    if (k_hi > p->n_bins) return fail(IRIS_E_INVALID, "%s: bins [%d, %d) leave [0, %d]", who, k_lo, k_hi, p->n_bins);
    if (n_events == 0) return IRIS_OK;  // nothing to do, no launch
    if (out_floats / 2 / (size_t)p->n_bins < (size_t)total)
        return fail(IRIS_E_CAPACITY, "%s: out of %zu floats, %lld needed", who, out_floats, 2LL * p->n_bins * total);
    const int groups = (p->n_bins + kPostBins - 1) / kPostBins;
    if (groups > 65535 || n_events > (1 << 24))
        return fail(IRIS_E_UNSUPPORTED, "%s: %d bin groups / %d events exceed the grid limit", who, groups, n_events);
    DeviceGuard guard(p->device);
    PostfilterArgs a;
    a.in = slabs;
    a.fac = factors;
    a.events = events_dev;
    a.tdoa = tdoa_dev;
    a.gmin = gmin_dev;
    a.out = out;
    a.B = batch;
    a.F = p->n_bins;
    a.T = n_frames;
    a.J = n_blocks;
    a.block = block;
    a.E = n_events;
    a.k_lo = k_lo;
    a.k_hi = k_hi;
    a.per_frame = per_frame ? 1 : 0;
    a.total = total;
    a.n_fft = 2.0 * (p->n_bins - 1);  // (a mel-only plan carries no n_fft)
    a.alpha = alpha;
    a.loading = loading;
    k_postfilter<<<dim3((unsigned)n_events, (unsigned)groups), 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" size_t iris_minmax_log_workspace(int n_rows, size_t row_len) {
    return n_rows > 0 ? 2 * (size_t)n_rows * n_chunks_of(row_len) : 0;
}

extern "C" int iris_minmax_log(float* x, int n_rows, size_t row_len, int do_minmax, int do_log, float eps_div,
                               float eps_log, float* workspace, size_t workspace_floats, void* stream) {
    if (!x) return fail(IRIS_E_INVALID, "iris_minmax_log: x is NULL");
    if (n_rows <= 0 || row_len == 0) return fail(IRIS_E_INVALID, "iris_minmax_log: empty tensor");
    if (n_rows > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_minmax_log: n_rows %d > 65535", n_rows);
    hipStream_t s = (hipStream_t)stream;
    const size_t n_part = n_chunks_of(row_len);
    if (do_minmax) {
        if (reinterpret_cast<uintptr_t>(workspace) & 7)
            return fail(IRIS_E_INVALID, "iris_minmax_log: workspace must be 8-byte aligned");
        if (!workspace || workspace_floats < iris_minmax_log_workspace(n_rows, row_len))
            return fail(IRIS_E_CAPACITY, "iris_minmax_log: workspace %zu floats < %zu", workspace_floats,
                        iris_minmax_log_workspace(n_rows, row_len));
        k_minmax_partial<<<dim3((unsigned)n_part, n_rows), 256, 0, s>>>(x, workspace, row_len, (int)n_part);
    }
    k_minmax_log_apply<<<dim3((unsigned)((row_len + kApply - 1) / kApply), n_rows), 256, 0, s>>>(x, workspace, (int)n_part, row_len, do_minmax,
                                                                     do_log, eps_div, eps_log);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

constexpr int kMaxChunkFrames = 16384;
// Chunk geometry of the fused kernel for `per_cu` workgroups per CU: every workgroup one
// chunk when the problem is large enough, chunks never span clips.
static void fused_geometry(const iris_plan* p, int batch, int T, int per_cu, int* chunk_frames, int* chunks_per_clip) {
    const int slots = p->num_cu * per_cu;
    const long total = (long)batch * T;
    int target = p->chunk_target > 0 ? p->chunk_target : (int)((total + slots - 1) / slots);
    target = std::max(target, std::min(8, T));
    int cpc = (T + target - 1) / target;
    // rounding up per clip can overshoot the slots by a few chunks, which would cost a whole
    // second round: prefer slightly larger chunks that fit one round
    if (p->chunk_target == 0 && (long)batch * cpc > slots && batch <= slots) cpc = std::max(1, slots / batch);
    cpc = std::max(cpc, (T + kMaxChunkFrames - 1) / kMaxChunkFrames);  // bounds the time-band bitmap in LDS
    *chunks_per_clip = cpc;
    *chunk_frames = (T + cpc - 1) / cpc;
}

// Geometry + grid of the fused kernel: one workgroup per CU (every wave the registers allow), checked once per
// (kernel, batch, frames) against the occupancy the hardware really grants and cached in the plan - the hot launch
// path does no runtime query.
static int fused_config(iris_plan* p, fused_kernel_t kernel, int batch, int T, int streams, bool bands, int fuse,
                        int* chunk_frames, int* chunks_per_clip, int* grid, size_t* lds) {
    for (const iris_plan::FusedGeom& g : p->geom_cache)
        if (g.kernel == (const void*)kernel && g.batch == batch && g.T == T) {
            *chunk_frames = g.chunk_frames;
            *chunks_per_clip = g.chunks_per_clip;
            *grid = g.grid;
            *lds = g.lds;
            return g.lds == 0 ? IRIS_E_UNSUPPORTED : IRIS_OK;  // lds 0: this shape does not fit (remembered)
        }
    const int per_cu = fuse ? 1 : IRIS_WGS_PER_CU;  // (the epilogue forms need every workgroup resident: one per CU)
    fused_geometry(p, batch, T, per_cu, chunk_frames, chunks_per_clip);
    *lds = fused_lds_bytes(p, streams, bands, *chunk_frames, fuse);
    if (fuse) *lds = fused_tile_off(*lds) + fused_tile_bytes(p, streams, bands, *chunk_frames, fuse);
    *grid = std::min(batch * *chunks_per_clip, p->num_cu * per_cu);
    if (p->geom_cache.size() >= 64) p->geom_cache.clear();
    if (*lds * per_cu > 160 * 1024) {
        p->geom_cache.push_back({(const void*)kernel, batch, T, *chunk_frames, *chunks_per_clip, *grid, 0});
        return fail(IRIS_E_UNSUPPORTED, "fused kernel needs %zu B of LDS", *lds);
    }
    int resident = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, (const void*)kernel,
                                                                64 * fused_waves(p->log2n, streams, bands, p->need_hi != 0, fuse, p->mel_mode), *lds);
    if (e != hipSuccess) return fail((int)e, "hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e));
    if (resident < per_cu) return fail(IRIS_E_UNSUPPORTED, "fused kernel does not fit %d workgroup(s) per CU (LDS %zu B)", per_cu, *lds);
    p->geom_cache.push_back({(const void*)kernel, batch, T, *chunk_frames, *chunks_per_clip, *grid, *lds});
    return IRIS_OK;
}

// bench hook: launch with the kernel's own start/stop timestamps attached to an event pair by the AMD launch
// extension (no hipEventRecord packets of our own on the stream)
static hipError_t launch_timed(std::vector<hipEvent_t>& ev, int& used, const void* kernel, dim3 grid, dim3 block,
                               void** kargs, size_t lds, hipStream_t s) {
    while ((int)ev.size() < 2 * (used + 1)) {
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
    }
    hipError_t rc = hipExtLaunchKernel(kernel, grid, block, kargs, lds, s, ev[2 * used], ev[2 * used + 1], 0);
    if (rc == hipSuccess) ++used;
    return rc;
}

// iris_wav_to_logmel and its FilterAugment sibling iris_wav_to_logmel_gain (`gain`: the sibling's kernels - the same forms,
// geometry and epilogues, the mel values multiplied by mel_gain[b, m] before min / max and log)
static int wav_to_logmel_impl(iris_plan* p, const float* wav, float* out, int batch, int len, int flags, const int32_t* t_bands,
                              int n_tb, const int32_t* f_bands, int n_fb, const float* mel_gain, bool gain, void* stream,
                              const char* who) {
    if (gain && !mel_gain) return fail(IRIS_E_INVALID, "%s: mel_gain is NULL", who);
    int rc = check_wav_args(p, wav, out, batch, len, who);
    if (rc) return rc;
    if ((rc = check_bands(t_bands, n_tb, who)) || (rc = check_bands(f_bands, n_fb, who))) return rc;
    if (take_status(p))  // raised by an earlier launch (host-visible word: no synchronisation here)
        return fail(IRIS_E_EPILOGUE_TIMEOUT,
                    "iris_wav_to_logmel: an earlier fused-epilogue launch of this plan gave up waiting for its clip's other "
                    "workgroups (they were not co-resident: concurrent kernels, a CU mask or another process on the device) and "
                    "wrote NaN; nothing was enqueued by this call, the plan now uses the two-kernel form");
    DeviceGuard guard(p->device);
    hipStream_t s = (hipStream_t)stream;
    FusedArgs a;
    a.wav = wav;
    a.out = out;
    a.consts = p->d_consts;
    a.band_lo = p->d_fband_lo;
    a.wband = p->d_wband;
    a.rows = p->rows;
    a.t_bands = n_tb ? t_bands : nullptr;
    a.n_tb = n_tb;
    a.f_bands = n_fb ? f_bands : nullptr;
    a.n_fb = n_fb;
    a.B = batch;
    a.C = p->channels;
    a.L = len;
    a.T = 1 + len / p->hop;
    a.hop = p->hop;
    a.M = p->n_mel;
    const int do_minmax = (flags & IRIS_F_MINMAX) ? 1 : 0, do_log = (flags & IRIS_F_LOG) ? 1 : 0;
    a.ablate = p->ablate;  // 0 unless this is an IRIS_DIAG build
    a.dbg = p->d_dbg;
    const bool bands = (n_tb > 0) || (n_fb > 0);
    const bool mfma = p->mel_precision == 1 && !bands;  // calls with bands always take the fp32 kernel
    const bool wclass = bands || gain;  // what decides a variant's wave count and LDS (fused_waves): bands or gains
    const int streams = mfma ? 1 : plan_streams(p);
    // min-max / log inside the kernel (one launch) unless: nothing to apply, the MFMA variant, two frame streams
    // (diag), the plan says two kernels, the stream is being captured (the epoch is a host counter: it would be
    // frozen in the graph), or the chunk's mel tile does not fit the LDS
    // fuse: 0 = two kernels, 1 = epilogue from the chunk's LDS tile, 2 = epilogue in place through `out` (only when the plan
    // asks for it, IRIS_EPILOGUE_IN_PLACE: an A/B form - see below)
    int fuse = ((do_minmax || do_log) && !mfma && streams == 1 && p->epilogue != IRIS_EPILOGUE_TWO_KERNELS)
                   ? (p->epilogue == IRIS_EPILOGUE_IN_PLACE ? 2 : 1) : 0;
    if (gain && fuse == 2) fuse = 0;  // the in-place form has no FilterAugment sibling (host_plan.h: fused_pick)
    if (fuse) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) fuse = 0;
    }
    fused_kernel_t kernel = nullptr;
    int grid = 0;
    size_t lds = 0;
    a.wfrag = p->d_wfrag;
    a.tile_ks = p->d_tile_ks;
    a.kb = p->mfma_kb;
    if (mfma) {
        kernel = mfma_kernel(p->log2n, gain);
        fused_geometry(p, batch, a.T, 1, &a.chunk_frames, &a.chunks_per_clip);
        lds = mfma_lds_bytes(p);
        grid = std::min(batch * a.chunks_per_clip, p->num_cu);
    } else {
        if (fuse) {
            kernel = fused_kernel(p->log2n, p->mel_mode, p->need_hi != 0, bands, streams, fuse, gain);
            rc = fused_config(p, kernel, batch, a.T, streams, wclass, fuse, &a.chunk_frames, &a.chunks_per_clip, &grid, &lds);
            // no fused epilogue when the LDS tile does not fit, or when a clip has more chunks than the grid has workgroups (a
            // workgroup would then wait for a chunk it has yet to process itself): the two-kernel form.  (Round 5 measured the
            // in-place form as the fallback for tiles beyond the LDS: same bytes through the same fabric as the second kernel,
            // moved by every CU at the same moment - 3-5 % slower at B = 128 and 512, equal at 256; it stays selectable.)
            if (rc == IRIS_E_UNSUPPORTED || (size_t)batch * a.chunks_per_clip > p->n_slots || a.chunks_per_clip > grid) fuse = 0;
            else if (rc) return rc;
        }
        if (!fuse) {
            kernel = fused_kernel(p->log2n, p->mel_mode, p->need_hi != 0, bands, streams, 0, gain);
            if ((rc = fused_config(p, kernel, batch, a.T, streams, wclass, 0, &a.chunk_frames, &a.chunks_per_clip, &grid, &lds)))
                return rc;
        }
    }
    a.slots = p->d_slots;
    a.status = p->d_status;
    a.timeout_ticks = p->timeout_ticks;
    a.epoch = 0;
    a.tile_off = a.pitch = 0;
    a.do_minmax = do_minmax;
    a.do_log = do_log;
    p->last_form = (do_minmax || do_log) ? (fuse == 1 ? IRIS_EPILOGUE_FUSED : (fuse == 2 ? IRIS_EPILOGUE_IN_PLACE : IRIS_EPILOGUE_TWO_KERNELS)) : -1;
    if (fuse) {
        if (++p->epoch == 0) p->epoch = 1;
        a.epoch = p->epoch;
        a.pitch = fuse == 1 ? fused_tile_pitch(p, a.chunk_frames) : 0;
        a.tile_off = (int)fused_tile_off(fused_lds_bytes(p, streams, wclass, a.chunk_frames, fuse));
    }
    if ((size_t)p->n_mel * a.T * p->channels * 4 > 0xffffffffull || (size_t)a.T * p->channels * 4 >= (1u << 24))
        return fail(IRIS_E_UNSUPPORTED, "%s: clip too long (%d frames x %d channels)", who, a.T, p->channels);
    a.n_chunks = batch * a.chunks_per_clip;
    a.chunk_base = a.T / a.chunks_per_clip;
    a.chunk_rem = a.T % a.chunks_per_clip;
    const int waves = mfma ? kMfmaWaves : fused_waves(p->log2n, streams, wclass, p->need_hi != 0, fuse, p->mel_mode);
    const int parts_per_chunk = waves;
    const size_t n_partial = 2 * (size_t)a.n_chunks * parts_per_chunk;
    a.partial = p->d_ws;
    a.sumsq = nullptr;
    a.n_sq = 0;
    if (flags & IRIS_F_NORMALIZE) {
        const size_t row = (size_t)p->channels * len;
        a.n_sq = (int)((row + kChunk - 1) / kChunk);
        float* sq = p->d_ws + n_partial;
        if (n_partial + (size_t)batch * a.n_sq > p->ws_floats)
            return fail(IRIS_E_CAPACITY, "%s: workspace too small", who);
        k_sumsq_partial<<<dim3(a.n_sq, batch), 256, 0, s>>>(wav, sq, row, a.n_sq);
        a.sumsq = sq;
    }
    if (n_partial > p->ws_floats) return fail(IRIS_E_CAPACITY, "%s: workspace too small", who);

    // bench hook (iris_timing_enable): every n-th call carries event pairs around both kernels; the first
    // kTimingSkip calls after enabling are never sampled (first dispatch on an idle GPU, clock ramp)
    const bool timed = p->timing > 0 && p->launch_no >= kTimingSkip && ((p->launch_no - kTimingSkip) % p->timing) == 0 &&
                       p->ev_used < kMaxTimedLaunches;
    p->launch_no++;
    hipError_t e;
    FusedGainArgs gargs = {a, mel_gain};  // (a sibling's kernel takes this block; `kernel` is then never called as a fused_kernel_t)
    if (timed) {
        FusedArgs args = a;
        void* kargs[] = {gain ? (void*)&gargs : (void*)&args};
        e = launch_timed(p->ev, p->ev_used, (const void*)kernel, dim3(grid), dim3(64 * waves), kargs, lds, s);
    } else if (gain) {
        void* kargs[] = {&gargs};
        e = hipLaunchKernel((const void*)kernel, dim3(grid), dim3(64 * waves), kargs, lds, s);
    } else {
        kernel<<<grid, 64 * waves, lds, s>>>(a);
        e = hipGetLastError();
    }
    HIP_TRY(e);
    if ((do_minmax || do_log) && !fuse) {
        size_t row_len = (size_t)p->n_mel * a.T * p->channels;
        const unsigned n_chunks = (unsigned)((row_len + kApply - 1) / kApply);
        float* x = out;
        const float* partial = p->d_ws;
        int n_part = a.chunks_per_clip * parts_per_chunk, mm = do_minmax, lg = do_log;
        float eps_div = 1e-8f, eps_log = 1e-8f;
        if (timed) {
            void* kargs[] = {&x, &partial, &n_part, &row_len, &mm, &lg, &eps_div, &eps_log};
            e = launch_timed(p->ev2, p->ev2_used, (const void*)k_minmax_log_apply, dim3(n_chunks, batch), dim3(256), kargs, 0, s);
        } else {
            k_minmax_log_apply<<<dim3(n_chunks, batch), 256, 0, s>>>(x, partial, n_part, row_len, mm, lg, eps_div, eps_log);
            e = hipGetLastError();
        }
        HIP_TRY(e);
    }
    return IRIS_OK;
}

extern "C" int iris_wav_to_logmel(iris_plan* p, const float* wav, float* out, int batch, int len, int flags,
                                  const int32_t* t_bands, int n_tb, const int32_t* f_bands, int n_fb,
                                  void* stream) {
    return wav_to_logmel_impl(p, wav, out, batch, len, flags, t_bands, n_tb, f_bands, n_fb, nullptr, false, stream, "iris_wav_to_logmel");
}

extern "C" int iris_wav_to_logmel_gain(iris_plan* p, const float* wav, float* out, int batch, int len, int flags,
                                       const int32_t* t_bands, int n_tb, const int32_t* f_bands, int n_fb,
                                       const float* mel_gain, void* stream) {
    return wav_to_logmel_impl(p, wav, out, batch, len, flags, t_bands, n_tb, f_bands, n_fb, mel_gain, true, stream,
                              "iris_wav_to_logmel_gain");
}

extern "C" int iris_mask_apply(void* x, size_t n_outer, size_t axis_len, size_t n_inner, int elem_size,
                               const int32_t* bands, int n_bands, size_t outer_per_group, void* stream) {
    if (!x) return fail(IRIS_E_INVALID, "iris_mask_apply: x is NULL");
    if (elem_size != 4 && elem_size != 8) return fail(IRIS_E_UNSUPPORTED, "iris_mask_apply: elem_size %d", elem_size);
    int rc = check_bands(bands, n_bands, "iris_mask_apply");
    if (rc) return rc;
    if (outer_per_group == 0) return fail(IRIS_E_INVALID, "iris_mask_apply: outer_per_group must be > 0");
    const size_t total = n_outer * axis_len * n_inner;
    if (total == 0 || n_bands == 0) return IRIS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (elem_size == 4)
        k_mask_apply<uint32_t><<<grid_for(total), 256, 0, s>>>((uint32_t*)x, n_outer, axis_len, n_inner, bands,
                                                              n_bands, outer_per_group);
    else
        k_mask_apply<uint64_t><<<grid_for(total), 256, 0, s>>>((uint64_t*)x, n_outer, axis_len, n_inner, bands,
                                                              n_bands, outer_per_group);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_agc_clip(const iris_agc_row* rows_dev, size_t n_rows, float clip_factor, float eps,
                             float clipvalue, void* stream) {
    if (!rows_dev) return fail(IRIS_E_INVALID, "iris_agc_clip: rows is NULL");
    if (n_rows == 0) return IRIS_OK;
    const int grid = (int)std::min<size_t>((n_rows + 3) / 4, 4096);
    k_agc_clip<<<grid, 256, 0, (hipStream_t)stream>>>(rows_dev, n_rows, clip_factor, eps, clipvalue);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bias_relu(float* x, const float* bias, size_t n_outer, int channels, void* stream) {
    if (!x || !bias) return fail(IRIS_E_INVALID, "iris_bias_relu: NULL argument");
    if (channels <= 0 || (channels & 3)) return fail(IRIS_E_UNSUPPORTED, "iris_bias_relu: channels=%d must be a positive multiple of 4", channels);
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(bias)) & 15)
        return fail(IRIS_E_INVALID, "iris_bias_relu: x and bias must be 16-byte aligned");
    if (n_outer == 0) return IRIS_OK;
    const size_t n4 = n_outer * (size_t)(channels / 4);
    k_bias_relu<<<grid_for(n4), 256, 0, (hipStream_t)stream>>>(x, bias, n4, channels / 4);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bias_relu_maxpool(const float* x, const float* bias, float* y, int batch, int height, int width, int channels,
                                      void* stream) {
    if (!x || !bias || !y) return fail(IRIS_E_INVALID, "iris_bias_relu_maxpool: NULL argument");
    if (channels <= 0 || (channels & 3)) return fail(IRIS_E_UNSUPPORTED, "iris_bias_relu_maxpool: channels=%d must be a positive multiple of 4", channels);
    if (batch <= 0 || height <= 0 || width <= 0) return fail(IRIS_E_INVALID, "iris_bias_relu_maxpool: empty tensor");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(y)) & 15)
        return fail(IRIS_E_INVALID, "iris_bias_relu_maxpool: x, bias and y must be 16-byte aligned");
    const size_t n4 = (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2) * (channels / 4);
    if (n4 >= 2147483648ull) return fail(IRIS_E_UNSUPPORTED, "iris_bias_relu_maxpool: more than 2^31 pooled float4 elements");
    k_bias_relu_pool<<<grid_for(n4), 256, 0, (hipStream_t)stream>>>(x, bias, y, batch, height, width, channels / 4);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bias_relu_nchw(float* x, const float* bias, size_t batch, int channels, size_t inner, void* stream) {
    if (!x || !bias) return fail(IRIS_E_INVALID, "iris_bias_relu_nchw: NULL argument");
    if (channels <= 0 || inner == 0 || (inner & 3)) return fail(IRIS_E_UNSUPPORTED, "iris_bias_relu_nchw: inner size %zu must be a positive multiple of 4", inner);
    if (reinterpret_cast<uintptr_t>(x) & 15) return fail(IRIS_E_INVALID, "iris_bias_relu_nchw: x must be 16-byte aligned");
    if (batch == 0) return IRIS_OK;
    const size_t n4 = batch * (size_t)channels * (inner / 4);
    k_bias_relu_nchw<<<grid_for(n4), 256, 0, (hipStream_t)stream>>>(x, bias, n4, inner / 4, channels);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bias_relu_maxpool_nchw(const float* x, const float* bias, float* y, int batch, int height, int width,
                                           int channels, void* stream) {
    if (!x || !bias || !y) return fail(IRIS_E_INVALID, "iris_bias_relu_maxpool_nchw: NULL argument");
    if (batch <= 0 || height <= 0 || width <= 0 || channels <= 0) return fail(IRIS_E_INVALID, "iris_bias_relu_maxpool_nchw: empty tensor");
    int tile_w = 64;
    while (tile_w > 1 && (size_t)tile_w * (channels + 1) * sizeof(float) > 48 * 1024) tile_w >>= 1;
    const size_t lds = (size_t)tile_w * (channels + 1) * sizeof(float);
    if (lds > 48 * 1024 || batch > 65535 || (height + 1) / 2 > 65535)
        return fail(IRIS_E_UNSUPPORTED, "iris_bias_relu_maxpool_nchw: %d channels / batch %d / height %d out of range", channels, batch, height);
    const int Wo = (width + 1) / 2;
    k_bias_relu_pool_nchw<<<dim3((Wo + tile_w - 1) / tile_w, (height + 1) / 2, batch), 256, lds, (hipStream_t)stream>>>(
        x, bias, y, height, width, channels, tile_w);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

static int bn_check(const void* a, const void* b, size_t rows, int channels, const char* who) {
    if (!a || !b) return fail(IRIS_E_INVALID, "%s: NULL argument", who);
    if (rows == 0 || channels <= 0 || (channels & 3) || channels > 4096)
        return fail(IRIS_E_UNSUPPORTED, "%s: rows %zu, channels %d (a positive multiple of 4, <= 4096)", who, rows, channels);
    return IRIS_OK;
}
static bool bn_overlap(const float* z, size_t n_z, const float* y, size_t n_y) { return y < z + n_z && z < y + n_y; }
static int grid_bn(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 2048); }  // fat blocks: the per-block coefficient setup is amortised
static unsigned bn_reduce_grid(size_t rows, int C4, int rows_per_pass = kBnRows) {
    const int cols = std::min(C4, 256), tys = 256 / cols;
    return (unsigned)((rows + (size_t)rows_per_pass * tys - 1) / ((size_t)rows_per_pass * tys));
}
static size_t bn_reduce_lds(int C4) {
    const int cols = std::min(C4, 256), tys = 256 / cols;
    return (size_t)tys * 2 * cols * 4 * sizeof(float);
}

// (kBnBins blocks of [slot][2][channels]: the statistics passes use the first, a convolution's epilogue all of them - bn_epilogue.h)
extern "C" size_t iris_bn_sums_len(int channels) { return channels > 0 ? (size_t)kBnBins * bn_region(channels) : 0; }

extern "C" int iris_bn_stats(const float* z, size_t rows, int channels, double* sums_zeroed, void* stream) {
    int rc = bn_check(z, sums_zeroed, rows, channels, "iris_bn_stats");
    if (rc) return rc;
    const int C4 = channels / 4;
    k_bn_reduce<false><<<bn_reduce_grid(rows, C4), 256, bn_reduce_lds(C4), (hipStream_t)stream>>>(z, nullptr, rows, C4, nullptr, nullptr,
                                                                                             nullptr, nullptr, sums_zeroed);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

static int bn_relu_apply_impl(const float* z, float* y, size_t rows, int channels, const double* sums, const float* gamma,
                              const float* beta, const float* conv_bias, float eps, float momentum, float* running_mean,
                              float* running_var, float* save_mean, float* save_rstd, int sums_about_zero, void* stream) {
    int rc = bn_check(z, y, rows, channels, "iris_bn_relu_apply");
    if (rc) return rc;
    if (!sums || !gamma || !beta || !running_mean || !running_var || !save_mean || !save_rstd)
        return fail(IRIS_E_INVALID, "iris_bn_relu_apply: NULL argument");
    // every block re-reads K = row 0 of z (the shift of the sums) while other blocks write y: in place, a block could
    // overwrite row 0 before its neighbours have read K
    if (bn_overlap(z, rows * (size_t)channels, y, rows * (size_t)channels)) return fail(IRIS_E_INVALID, "iris_bn_relu_apply: y must not overlap z (not an in-place op)");
    const size_t n4 = rows * (size_t)(channels / 4);
    const double m = (double)rows;
    k_bn_relu_apply<<<grid_bn(n4), 256, 2 * (size_t)channels * sizeof(float), (hipStream_t)stream>>>(z, y, n4, channels / 4, 1.0 / m, rows > 1 ? m / (m - 1.0) : 1.0, sums,
                                                                   gamma, beta, conv_bias, eps, momentum, running_mean, running_var,
                                                                   save_mean, save_rstd, sums_about_zero);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bn_relu_apply(const float* z, float* y, size_t rows, int channels, const double* sums, const float* gamma,
                                  const float* beta, const float* conv_bias, float eps, float momentum, float* running_mean,
                                  float* running_var, float* save_mean, float* save_rstd, void* stream) {
    return bn_relu_apply_impl(z, y, rows, channels, sums, gamma, beta, conv_bias, eps, momentum, running_mean, running_var, save_mean,
                              save_rstd, 0, stream);
}
// the same with `sums` = (sum z, sum z^2) as a convolution's epilogue accumulated them (iris_conv3x3_*_bn): no iris_bn_stats pass
extern "C" int iris_bn_relu_apply_sums0(const float* z, float* y, size_t rows, int channels, const double* sums, const float* gamma,
                                        const float* beta, const float* conv_bias, float eps, float momentum, float* running_mean,
                                        float* running_var, float* save_mean, float* save_rstd, void* stream) {
    return bn_relu_apply_impl(z, y, rows, channels, sums, gamma, beta, conv_bias, eps, momentum, running_mean, running_var, save_mean,
                              save_rstd, 1, stream);
}

extern "C" int iris_bn_relu_bwd_reduce(const float* z, const float* dy, size_t rows, int channels, const float* save_mean,
                                       const float* save_rstd, const float* gamma, const float* beta, double* sums_zeroed,
                                       void* stream) {
    int rc = bn_check(z, sums_zeroed, rows, channels, "iris_bn_relu_bwd_reduce");
    if (rc) return rc;
    if (!dy || !save_mean || !save_rstd || !gamma || !beta) return fail(IRIS_E_INVALID, "iris_bn_relu_bwd_reduce: NULL argument");
    const int C4 = channels / 4;
    k_bn_reduce<true><<<bn_reduce_grid(rows, C4), 256, bn_reduce_lds(C4), (hipStream_t)stream>>>(z, dy, rows, C4, save_mean, save_rstd, gamma,
                                                                                            beta, sums_zeroed);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bn_relu_bwd_dx(const float* z, const float* dy, float* dz, size_t rows, int channels, const float* save_mean,
                                   const float* save_rstd, const float* gamma, const float* beta, const double* sums,
                                   float* dgamma, float* dbeta, void* stream) {
    int rc = bn_check(z, dz, rows, channels, "iris_bn_relu_bwd_dx");
    if (rc) return rc;
    if (!dy || !save_mean || !save_rstd || !gamma || !beta || !sums || !dgamma || !dbeta)
        return fail(IRIS_E_INVALID, "iris_bn_relu_bwd_dx: NULL argument");
    const size_t n4 = rows * (size_t)(channels / 4);
    k_bn_relu_bwd_dx<<<grid_bn(n4), 256, 4 * (size_t)channels * sizeof(float), (hipStream_t)stream>>>(
        z, dy, dz, n4, channels / 4, (float)(1.0 / (double)rows), save_mean, save_rstd, gamma, beta, sums, dgamma, dbeta);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

// -- the same three passes with MaxPool 2x2 / stride 2 / 'same' folded in (z [B, H, W, C]; p, dp [B, ceil(H/2), ceil(W/2), C])
static int bn_pool_check(const void* a, const void* b, int batch, int height, int width, int channels, const char* who) {
    if (batch <= 0 || height <= 0 || width <= 0) return fail(IRIS_E_INVALID, "%s: empty tensor", who);
    if ((double)batch * ((height + 1) / 2) * ((width + 1) / 2) * (double)std::max(channels, 4) / 4 >= 2147483648.0)
        return fail(IRIS_E_UNSUPPORTED, "%s: more than 2^31 pooled float4 elements", who);
    return bn_check(a, b, (size_t)batch * height * width, channels, who);
}

static int bn_relu_pool_apply_impl(const float* z, float* p, int batch, int height, int width, int channels, const double* sums,
                                   const float* gamma, const float* beta, const float* conv_bias, float eps, float momentum,
                                   float* running_mean, float* running_var, float* save_mean, float* save_rstd, int sums_about_zero,
                                   void* stream) {
    int rc = bn_pool_check(z, p, batch, height, width, channels, "iris_bn_relu_pool_apply");
    if (rc) return rc;
    if (bn_overlap(z, (size_t)batch * height * width * channels, p, (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2) * channels))
        return fail(IRIS_E_INVALID, "iris_bn_relu_pool_apply: p must not overlap z");
    if (!sums || !gamma || !beta || !running_mean || !running_var || !save_mean || !save_rstd)
        return fail(IRIS_E_INVALID, "iris_bn_relu_pool_apply: NULL argument");
    const size_t n4 = (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2) * (channels / 4);
    const double m = (double)batch * height * width;  // the statistics are those of the full-size activation
    k_bn_relu_pool_apply<<<grid_bn(n4), 256, 2 * (size_t)channels * sizeof(float), (hipStream_t)stream>>>(
        z, p, batch, height, width, channels / 4, 1.0 / m, m > 1.0 ? m / (m - 1.0) : 1.0, sums, gamma, beta, conv_bias, eps, momentum,
        running_mean, running_var, save_mean, save_rstd, sums_about_zero);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bn_relu_pool_apply(const float* z, float* p, int batch, int height, int width, int channels, const double* sums,
                                       const float* gamma, const float* beta, const float* conv_bias, float eps, float momentum,
                                       float* running_mean, float* running_var, float* save_mean, float* save_rstd, void* stream) {
    return bn_relu_pool_apply_impl(z, p, batch, height, width, channels, sums, gamma, beta, conv_bias, eps, momentum, running_mean,
                                   running_var, save_mean, save_rstd, 0, stream);
}
extern "C" int iris_bn_relu_pool_apply_sums0(const float* z, float* p, int batch, int height, int width, int channels, const double* sums,
                                             const float* gamma, const float* beta, const float* conv_bias, float eps, float momentum,
                                             float* running_mean, float* running_var, float* save_mean, float* save_rstd, void* stream) {
    return bn_relu_pool_apply_impl(z, p, batch, height, width, channels, sums, gamma, beta, conv_bias, eps, momentum, running_mean,
                                   running_var, save_mean, save_rstd, 1, stream);
}

extern "C" int iris_bn_relu_pool_bwd_reduce(const float* z, const float* dp, int batch, int height, int width, int channels,
                                            const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                            double* sums_zeroed, void* stream) {
    int rc = bn_pool_check(z, sums_zeroed, batch, height, width, channels, "iris_bn_relu_pool_bwd_reduce");
    if (rc) return rc;
    if (!dp || !save_mean || !save_rstd || !gamma || !beta) return fail(IRIS_E_INVALID, "iris_bn_relu_pool_bwd_reduce: NULL argument");
    const int C4 = channels / 4;
    const size_t prow = (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2);
    k_bn_pool_bwd_reduce<<<bn_reduce_grid(prow, C4, kBnPoolRows), 256, bn_reduce_lds(C4), (hipStream_t)stream>>>(
        z, dp, batch, height, width, C4, save_mean, save_rstd, gamma, beta, sums_zeroed);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_bn_relu_pool_bwd_dx(const float* z, const float* dp, float* dz, int batch, int height, int width, int channels,
                                        const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                        const double* sums, float* dgamma, float* dbeta, void* stream) {
    int rc = bn_pool_check(z, dz, batch, height, width, channels, "iris_bn_relu_pool_bwd_dx");
    if (rc) return rc;
    if (!dp || !save_mean || !save_rstd || !gamma || !beta || !sums || !dgamma || !dbeta)
        return fail(IRIS_E_INVALID, "iris_bn_relu_pool_bwd_dx: NULL argument");
    const size_t n4 = (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2) * (channels / 4);
    const double m = (double)batch * height * width;
    k_bn_relu_pool_bwd_dx<<<grid_bn(n4), 256, 4 * (size_t)channels * sizeof(float), (hipStream_t)stream>>>(
        z, dp, dz, batch, height, width, channels / 4, (float)(1.0 / m), save_mean, save_rstd, gamma, beta, sums, dgamma, dbeta);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_plan_kernel_name(const iris_plan* p, int with_bands, char* out, int capacity) {
    if (!p || !out || capacity <= 0) return fail(IRIS_E_INVALID, "iris_plan_kernel_name: bad argument");
    if (p->mel_only) return fail(IRIS_E_UNSUPPORTED, "iris_plan_kernel_name: mel-only plan");
    if (p->mel_precision == 1 && !with_bands)
        snprintf(out, (size_t)capacity, "k_wav_to_mel_mfma<%d>", p->log2n);
    else
        snprintf(out, (size_t)capacity, "k_wav_to_mel<%d,%d,%s,%s,1,%d>", p->log2n, p->mel_mode,
                 (p->need_hi && p->mel_mode != 0 && p->mel_mode != 3) ? "true" : "false", with_bands ? "true" : "false",
                 p->epilogue == IRIS_EPILOGUE_FUSED ? 1 : (p->epilogue == IRIS_EPILOGUE_IN_PLACE ? 2 : 0));
    return IRIS_OK;
}

extern "C" int iris_timing_enable(iris_plan* p, int enable) {
    if (!p) return fail(IRIS_E_INVALID, "iris_timing_enable: NULL plan");
    p->timing = enable > 0 ? enable : 0;
    p->launch_no = 0;
    p->ev_used = 0;
    p->ev2_used = 0;
    return IRIS_OK;
}

static int read_events(const std::vector<hipEvent_t>& ev, int used, float* out_ms, int capacity, double* total) {
    *total = 0.0;
    for (int i = 0; i < used; ++i) {
        HIP_TRY(hipEventSynchronize(ev[2 * i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
        *total += ms;
        if (out_ms && i < capacity) out_ms[i] = ms;
    }
    return IRIS_OK;
}

extern "C" int iris_timing_read(iris_plan* p, int* n_launches, float* mean_ms) {
    if (!p || !n_launches || !mean_ms) return fail(IRIS_E_INVALID, "iris_timing_read: NULL argument");
    DeviceGuard guard(p->device);
    double total = 0.0;
    int rc = read_events(p->ev, p->ev_used, nullptr, 0, &total);
    if (rc) return rc;
    *n_launches = p->ev_used;
    *mean_ms = p->ev_used ? (float)(total / p->ev_used) : 0.f;
    p->ev_used = 0;
    p->ev2_used = 0;
    return IRIS_OK;
}

extern "C" int iris_timing_samples(iris_plan* p, int kernel, float* out_ms, int capacity, int* n_samples) {
    if (!p || !n_samples || (capacity > 0 && !out_ms)) return fail(IRIS_E_INVALID, "iris_timing_samples: NULL argument");
    if (kernel != 0 && kernel != 1) return fail(IRIS_E_INVALID, "iris_timing_samples: kernel must be 0 or 1");
    DeviceGuard guard(p->device);
    double total = 0.0;
    const int used = kernel == 0 ? p->ev_used : p->ev2_used;
    int rc = read_events(kernel == 0 ? p->ev : p->ev2, used, out_ms, capacity, &total);
    if (rc) return rc;
    *n_samples = used;
    return IRIS_OK;
}

// ---------------------------------------------------------------------------
// shoebox room simulation (k_ism.h): the checks read the HOST copy of the table, the kernel its device copy
// ---------------------------------------------------------------------------
static int ism_check_record(const iris_ism_src& r, int i, int channels, int max_taps, double fs) {
    if (!r.dst) return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: dst is NULL", i);
    if (r.n_taps < 1 || r.n_taps > kIsmMaxTaps)
        return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: n_taps = %d is outside 1 .. %d", i, r.n_taps, kIsmMaxTaps);
    if (max_taps < r.n_taps) return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: max_taps = %d < n_taps = %d", i, max_taps, r.n_taps);
    for (int a = 0; a < 3; ++a) {
        if (!(std::isfinite(r.room[a]) && r.room[a] > 0))
            return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: room[%d] = %g must be positive and finite", i, a, r.room[a]);
        if (!(r.src[a] >= 0 && r.src[a] <= r.room[a]))
            return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: src[%d] = %g is outside the room [0, %g]", i, a, r.src[a], r.room[a]);
        for (int c = 0; c < channels; ++c)
            if (!(r.mic[c][a] >= 0 && r.mic[c][a] <= r.room[a]))
                return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: mic[%d][%d] = %g is outside the room [0, %g]", i, c, a,
                            r.mic[c][a], r.room[a]);
    }
    if (!(r.beta >= 0 && r.beta < 1)) return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: beta = %g is outside [0, 1)", i, r.beta);
    const IsmGeom g = ism_geometry(r, channels, fs);
    if (!(g.d_min > 0)) return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: the source sits on its nearest microphone", i);
    if (!(g.images <= 2147483647.0))
        return fail(IRIS_E_INVALID, "iris_ism_rir: record %d: a lattice of %.0f images (> 2^31 - 1)", i, g.images);
    return IRIS_OK;
}

static int ism_check(const iris_ism_src* table_host, const void* table_dev, int n_src, int channels, int max_taps, double fs) {
    if (n_src < 0) return fail(IRIS_E_INVALID, "iris_ism_rir: n_src = %d is negative", n_src);
    if (channels <= 0) return fail(IRIS_E_INVALID, "iris_ism_rir: channels = %d must be positive", channels);
    if (channels > IRIS_ISM_MAX_CHAN)
        return fail(IRIS_E_UNSUPPORTED, "iris_ism_rir: channels = %d > %d microphones per record", channels, IRIS_ISM_MAX_CHAN);
    if (n_src == 0) return IRIS_OK;
    if (!table_host || !table_dev) return fail(IRIS_E_INVALID, "iris_ism_rir: table is NULL");
    if (max_taps < 1 || max_taps > kIsmMaxTaps)
        return fail(IRIS_E_INVALID, "iris_ism_rir: max_taps = %d is outside 1 .. %d", max_taps, kIsmMaxTaps);
    if (!(std::isfinite(fs) && fs > 0)) return fail(IRIS_E_INVALID, "iris_ism_rir: sample_rate = %g must be positive and finite", fs);
    if (n_src > 65535) return fail(IRIS_E_UNSUPPORTED, "iris_ism_rir: n_src = %d > 65535", n_src);
    for (int i = 0; i < n_src; ++i) {
        const int rc = ism_check_record(table_host[i], i, channels, max_taps, fs);
        if (rc) return rc;
    }
    return IRIS_OK;
}

extern "C" int iris_ism_rir(const iris_ism_src* table_host, const void* table_dev, int n_src, int channels, int max_taps,
                            double sample_rate, int normalize, void* stream) {
    const int rc = ism_check(table_host, table_dev, n_src, channels, max_taps, sample_rate);
    if (rc || n_src == 0) return rc;
    k_ism_rir<<<(unsigned)n_src, kIsmThreads, 0, (hipStream_t)stream>>>(static_cast<const iris_ism_src*>(table_dev), channels,
                                                                        max_taps, sample_rate, normalize);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
