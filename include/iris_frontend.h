/*
 * iris_frontend.h -- C ABI of the MI355X (gfx950) audio feature frontend.
 *
 * Drop-in boundary for the reference's feature hot path.  The reference
 * (IRIS-AUDIO/challenge) has no FFI of its own -- its boundary is a set of
 * Python callables.  This header is what a binding for
 * those callables binds to; every entry point cites the reference interface it
 * replaces (file:line in the upstream tree).  INTEGRATION.md shows the ctypes
 * stub a maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch / framework types.
 *  - Every tensor argument is a DEVICE pointer owned by the caller (e.g. the
 *    PyTorch caching allocator).  Entry points never allocate, never free and
 *    never synchronise: all work is enqueued on the caller's `stream`
 *    (a hipStream_t passed as void*; NULL = the default stream).  They are
 *    therefore safe to capture into a hipGraph.
 *  - A plan owns its device tables (window, twiddles, mel bands) and a small
 *    workspace.  A plan is bound to one device; calls on one plan must be
 *    issued from one thread at a time (the workspace is shared); distinct plans
 *    are independent.
 *  - Return value: 0 = ok; negative = IRIS_E_* (bad argument / unsupported
 *    shape); positive = hipError_t passed through.  iris_last_error() returns a
 *    thread-local description of the last failure on this thread.
 *  - All arithmetic is IEEE fp32.  Layouts are row-major ("C order").
 *
 * Tensor layouts (reference conventions)
 *    wav   [B, C, L]        fp32 waveform, 16 kHz or any rate
 *    spec  [B, F, T, 2C]    complex STFT, re block then im block on the last
 *                           axis: [..., :C] = re, [..., C:] = im
 *                           (pipeline.py:131-133, data_utils.py:26-27)
 *    mel   [B, M, T, C]     (transforms.py:58-68)
 *    F = n_fft/2 + 1,  T = 1 + L / hop  (torch.stft center=True)
 */
#ifndef IRIS_FRONTEND_H
#define IRIS_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRIS_ABI_VERSION 1

enum {
    IRIS_OK = 0,
    IRIS_E_INVALID = -1,     /* null pointer, non-positive size, inconsistent arguments */
    IRIS_E_UNSUPPORTED = -2, /* shape outside what the kernels are built for */
    IRIS_E_CAPACITY = -3,    /* batch / length larger than the plan was created for */
    IRIS_E_NOMEM = -4,
    IRIS_E_EPILOGUE_TIMEOUT = -5 /* an EARLIER fused-epilogue launch of this plan gave up a bounded wait (see iris_plan_set_epilogue) */
};

/* flags for iris_wav_to_logmel */
enum {
    IRIS_F_MINMAX = 1,    /* apply per-sample min-max (data_utils.py:37-47) */
    IRIS_F_LOG = 2,       /* apply ln(x + 1e-8)       (data_utils.py:50-55) */
    IRIS_F_NORMALIZE = 4  /* apply x / (10 rms) per clip first (data_utils.py:32-34) */
};

typedef struct iris_plan iris_plan;

int iris_abi_version(void);
const char* iris_last_error(void);

/*
 * Host-side helper.  W[F, M] of tf.signal.linear_to_mel_weight_matrix as the
 * reference builds it once per closure (transforms.py:55-56): HTK mel scale,
 * triangles linear in mel, DC bin zeroed, all arithmetic fp32.
 * `out` is HOST memory, n_bins * n_mel floats, row-major [n_bins][n_mel].
 */
int iris_mel_weight_matrix(int n_mel, int n_bins, float sample_rate,
                           float lower_hz, float upper_hz, float* out_host);

/*
 * Plan: the state the closure magphase_to_mel(num_mel_bins,
 * num_spectrogram_bins, sample_rate, **kw) (transforms.py:51-56) and
 * torchaudio.transforms.Spectrogram(n_fft, power=None) (data_utils.py:17) hold.
 *
 *   n_fft       power of two in [256, 2048]; window = periodic Hann(n_fft).
 *               0 = mel-only plan: any n_bins >= 2, only iris_magmel is available
 *               (magphase_to_mel on spectra of an arbitrary bin count)
 *   hop         > 0 (Spectrogram default: n_fft / 2)
 *   n_mel       M >= 1
 *   n_bins      must equal n_fft/2 + 1 (unless n_fft == 0)
 *   channels    C >= 1 audio channels per clip
 *   max_batch, max_len   capacity of the workspace (clips, samples per channel)
 *   mel_host    optional HOST [n_bins*n_mel] matrix to use instead of the
 *               built-in recipe (any non-negative matrix; band structure is
 *               detected); NULL = iris_mel_weight_matrix(...)
 */
int iris_plan_create(iris_plan** out, int device, int n_fft, int hop, int n_mel,
                     int n_bins, float sample_rate, float lower_hz, float upper_hz,
                     int channels, int max_batch, int max_len, const float* mel_host);
int iris_plan_destroy(iris_plan* plan);

/*
 * Precision of the mel contraction of iris_wav_to_logmel (transforms.py:65, tf.tensordot over the bin axis):
 *   IRIS_MEL_F32       (default) banded fp32 reduction on the vector units.  Stated accuracy of the mel magnitudes against
 *                      an fp64 evaluation of the same chain, for every shape, input level and seed:
 *                      |mel - ref| <= 1e-5 |ref| + 4 eps_fp32 xrms[b, t, c] sum_k W[k, m]  (1e-5 relative + the noise floor of
 *                      any fp32 transform: ~1.2 u x the rms of the frame's spectrum on every bin; measured <= 0.45 of this bound
 *                      over 50 seeds x 5 shapes, profiles/r4/hip_vs_fp64_sweep.log; torch.stft's fp32 engine: 0.82);
 *   IRIS_MEL_F16_MFMA  |X| and W in fp16, v_mfma_f32_16x16x32_f16 with fp32 accumulation (BASELINE configs[4]);
 *                      2e-3 relative.  Needs n_fft 512/1024/2048, n_mel <= 128, every band inside the lower
 *                      half of the spectrum and <= 256 bins per group of 16 bands, else IRIS_E_UNSUPPORTED
 *                      (the plan keeps its previous setting).  Calls with SpecAugment bands always run fp32.
 *                      Dynamic range: 2|X| is cast to fp16 (max 65504, 11 significant bits, subnormal below 6e-5), so
 *                      the waveform must be normalised - as load_wav does (data_utils.py:32-34) - or IRIS_F_NORMALIZE
 *                      set, which scales the samples before the transform; un-normalised PCM-range floats without
 *                      that flag overflow to inf.  The fp32 kernel has no such limit.
 */
#define IRIS_MEL_F32 0
#define IRIS_MEL_F16_MFMA 1
int iris_plan_set_mel_precision(iris_plan* plan, int precision);

/*
 * How iris_wav_to_logmel applies min-max / log (data_utils.py:37-55):
 *   IRIS_EPILOGUE_FUSED        (default) inside the fused kernel: ONE launch per call.  A clip's workgroups exchange
 *                              their (min, max) through the plan's device memory while the kernel runs, which needs
 *                              every workgroup of the launch resident (guaranteed: grid <= CUs) and a per-launch epoch
 *                              from the host - so calls made while `stream` is being captured into a hipGraph, the
 *                              fp16-MFMA variant and shapes whose chunk does not fit the LDS tile take the two-kernel
 *                              path by themselves.  Do not run several fused launches CONCURRENTLY on one device
 *                              (plans on different streams): each could hold CUs while waiting for workgroups the
 *                              other keeps from starting (so could a CU mask, or another process on the device).
 *                              The wait is bounded (~2 s), never a hang, and its failure is LOUD: the affected clips come
 *                              out as NaN, the kernel raises the plan's status word - which lives in host-visible memory -
 *                              and the next iris_wav_to_logmel on the plan (it reads the word on entry: no
 *                              synchronisation, no device access) enqueues nothing, switches the plan to TWO_KERNELS for
 *                              good and returns IRIS_E_EPILOGUE_TIMEOUT: outputs of this plan since the last successful
 *                              iris_plan_status / since that call's predecessor are suspect.  Use TWO_KERNELS from the
 *                              start for pipelines that overlap plans.
 *   IRIS_EPILOGUE_TWO_KERNELS  fused kernel (raw mel + per-wave partials), then the min-max / log kernel.
 *   IRIS_EPILOGUE_IN_PLACE     one launch like FUSED, without the LDS tile: the raw mel goes to `out` and the workgroup
 *                              that wrote a chunk finishes its rows in place once the clip's range is known (same
 *                              exchange, same co-residency rules, same bits), for chunks of any size.  Measured 3-5 %
 *                              SLOWER than TWO_KERNELS where the tile does not fit (c2 geometry from batch 128 on: the same
 *                              bytes move through the same fabric, all CUs at once) - an A/B form, never chosen by itself.
 * A plan created while ROC_GLOBAL_CU_MASK or HSA_CU_MASK is set starts on TWO_KERNELS (a CU mask breaks the co-residency).
 * IRIS_EPILOGUE=1 in the environment at plan creation selects TWO_KERNELS (test / A-B hook; so do IRIS_CHUNK_FRAMES=n,
 * frames per chunk of the fused kernel, and IRIS_MAGMEL_GENERIC - test hooks read once per plan, never per launch).
 * iris_plan_status: synchronises with the device, then 0 = every bounded wait so far completed, 1 = one gave up (the
 * word is reset and the plan stays on TWO_KERNELS from then on).
 * iris_plan_set_epilogue_timeout: the bound of those waits in microseconds (default 2,000,000; 0 = give up after the
 * first sweep - the test hook that makes the failure path reachable on a healthy device).
 */
#define IRIS_EPILOGUE_FUSED 0
#define IRIS_EPILOGUE_TWO_KERNELS 1
#define IRIS_EPILOGUE_IN_PLACE 2
int iris_plan_set_epilogue(iris_plan* plan, int mode);
/* form the plan's last iris_wav_to_logmel call took: IRIS_EPILOGUE_* (a FUSED plan reports TWO_KERNELS where it fell back by
 * itself - a chunk tile beyond the LDS, a capture in progress, an earlier epilogue timeout; IN_PLACE is only ever taken when it
 * was asked for), -1 before the first call or when neither min-max nor log was asked for */
int iris_plan_last_epilogue(const iris_plan* plan, int* form_out);
int iris_plan_status(iris_plan* plan, int* status_out);
int iris_plan_set_epilogue_timeout(iris_plan* plan, unsigned long long microseconds);

/* Name of the fused kernel iris_wav_to_logmel launches for this plan (with / without SpecAugment bands), as rocprofv3
 * prints it without the argument list, e.g. "k_wav_to_mel<10,0,false,false,1,true>" (last flag: min-max / log epilogue inside the kernel); HOST buffer. */
int iris_plan_kernel_name(const iris_plan* plan, int with_bands, char* out_host, int capacity);
/* Copy the plan's mel matrix [n_bins*n_mel] to HOST memory. */
int iris_plan_get_mel(const iris_plan* plan, float* out_host);
/* Frames for a clip of `len` samples: 1 + len / hop. */
int iris_plan_num_frames(const iris_plan* plan, int len);

/*
 * resample (data_utils.py:20-21: torchaudio.compliance.kaldi.resample_waveform(wav, r, 16000), the step of load_wav in front of
 * normalize + STFT).  torchaudio (unpinned in requirements.txt:5, not vendored) implements it as functional.resample with
 * lowpass_filter_width 6, rolloff 0.99 and a Hann-windowed sinc: a polyphase FIR of 2 ceil(6 o / (0.99 min(o, n))) + o taps per
 * output phase on the reduced ratio o : n; csrc/k_resample.h restates it (taps in fp64, rounded once).
 * wav: DEVICE [channels][len] fp32 at orig_freq; out: DEVICE [channels][iris_resample_len(len, orig_freq, new_freq)] fp32.
 * orig_freq == new_freq is a copy.  Runs on the current HIP device; the tap table of a rate pair is cached per device.
 */
long long iris_resample_len(long long len, int orig_freq, int new_freq);
int iris_resample(const float* wav, int channels, long long len, int orig_freq, int new_freq, float* out, void* stream);

/*
 * normalize (data_utils.py:32-34):  out[r] = wav[r] / (10 * sqrt(mean(wav[r]^2)))
 * per row r of wav[n_rows, row_len]; one row = all C*L samples of one clip (the
 * reference takes the rms over every channel jointly).  out may alias wav.
 * workspace: DEVICE scratch of iris_normalize_workspace(n_rows, row_len) floats.
 * Runs on the current HIP device.
 */
size_t iris_normalize_workspace(int n_rows, size_t row_len);
int iris_normalize(const float* wav, float* out, int n_rows, size_t row_len, float* workspace,
                   size_t workspace_floats, void* stream);

/*
 * STFT of load_wav (data_utils.py:17-27): reflect-pad n_fft/2, frame at `hop`,
 * periodic Hann, one-sided FFT, no normalisation, written in the reference's
 * [B, F, T, 2C] re-block / im-block layout.
 * flags: 0, or IRIS_F_NORMALIZE = `normalize` of load_wav (data_utils.py:22-23, :32-34: wav / (10 rms), rms over all
 *        channels of a clip jointly) folded into the transform: one partial-sums launch, then the spectrum is scaled by
 *        1 / (10 rms) as it is written (the STFT is linear) - the normalised waveform is never materialised.  Differs
 *        from normalising first by the fp32 rounding of the scaled samples (<= 2e-6 of the spectrum's peak).
 */
int iris_stft(iris_plan* plan, const float* wav, float* spec, int batch, int len, int flags,
              void* stream);
/*
 * The geometry iris_stft launches with for (plan, batch, len), host arithmetic only (no launch, no HIP call):
 * out = { tile_frames (frames of the LDS tile), chunks_per_clip, n_chunks = batch * chunks_per_clip, grid (workgroups),
 * waves per workgroup }.  A clip's 1 + len / hop frames are split into chunks_per_clip chunks whose sizes differ by at
 * most one; a workgroup walks a chunk in tiles of tile_frames frames and takes chunks grid apart.  Same argument checks
 * as iris_stft (NULL: IRIS_E_INVALID; beyond the plan's capacity: IRIS_E_CAPACITY; len <= n_fft / 2: IRIS_E_INVALID).
 */
int iris_stft_geometry(const iris_plan* plan, int batch, int len, int out[5]);

/*
 * complex_to_magphase (transforms.py:111-123) on n_outer rows of 2C floats:
 * out[..., :C] = sqrt(re^2 + im^2), out[..., C:] = atan2(im, re).
 * magphase_to_complex (transforms.py:126-134) is the inverse.
 */
int iris_complex_to_magphase(const float* in, float* out, size_t n_outer, int channels,
                             void* stream);
int iris_magphase_to_complex(const float* in, float* out, size_t n_outer, int channels,
                             void* stream);

/*
 * complex_to_magphase + magphase_to_mel fused (transforms.py:111-123, :58-70,
 * call sites sj_train.py:119-120): mel[b,m,t,c] = sum_f W[f,m] * |spec[b,f,t,c]|.
 * `is_magphase` != 0: `spec` already holds magnitudes in [..., :C] (the phase
 * half is ignored, transforms.py:64), i.e. plain magphase_to_mel.
 * t_bands / f_bands: optional DEVICE int32 [B, n, 2] (offset, size) bands zeroed
 * along time / linear frequency before the reduction -- SpecAugment `mask`
 * (transforms.py:12-40) as `augment` applies it (data_utils.py:58-61) and
 * stft_filter (data_utils.py:126-136).  NULL / 0 = none.
 */
int iris_magmel(iris_plan* plan, const float* spec, float* mel, int batch, int n_frames,
                int is_magphase, const int32_t* t_bands, int n_t_bands,
                const int32_t* f_bands, int n_f_bands, void* stream);

/*
 * Inter-channel phase difference per mel band (opt-in feature; its own kernel, k_spec_ipd - the mel kernels are untouched).
 * spec: a STEREO complex spectrum [batch, n_bins, n_frames, 4] with last axis (re0, re1, im0, im1) - what iris_stft and the
 * mixers write.  out [batch, n_mel, n_frames, 2] = (cos, sin) of the magnitude-weighted band average of X0 conj(X1):
 *     re_k = re0 re1 + im0 im1,  im_k = im0 re1 - re0 im1,  a_k = sqrt((re0^2 + im0^2)(re1^2 + im1^2))
 *     den_m = sum_k W[k,m] a_k,  cos_m = sum_k W[k,m] re_k / (den_m + 1e-20),  sin_m = sum_k W[k,m] im_k / (den_m + 1e-20)
 * with W the plan's mel matrix (any matrix, a user-supplied one included).  cos^2 + sin^2 <= 1 (the length is the band's
 * coherence); identical channels give (1, 0); swapping the channels flips sin; a silent or fully masked band or frame gives
 * exactly (0, 0); a common positive scale of the spectrum cancels.  fp32 error against the float64 form from the same fp32
 * spectrum: at most (2 n_m + 9) 2^-24 on every element, n_m = non-zero weights of band m.
 * t_bands / f_bands: as for iris_magmel (zeroed in the complex spectrum first).  Arguments as iris_magmel; refused before any
 * HIP call: NULL pointers, empty shapes (IRIS_E_INVALID), a plan whose channel count is not 2, is_magphase != 0 (complex
 * spectra only; IRIS_E_UNSUPPORTED), spec not 16-byte or out not 8-byte aligned (IRIS_E_INVALID).  One launch on `stream`,
 * no workspace, no atomics: bitwise reproducible, capturable.
 */
int iris_spec_ipd(iris_plan* plan, const float* spec, float* out, int batch, int n_frames,
                  int is_magphase, const int32_t* t_bands, int n_t_bands,
                  const int32_t* f_bands, int n_f_bands, void* stream);

/*
 * Spatially whitened mel-band energy (opt-in feature; its own two kernels, k_whiten.h - the mel kernels are untouched): the
 * two-microphone adaptive-matched-filter statistic x^H (R + d I)^-1 x, which stays near 2 for a frame that holds only the
 * coherent interferer dominating R, however loud, and rises for energy from any other direction.
 * spec: a STEREO complex spectrum [batch, n_bins, n_frames, 4] = (re0, re1, im0, im1), as for iris_spec_ipd.  Frames are
 * grouped into J = ceil(n_frames / block) consecutive blocks of `block` frames from frame 0 (block > n_frames counts as
 * n_frames; the last block may be shorter).
 *
 * iris_spec_whiten_factors: per (sample, bin, block), over the block's n frames,
 *     r00 = mean |X0|^2,  r11 = mean |X1|^2,  r10 = mean X1 conj(X0),  d = loading (r00 + r11) / 2
 *     d == 0 (a silent block): a = b = c = 0
 *     else l00 = sqrt(r00 + d),  l10 = r10 / l00,  l11 = sqrt(r11 + d - |l10|^2),  a = 1 / l00,  b = 1 / l11,  c = l10 / l00
 * (the Cholesky factor of R + d I, inverted), accumulated and factorised in double and written as (a, b, Re c, Im c) fp32 into
 * factors [batch, n_bins, J, 4] (caller-provided, 16-byte aligned).  Each of a, b and |c| is within 4 * 2^-24 relative of the
 * float64 form from the same fp32 spectrum.
 *
 * iris_spec_whiten: out [batch, n_mel, n_frames] fp32,
 *     z0 = a X0,  z1 = b (X1 - c X0),  q = |z0|^2 + |z1|^2,  e[m, t] = wnorm[m] sum_k W[k, m] q[k, t]
 * with W the plan's mel matrix (any matrix) and wnorm[m] = 1 / (2 sum_k W[k, m]) (0 for an all-zero band); log != 0 writes
 * ln(e + 1e-8).  The mean of e over a block lies in (0, 1]; zero frames and silent blocks give exactly 0; scaling a bin
 * leaves e unchanged (by a power of two: the same bits).  fp32 error of e against the float64 form from the same fp32
 * spectrum: at most (n_m + 16) 2^-24 A[m, t], A = wnorm[m] sum_k W[k, m] (|z0|^2 + ((|X1| + |c| |X0|) b)^2), n_m = non-zero
 * weights of band m.  t_bands / f_bands ([batch, n, 2] (offset, size)) act on the OUTPUT only: a frame inside a time band gives
 * e = 0, a bin inside a frequency band adds nothing to the sum; neither the covariance nor wnorm sees them (unlike
 * iris_spec_ipd, which zeroes the spectrum first: that would change R).
 *
 * Refused before any HIP call: NULL pointers (the factor buffer included), empty shapes, block < 1, loading not finite or
 * <= 0, a bands pointer / count mismatch, spec or factors not 16-byte aligned (IRIS_E_INVALID); a plan whose channel count is
 * not 2, is_magphase != 0 (IRIS_E_UNSUPPORTED).  One launch each on `stream`, no workspace, no atomics, fixed summation
 * orders: bitwise reproducible, independent of the batch a sample sits in, capturable.
 */
int iris_spec_whiten_factors(iris_plan* plan, const float* spec, float* factors, int batch, int n_frames,
                             int is_magphase, int block, double loading, void* stream);
int iris_spec_whiten(iris_plan* plan, const float* spec, const float* factors, float* out, int batch, int n_frames,
                     int is_magphase, int block, int log, const int32_t* t_bands, int n_t_bands,
                     const int32_t* f_bands, int n_f_bands, void* stream);

/*
 * iris_spec_whiten_factors_ranges (k_whiten.h, K18): the same factors, with the covariance of every (sample, block) taken
 * over the frames a table names - the noise covariance from the frames OUTSIDE detected events.
 * mask: DEVICE bytes [batch, n_frames], non-zero where a frame is inside an event.  ranges: int32 [batch, J, 3] = (t0, t1,
 * use_mask) per (sample, block), J = ceil(n_frames / min(block, n_frames)), once on the device (ranges_dev, what the kernel
 * reads) and once on the host (ranges_host, what is checked here).  The means r00, r11, r10 of block j are taken over the
 * frames t of [t0, t1) that count: with use_mask = 1 those with mask[sample, t] == 0, with use_mask = 0 all of them; the
 * factorisation is iris_spec_whiten_factors'.  use_mask = 1 with no unmasked frame in the range: a = b = c = 0, like a
 * silent block.  A range may lie anywhere in [0, n_frames) and have any length (the block and its neighbours).
 * factors [batch, n_bins, J, 4] as above; each of a, b and |c| is within 4 * 2^-24 relative of the float64 form from the same
 * fp32 spectrum.  A group of G lanes sums a range, G a function of `block` AS PASSED (a quarter of the power of two >=
 * block, 1 .. 64; not cut to n_frames, so that a recording shorter than a block is summed in the same order when it is padded
 * into a longer batch).  With block <= n_frames, a row (j block, min((j + 1) block, n_frames), 0) gives the bits of
 * iris_spec_whiten_factors for that block, and so does use_mask = 1 under an all-zero mask.
 * Refused before any HIP call: NULL pointers, empty shapes, block < 1, loading not finite or <= 0, spec or factors not 16-byte
 * aligned, a device table that is not 4-byte aligned, a ranges_host row with t0 < 0, t0 >= t1, t1 > n_frames or use_mask
 * outside {0, 1} (IRIS_E_INVALID); batch > 65535, a plan whose channel count is not 2 (IRIS_E_UNSUPPORTED).  One launch on
 * `stream`, no workspace, no atomics, fixed summation orders: bitwise reproducible, independent of the batch a sample sits in,
 * capturable.
 */
int iris_spec_whiten_factors_ranges(iris_plan* plan, const float* spec, const uint8_t* mask, const int32_t* ranges_dev,
                                    const int32_t* ranges_host, float* factors, int batch, int n_frames, int block,
                                    double loading, void* stream);

/*
 * Event localisation (k_locate.h): the noise-whitened steered response of a two-microphone delay vector over the frames of
 * detected events - the adaptive matched filter the whitening factors above were built for.
 * spec: a STEREO complex spectrum [batch, n_bins, n_frames, 4] = (re0, re1, im0, im1); factors: [batch, n_bins, n_blocks, 4]
 * = (a, b, Re c, Im c) as iris_spec_whiten_factors writes them for blocks of `block` frames (block > n_frames counts as
 * n_frames), or NULL: a = b = 1, c = 0 and one block - the plain power-weighted steered response (`block` and `n_blocks` are
 * then not used).  Events: int32 [n_events, 4] = (sample, first frame, last frame, first segment), frames inclusive, once on
 * the device (events_dev, what the kernels read) and once on the host (events_host, what is checked here): an event is cut
 * at block boundaries into the segments j = first / block .. last / block, and `first segment` is the running count of the
 * segments of the events before it.  Lags n = -max_lag .. max_lag in steps of 1 / q sample, bins [k_lo, k_hi).
 * Per (segment, bin k) with (a, b, c) = factors[sample, k, j], a != 0 (a == 0, a silent block, contributes nothing):
 *     z0 = a X0,  z1 = b (X1 - c X0),  p00 = sum |z0|^2,  p11 = sum |z1|^2,  p10 = sum z1 conj(z0)   over the segment's frames
 *     e = exp(-i 2 pi k n / (n_fft q))   (a positive delay: channel 1 hears it later),  s1 = b (e - c)
 *     term = (a^2 p00 + |s1|^2 p11 + 2 a Re(conj(s1) p10)) / (a^2 + |s1|^2)      ( = sum_t |s^H z|^2 / (s^H s), s = [a, s1])
 * curve [n_events, 2 max_lag + 1] double: the sum of the terms over the event's segments and bins; n_terms [n_events] int64:
 * the sum over the contributing (segment, bin) pairs of the segment's frame count (curve / n_terms is near 1 under noise
 * alone).  Everything is accumulated in double from the fp32 inputs; against the float64 definition from the same inputs
 * |curve - exact| <= (n_l + n_s + 72) 2^-53 sum A, A a term's magnitude with nothing cancelled (k_locate.h), n_l =
 * ceil(longest segment / 64), n_s = segments of the event x ceil((k_hi - k_lo) / 64).
 * workspace: DEVICE scratch of 32 bytes x (segments of all events) x (k_hi - k_lo), 8-byte aligned.
 * Refused before any HIP call: NULL plan or spec, empty shapes, n_events < 0, spec or factors not 16-byte aligned, block < 1
 * or n_blocks != ceil(n_frames / block) (with factors), a bin range that is empty or leaves [0, n_bins], q < 1, max_lag < 0
 * (IRIS_E_INVALID); a plan whose channel count is not 2, more than 4097 lags (max_lag > 2048), q > 65536, n_frames > 2^30
 * (IRIS_E_UNSUPPORTED); then, with n_events > 0: NULL or misaligned tables and outputs, an event naming a sample outside
 * [0, batch), frames outside [0, n_frames) or first > last, a `first segment` that is not the running count (IRIS_E_INVALID),
 * a workspace that is too small (IRIS_E_CAPACITY).  n_events == 0 returns IRIS_OK without a launch.  Two launches on `stream`,
 * no atomics, fixed summation orders: bitwise reproducible, and an event's row depends on no other event or sample of the call.
 */
int iris_locate_events(iris_plan* plan, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                       const int32_t* events_host, int n_events, int batch, int n_frames, int block, int k_lo, int k_hi,
                       int max_lag, int q, double* workspace, size_t workspace_bytes, double* curve, int64_t* n_terms,
                       void* stream);

/*
 * Event extraction (k_beamform.h): the MVDR (minimum-variance distortionless-response) beamformer w = R^-1 d / (d^H R^-1 d)
 * of a two-microphone delay vector d = [1, e], applied over the frames of detected events - the audio of an event with the
 * interferer the whitening factors describe nulled.
 * spec, factors, n_blocks, block, k_lo, k_hi: as for iris_locate_events (factors NULL: a = b = 1, c = 0 and one block, the
 * delay-and-sum beamformer Y = (X0 + conj(e) X1) / 2).  Events: int32 [n_events, 4] = (sample, first frame, last frame, first
 * output frame), frames inclusive, once on the device (events_dev, what the kernel reads) and once on the host (events_host,
 * what is checked here); `first output frame` is the running count of the frames of the events before it.  tdoa_dev: DEVICE
 * double [n_events], the delay of each event in samples, positive when channel 1 hears the event later (locate_peak's sign).
 * For event e, frame t in first .. last, block j = t / block, bin k, (a, b, c) = factors[sample, k, j]:
 *     k outside [k_lo, k_hi), a == 0 (a silent block) or tdoa not finite:  Y = 0 exactly
 *     r = k tdoa / n_fft (double, n_fft = 2 (n_bins - 1)),  r -= rint(r),  e = cos(2 pi r) - i sin(2 pi r)
 *     s1 = b (e - c),  den = a^2 + |s1|^2,  g1 = b conj(s1) / den,  g0 = a^2 / den - g1 c,   Y = g0 X0 + g1 X1
 * out: slab e = [n_bins, T_e, 2] = (Re Y, Im Y) fp32, T_e = last - first + 1, at float 2 n_bins x (first output frame): the
 * record layout of iris_istft for one channel.  g0, g1 are formed in double and rounded once to fp32; per component one
 * product and three fmas in a fixed order.  Against the float64 definition from the same fp32 inputs, per real component,
 * |Y - exact| <= 6 x 2^-24 A, A = |g0| |X0| + |g1| |X1| (nothing cancelled; the count is in k_beamform.h).  X1 = e X0 gives
 * Y = X0 (distortionless).
 * Refused before any HIP call: NULL plan or spec, empty shapes, n_events < 0, spec or factors not 16-byte aligned, block < 1
 * or n_blocks != ceil(n_frames / block) (with factors), a bin range that is empty or leaves [0, n_bins] (IRIS_E_INVALID);
 * n_frames > 2^30, a plan whose channel count is not 2 (IRIS_E_UNSUPPORTED); then, with n_events > 0: a NULL table, tdoa or
 * out, a table that is not 4-byte or tdoa / out that are not 8-byte aligned, an event naming a sample outside [0, batch),
 * frames outside [0, n_frames) or first > last, a `first output frame` that is not the running count (IRIS_E_INVALID), more
 * than 2^31 - 1 output frames, more than 2^24 events, ceil(n_bins / 16) x ceil(longest event / 256) > 262140 (the grid;
 * IRIS_E_UNSUPPORTED), out_floats <
 * 2 n_bins x (frames of all events) (IRIS_E_CAPACITY).  n_events == 0 returns IRIS_OK without a launch.  One launch on
 * `stream`, no workspace, no atomics: capturable, bitwise reproducible, and a frame's value depends on its sample, frame, bin
 * and delay only - not on the event it sits in or on the other events of the call.
 */
int iris_beamform_events(iris_plan* plan, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                         const int32_t* events_host, const double* tdoa_dev, int n_events, int batch, int n_frames, int block,
                         int k_lo, int k_hi, float* out, size_t out_floats, void* stream);

/*
 * Tracking the delay of a moving event (k_track.h, K19): the steered response per STEP of frames, the best path through its
 * lags, and the beamformer steered per frame.
 *
 * iris_locate_steps: iris_locate_events with "segment" read as "step".  Frames are grouped into steps of `step` frames counted
 * from frame 0; with more than one block, block % step == 0 is required, so a step lies in one block.  Events: int32
 * [n_events, 4] = (sample, first frame, last frame, first row): an event is cut into the steps first / step .. last / step (the
 * first and last may be short), each one ROW, and `first row` is the running count of the rows of the events before it.
 * response [rows, 2 max_lag + 1] double: per row iris_locate_events' term sum - the moments over the step's frames, the factors
 * of the step's block t0 / block, the same lags and bins; n_terms [rows] int64: the step's frames x its contributing bins.
 * |response - exact| <= (n_l + n_s + 72) 2^-53 sum A, n_l = ceil(step frames / 64), n_s = ceil((k_hi - k_lo) / 64).
 * workspace: DEVICE scratch of 32 bytes x rows x (k_hi - k_lo), 8-byte aligned.  Refusals: those of iris_locate_events with
 * rows for segments, and step < 1 or (n_blocks > 1 and block % step != 0) (IRIS_E_INVALID).  Two launches on `stream`, no
 * atomics, fixed summation orders: bitwise reproducible, and a row depends on its own event only.
 *
 * iris_track_lags: response [n_rows, L] (L = 2 max_lag + 1), offsets int32 [n_events + 1] (event e owns the rows offsets[e] ..
 * offsets[e + 1] - 1; once on the device, once on the host: what is checked here), penalty_dev: DEVICE double [n_penalty] =
 * P[d] = d x pen for d = 0 .. min(max_jump, L - 1), formed on the host -> path int32 [n_rows]: per event
 *     D_0[n] = R[0, n];   D_u[n] = max over n' in [max(0, n - max_jump), min(L - 1, n + max_jump)] of (D_{u-1}[n'] - P[|n - n'|]) + R[u, n]
 * the maximiser the smallest such n'; the last row takes the smallest argmax of D, earlier rows follow the back-pointers.  Only
 * subtractions, additions and comparisons of doubles: a host loop with the same operations gives the same integers.
 * workspace: DEVICE scratch of 4 bytes x n_rows x L (the back-pointers).  Refused before any HIP call: a NULL plan, negative
 * counts, n_penalty != min(max_jump, L - 1) + 1, NULL or misaligned arrays (8 bytes: response, penalty; 4: the rest), offsets
 * that do not start at 0, do not strictly ascend or do not end at n_rows (IRIS_E_INVALID); more than 2049 lags (max_lag > 1024:
 * two rows of doubles in LDS; IRIS_E_UNSUPPORTED); a workspace that is too small (IRIS_E_CAPACITY).  n_events == 0 returns
 * IRIS_OK without a launch.  One launch on `stream`, one workgroup per event, no atomics.
 *
 * iris_beamform_frames: iris_beamform_events with one delay per OUTPUT FRAME: tdoa_dev [n_tdoa] double, frame t of event e
 * reads tdoa_dev[first output frame + (t - first)]; a frame whose delay is not finite is exactly 0.  n_tdoa must be the frames
 * of all events (IRIS_E_INVALID); the grid holds n_bins x ceil(longest event / 64) <= 262140 (IRIS_E_UNSUPPORTED); otherwise
 * iris_beamform_events' checks, bound (6 x 2^-24 A) and properties.  A delay that is constant over an event gives the bits of
 * iris_beamform_events.
 */
int iris_locate_steps(iris_plan* plan, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                      const int32_t* events_host, int n_events, int batch, int n_frames, int block, int step, int k_lo, int k_hi,
                      int max_lag, int q, double* workspace, size_t workspace_bytes, double* response, int64_t* n_terms,
                      void* stream);
int iris_track_lags(iris_plan* plan, const double* response, const int32_t* offsets_dev, const int32_t* offsets_host,
                    int n_events, int n_rows, int max_lag, const double* penalty_dev, int n_penalty, int max_jump,
                    int32_t* workspace, size_t workspace_bytes, int32_t* path, void* stream);
int iris_beamform_frames(iris_plan* plan, const float* spec, const float* factors, int n_blocks, const int32_t* events_dev,
                         const int32_t* events_host, const double* tdoa_dev, size_t n_tdoa, int n_events, int batch,
                         int n_frames, int block, int k_lo, int k_hi, float* out, size_t out_floats, void* stream);

/*
 * The Wiener post-filter of event extraction (k_postfilter.h): a decision-directed single-channel gain on the beamformer's
 * output, its noise power taken in closed form from the factors of a covariance that is free of the event (noise="quiet").
 * slabs: the device buffer iris_beamform_events / iris_beamform_frames wrote for the SAME events table, delays, factors,
 * block, bins and plan; out: a buffer of the same layout, at least 2 n_bins x (frames of all events) floats.  per_frame != 0:
 * tdoa_dev holds n_tdoa = the frames of all events delays, one per output frame; else n_tdoa = n_events.  gmin_dev /
 * gmin_host: one gain floor per event, double, in (0, 1], on the device and the host's copy that is checked here.
 * For bin k in [k_lo, k_hi), frame t of event e, block j = t / block, (a, b, c) = factors[sample, k, j], and e_k, s1, den, g0, g1
 * as iris_beamform_events defines them, kept in double:
 *     S = 1/a^2 + |c|^2/a^2 + 1/b^2,  d = loading S / (2 (1 + loading)),  phi = max(1/den - d (|g0|^2 + |g1|^2), 1e-3 / den)
 *     gamma = |Y|^2 / phi;  gamma = 0 where a == 0 or the delay is not finite
 * and along the event's frames, p = 1 before the first:
 *     xi = alpha p + (1 - alpha) max(gamma - 1, 0),  G = max(xi / (1 + xi), g_min[e]),  p = G^2 gamma,  Z = fl32(G) Y
 * Bins outside [k_lo, k_hi) are written as exact zeros and not read; g_min = 1 returns Y bit for bit.  Per real component
 * |Z - exact| <= 3 x 2^-24 |G| |Y| against the float64 definition from the same fp32 inputs.  The same inputs give the same
 * bits; an event's result depends on its own slab, record, delays and floor only.  One launch on `stream` (a workgroup per
 * (event, 64 bins), 33 280 bytes of LDS), no atomics, no workspace.
 * Refused before any launch: NULL plan or factors (there is no identity noise model), batch or n_frames < 1, n_events < 0, an
 * empty bin range or one outside [0, n_bins], alpha outside [0, 1), a loading that is not positive and finite, block < 1,
 * n_blocks != ceil(n_frames / min(block, n_frames)), NULL or misaligned arrays (16 bytes: factors; 8: slabs, out, tdoa, g_min;
 * 4: events), a record that does not fit or does not start at the running frame count, a floor outside (0, 1], a delay count
 * that fits neither form (IRIS_E_INVALID); a plan of other than 2 channels, more than 2^31 - 1 output frames, 2^24 events
 * (IRIS_E_UNSUPPORTED); an `out` that is too small (IRIS_E_CAPACITY).  n_events == 0 returns IRIS_OK without a launch.
 */
int iris_postfilter_events(iris_plan* plan, const float* slabs, const float* factors, int n_blocks, const int32_t* events_dev,
                           const int32_t* events_host, const double* tdoa_dev, size_t n_tdoa, int per_frame,
                           const double* gmin_dev, const double* gmin_host, int n_events, int batch, int n_frames, int block,
                           double loading, double alpha, int k_lo, int k_hi, float* out, size_t out_floats, void* stream);

/*
 * minmax + log_on_mel (data_utils.py:37-55; fused twin trainer.py:63-77),
 * in place on x[n_rows, row_len]: per row (x - min) / max(max - min, eps_div)
 * when do_minmax, then ln(x + eps_log) when do_log.  A batched [B,M,T,C] tensor
 * is n_rows = B; the unbatched [M,T,C] call of metrics.py:53 is n_rows = M
 * (the reference reduces "every axis except 0").
 * workspace: DEVICE scratch of iris_minmax_log_workspace(n_rows, row_len)
 * floats (may be NULL when !do_minmax).  Runs on the current HIP device.
 */
size_t iris_minmax_log_workspace(int n_rows, size_t row_len);
int iris_minmax_log(float* x, int n_rows, size_t row_len, int do_minmax, int do_log, float eps_div,
                    float eps_log, float* workspace, size_t workspace_floats, void* stream);

/*
 * Per-channel energy normalisation (PCEN; Wang et al. 2017, Lostanlen et al. 2019), an opt-in alternative to
 * min-max + log.  mel >= 0 viewed as [n_rows, n_time, n_inner] (a row's n_time * n_inner floats contiguous): the batched
 * [B, M, T, C] tensor is n_rows = B M, the unbatched [M, T, C] one n_rows = M.  Per (row, inner) sequence, along time:
 *     M[0] = E[0],  M[t] = (1 - s) M[t-1] + s E[t]
 *     out  = d^r expm1(r log1p(E exp(-a (log eps + log1p(M / eps))) / d))   = (E / (eps + M)^a + d)^r - d^r
 * with s = smooth, a = gain, d = bias, r = power.  Accepted: 0 < s <= 1, a >= 0, d > 0, 0 < r <= 1, eps > 0, all finite
 * (IRIS_E_INVALID otherwise, checked before any HIP call).  E == 0 gives exactly 0; a NaN propagates forward in time
 * along its sequence only.  out == mel (in place) is allowed, any other overlap is refused.  Any n_time (no length cap),
 * n_inner up to 65535 * 256.  One launch, no workspace, deterministic (the same inputs give the same bits), capturable.
 * iris_pcen_smoother writes the smoother M itself.  Runs on the current HIP device.
 */
int iris_pcen(const float* mel, float* out, int n_rows, int n_time, int n_inner, float smooth, float gain, float bias,
              float power, float eps, void* stream);
int iris_pcen_smoother(const float* mel, float* m_out, int n_rows, int n_time, int n_inner, float smooth, void* stream);

/*
 * PCEN with its own parameters per band, and their gradient: the two halves of the trainable PCEN layer (model.PCEN).
 * The view [n_rows, n_time, n_inner] is iris_pcen's; row i belongs to band i % n_bands (the batched [B, M, T, C] tensor:
 * n_rows = B M, n_bands = M; the unbatched [M, T, C] one: n_rows = n_bands = M) and params is a DEVICE array
 * params[4][n_bands] of the EFFECTIVE values s (0 < s <= 1), a (>= 0), d (> 0), r (0 < r <= 1), in this order.  The
 * per-band constants (1 - s, ln d, d^r) are formed on the device.  The values cannot be range-checked here without a
 * synchronisation: the caller guarantees them (model.PCEN maps unconstrained parameters through exp / sigmoid).  eps is a
 * host scalar as in iris_pcen.  Checked before any HIP call (IRIS_E_INVALID): NULL pointers, non-positive shape,
 * n_bands <= 0, n_rows % n_bands != 0, eps; IRIS_E_CAPACITY: workspace too small.
 *
 * iris_pcen_banded: the same definition, scan, zero / NaN semantics and in-place rule as iris_pcen; one launch.
 *
 * iris_pcen_banded_grad: dparams[4][n_bands] = sum over a band's elements of dout * d out / d (s, a, d, r), the gradient
 * of a scalar loss whose gradient with respect to the output is dout (same shape as mel).  The smoother and its
 * sensitivity dM / ds are recomputed from mel by a forward scan (nothing is saved by the forward; mel is data, so no
 * gradient with respect to it is produced).  Two launches: per-workgroup partial sums into `workspace`
 * (iris_pcen_banded_grad_workspace(n_rows, n_time, n_inner) floats, DEVICE), then their sum per band in a fixed order.
 * No atomics: bitwise reproducible.  Both enqueue on `stream`, allocate nothing, never synchronise: capturable.
 */
int iris_pcen_banded(const float* mel, float* out, int n_rows, int n_time, int n_inner, const float* params, int n_bands,
                     float eps, void* stream);
size_t iris_pcen_banded_grad_workspace(int n_rows, int n_time, int n_inner);
int iris_pcen_banded_grad(const float* mel, const float* dout, int n_rows, int n_time, int n_inner, const float* params,
                          int n_bands, float eps, float* dparams, float* workspace, size_t workspace_floats, void* stream);

/*
 * The fused hot path: [normalize ->] STFT -> magnitude -> band masks -> mel
 * [-> min-max] [-> log] without materialising the spectrum
 * (load_wav data_utils.py:22-23 + sj_train.py:108-123).  flags = IRIS_F_*.
 * One launch on `stream` (min-max / log inside the fused kernel, IRIS_EPILOGUE_FUSED) or two (the fused kernel, then
 * min-max / log over its per-wave partials) - see iris_plan_set_epilogue.  Partials and exchange slots live in the
 * plan's own workspace, so calls on ONE plan must be ordered on one stream (or otherwise serialised) - create one
 * plan per stream to run batches concurrently.  Safe under hipGraph capture and replay: a call made during capture
 * takes the two-kernel path, which keeps no per-call host state and has no atomics to reset.
 */
int iris_wav_to_logmel(iris_plan* plan, const float* wav, float* out, int batch, int len,
                       int flags, const int32_t* t_bands, int n_t_bands,
                       const int32_t* f_bands, int n_f_bands, void* stream);

/*
 * FilterAugment (Nam, Kim, Park, ICASSP 2022) inside the hot path: iris_wav_to_logmel / iris_magmel with every finished mel
 * value multiplied by a per-sample, per-band gain, mel'[b, m, t, c] = fl(mel_gain[b, m] * mel[b, m, t, c]) - ONE separately
 * rounded fp32 multiply, applied BEFORE the min / max reduction and the log (with IRIS_F_MINMAX and IRIS_F_LOG off the result
 * is bitwise mel_gain * the ungained result).  mel_gain: DEVICE fp32 [batch, n_mel], read at launch time (a captured call
 * re-reads it at every replay); all channels of a sample share its row.  Everything else - arguments, forms, epilogues,
 * capture - is as for the ungained entry, which these siblings leave untouched: the gain is a compile-time variant of the
 * kernels, not a branch in them.  (A plan set to IRIS_EPILOGUE_IN_PLACE runs a gained call on two kernels.)
 * IRIS_E_INVALID before any HIP call for a NULL mel_gain.
 */
int iris_wav_to_logmel_gain(iris_plan* plan, const float* wav, float* out, int batch, int len,
                            int flags, const int32_t* t_bands, int n_t_bands,
                            const int32_t* f_bands, int n_f_bands, const float* mel_gain, void* stream);
int iris_magmel_gain(iris_plan* plan, const float* spec, float* mel, int batch, int n_frames,
                     int is_magphase, const int32_t* t_bands, int n_t_bands,
                     const int32_t* f_bands, int n_f_bands, const float* mel_gain, void* stream);

/*
 * mask apply (transforms.py:12-40, deterministic part): x viewed as
 * [n_outer, axis_len, n_inner]; elements whose axis index falls in any band
 * [offset_i, offset_i + size_i) are set to zero (= multiply by the product of
 * the 0/1 masks, in x's dtype).  bands: DEVICE int32 [n_groups, n_bands, 2];
 * outer index o uses group o / outer_per_group (one group per sample).
 * elem_size 4 or 8 bytes (float32/int32 or float64/int64).  In place.
 */
int iris_mask_apply(void* x, size_t n_outer, size_t axis_len, size_t n_inner, int elem_size,
                    const int32_t* bands, int n_bands, size_t outer_per_group, void* stream);

/*
 * adaptive_clip_grad (sj_train.py:145-155 with unitwise_norm, utils.py:350-366) followed by the
 * optimiser's element-wise clipvalue (sj_train.py:435), in place on the gradients, one launch for
 * the whole model.  rows: DEVICE array, one record per output unit (a row of a Linear / LSTM
 * weight, an output channel of a conv kernel, or a whole 1-D tensor): for each row
 *     max_norm = max(||param||, eps) * clip_factor
 *     grad    *= max_norm / max(||grad||, 1e-6)      where ||grad|| >= max_norm
 *     grad     = clamp(grad, -clipvalue, +clipvalue)  when clipvalue > 0
 * A NaN anywhere in a row's gradient makes that whole row NaN, as torch.clamp / tf.maximum do (neither max nor the clamp drops it);
 * other rows are untouched by it.
 * Runs on the current HIP device.
 */
typedef struct {
    const float* param; /* first element of the row, contiguous */
    float* grad;
    int64_t len;
} iris_agc_row;
int iris_agc_clip(const iris_agc_row* rows_dev, size_t n_rows, float clip_factor, float eps,
                  float clipvalue, void* stream);

/*
 * The same launch carrying on into the optimiser (round 6): AGC + clipvalue + the Adam update of sj_train.py:434-435 / :176-182 in
 * one pass over parameters, gradients and both moments (torch.optim.Adam's arithmetic, no weight decay / amsgrad; the clipped
 * gradient is written back to `grad`).  use_agc == 0: clipvalue + Adam only.  lr_dev: nullable DEVICE float (a capturable
 * optimiser's learning-rate tensor), else lr_host; step_dev: DEVICE float holding the step count t >= 1 of THIS update (the
 * optimiser's already incremented counter).  Rows as for iris_agc_clip, plus the two moment rows in the parameter's own layout.
 */
typedef struct {
    float* param;
    float* grad;
    int64_t len;
    float* exp_avg;
    float* exp_avg_sq;
} iris_agc_adam_row;
int iris_agc_clip_adam(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                       int use_agc, const float* lr_dev, float lr_host, double beta1, double beta2, float eps,
                       const float* step_dev, void* stream);

/*
 * The same launch once more, carrying on into an exponential moving average of the weights (model EMA / mean teacher): after
 * p' = p - step m' / denom, still in its register,
 *     d_t = min(decay, (1 + t) / (10 + t))        in double; t = step_dev[0], the counter the bias corrections read
 *     e'  = e + (p' - e) (float)(1 - d_t)          fp32, written back to `ema`
 * (TensorFlow's ExponentialMovingAverage(num_updates) warm-up; formed on the device, so a replayed hipGraph sees every step).
 * decay in [0, 1).  Rows as for iris_agc_clip_adam plus `ema`, a contiguous row in the parameter's own layout; the float4 path
 * runs where all FIVE pointers are 16-byte aligned and 4 | len, the scalar path elsewhere.  param, grad and both moments come out
 * bit for bit as from iris_agc_clip_adam.  A NaN in p' goes into e' (the parameter is lost at that point anyway).
 */
typedef struct {
    float* param;
    float* grad;
    int64_t len;
    float* exp_avg;
    float* exp_avg_sq;
    float* ema;
} iris_agc_adam_ema_row;
int iris_agc_clip_adam_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                           int use_agc, const float* lr_dev, float lr_host, double beta1, double beta2, float eps,
                           const float* step_dev, double decay, void* stream);

/*
 * The siblings of iris_agc_clip_adam for the other two optimisers of sj_train.py:436-439: AGC + clipvalue exactly as above (x, the
 * clipped gradient, is written back to `grad`), then
 *     sgd      b' = mu b + x;                                                  p' = p - lr b'
 *     rmsprop  s' = alpha s + (float)(1 - alpha) x x;  b' = mu b + x / (sqrtf(s') + eps);  p' = p - lr b'
 * torch.optim.SGD (momentum, no dampening / nesterov / weight decay) and torch.optim.RMSprop (momentum, not centered, no weight
 * decay) in fp32; a zero momentum buffer gives torch's first step.  The rows are iris_agc_adam_row / iris_agc_adam_ema_row with the
 * momentum buffer in `exp_avg` and rmsprop's square average in `exp_avg_sq`; the sgd entry points never read the `exp_avg_sq`
 * slot (it may hold anything).  mu, alpha in [0, 1), eps >= 0; lr_dev: nullable DEVICE float, else lr_host.  Neither update has a
 * bias correction: only the _ema siblings take a counter - step_dev, a DEVICE float holding t >= 1 of THIS update - for
 *     e' = e + (p' - e) (float)(1 - min(decay, (1 + t) / (10 + t)))            decay in [0, 1)
 * The float4 path runs where 4 | len and every pointer the entry point reads is 16-byte aligned.  Arguments are checked before any
 * HIP call; n_rows == 0 returns IRIS_OK; nothing is allocated or synchronised, the launch goes to `stream`.
 */
int iris_agc_clip_sgd(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                      int use_agc, const float* lr_dev, float lr_host, double mu, void* stream);
int iris_agc_clip_sgd_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                          int use_agc, const float* lr_dev, float lr_host, double mu, const float* step_dev, double decay,
                          void* stream);
int iris_agc_clip_rmsprop(const iris_agc_adam_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                          int use_agc, const float* lr_dev, float lr_host, double mu, double alpha, float eps, void* stream);
int iris_agc_clip_rmsprop_ema(const iris_agc_adam_ema_row* rows_dev, size_t n_rows, float clip_factor, float eps_agc, float clipvalue,
                              int use_agc, const float* lr_dev, float lr_host, double mu, double alpha, float eps,
                              const float* step_dev, double decay, void* stream);

/*
 * The reference's training metrics of one batch (metrics.py:217-299) in ONE launch, capturable:
 *   y_true [B, T, K], y_pred [B, T', K] fp32 contiguous; 1 <= K <= 16, 1 <= T, T' <= 8192, B >= 1.
 *   er_out   [B]  er_score per clip: yt = y_true >= threshold, yp = y_pred >= threshold (after AveragePooling1D(pool,
 *                 padding='same', stride = pool) when pool > 1: T' -> ceil(T' / pool) windows, each the mean of its in-range
 *                 frames); runs are maximal 1-runs per (clip, class); a true run [ts, te] is correct iff a predicted run of the
 *                 same clip and class has its middle (s + e) / 2 in [ts, te] (middles compared as indices with label frames);
 *                 er = (n_true + n_pred - 2 correct) / max(n_true, 1) in fp32.
 *   cos_out  [B]  nullable; cos_sim per clip (Keras' negative cosine over time, classes weighted by the mask sum_t y_true > 0).
 *   f1_state [3]  nullable, DEVICE fp64 (tp, fp, fn), CUMULATIVE: the batch's sum p y, p (1 - y), (1 - p) y with p = y_pred >
 *                 f1_threshold is added; f1_out [1] (with f1_state) = micro F1 of the cumulative counts (div-no-nan).
 *   accum    [5]  nullable, DEVICE fp64: += (sum er, sum cos, f1_out, B, 1) - an epoch accumulator the caller zeroes.
 *   cos_out and f1_state need T' == T.  With f1_state or accum: slab [3 B] fp64 workspace and ticket [1] uint32, zero before
 *   the first launch (the kernel leaves it zero); one (slab, ticket) pair per stream.  Deterministic: the same inputs give the
 *   same bits, no float atomics.
 */
int iris_event_metrics(const float* y_true, const float* y_pred, int batch, int n_time, int n_time_pred, int n_classes,
                       float threshold, int pool, float f1_threshold, float* er_out, float* cos_out, double* f1_state,
                       float* f1_out, double* accum, double* slab, unsigned int* ticket, void* stream);

/*
 * Score histogram of one batch per (class, label), ONE launch on `stream`, capturable; the primitive behind the threshold-free
 * validation numbers (ROC-AUC, average precision, best-F1 threshold, calibration error: host arithmetic on the counts).
 *   y_true, y_pred [B, T, K] fp32 contiguous, at the same frame rate; 1 <= K <= 16, B * T <= 2^31 - 1.
 *   bins     a power of two in [16, 4096].
 *   counts   [K][2][bins + 1] int64, DEVICE, CUMULATIVE (the caller zeroes it): counts[k][label][slot] += 1 per frame with
 *            label = y_true >= 0.5f (a NaN label is negative; labels above 1 are positive) and, for a prediction p,
 *            slot = min(bins - 1, max(0, (int)floorf(p * bins))) - p <= 0, -0.0, subnormals and -inf: 0; p >= 1 and +inf:
 *            bins - 1 - or slot = bins for a NaN prediction (kept, never folded into a bin).  p * bins is exact in fp32, so
 *            "slot >= b" is the predicate p >= b / bins.
 * Integer adds only: independent of the order, bitwise reproducible, and the counts of several ranks sum exactly.
 * Refused before any HIP call: NULL pointers, B / T / K < 1 (INVALID); K > 16, bins not a power of two in range,
 * B * T > 2^31 - 1 (UNSUPPORTED).
 */
int iris_score_hist(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes, int bins,
                    long long* counts, void* stream);

/*
 * Segment- and event-based detection counts of one batch (Mesaros, Heittola & Virtanen 2016: the measures sed_eval reports) at
 * n_thr thresholds, TWO launches on `stream`, capturable, no host synchronisation and no allocation; ratios are host arithmetic.
 *   y_true, y_pred [B, T, K] fp32 contiguous, DEVICE, at the same frame rate; 1 <= K <= 16, T <= 2^20, B * T <= 2^31 - 1.
 *   thresholds     [n_thr] fp32, HOST, finite and strictly increasing, 1 <= n_thr <= 16 (read before the launches).
 *   Label activity is y_true >= 0.5f, predicted activity at threshold h is y_pred >= h in fp32; a NaN is inactive.
 *   Segments: frame f of a clip lies in segment (f * hop) / seg_samples (segments restart with every clip; a partial last one
 *     counts); a class is active in a segment if any of its frames is.  Per (threshold, class) tp / fp / fn over all segments;
 *     per (threshold, segment) with Nfn / Nfp the classes active in the labels / the prediction only: S = min(Nfn, Nfp),
 *     D = max(0, Nfn - Nfp), I = max(0, Nfp - Nfn).
 *   Events: maximal runs [s, e] of active frames of one (clip, class) row (a run open at the end closes at T - 1); onset s * hop,
 *     offset (e + 1) * hop, length (e + 1 - s) * hop samples, 64-bit.  A predicted event p may match a reference event r of its
 *     row if |on_p - on_r| <= collar_samples and 100 |off_p - off_r| <= max(100 collar_samples, offset_pct * len_r).  Reference
 *     events in time order each take the earliest still free predicted event that may match them (greedy, not an optimal
 *     assignment).  ev_tp the matches, ev_fp = n_pred - ev_tp, ev_fn = n_ref - ev_tp; classes are scored independently.
 *   counts         [n_thr][K + 1][6] int64, DEVICE, CUMULATIVE (the caller zeroes it): rows k < K hold (seg_tp, seg_fp, seg_fn,
 *                  ev_tp, ev_fp, ev_fn), row K holds (S, D, I, n_segments, 0, 0).
 *   workspace      DEVICE, 4-byte aligned, at least iris_sed_workspace_bytes(...) bytes (0 for a shape that is refused); its
 *                  contents are scratch, rewritten by every call: calls that share one must be ordered on one stream.
 * Integer adds only: independent of the order, bitwise reproducible, and the counts of several ranks sum exactly.
 * Refused before any HIP call: NULL pointers, B / T / K < 1, n_thr outside [1, 16], thresholds not finite or not increasing,
 * hop < 1, seg_samples < hop, collar_samples < 0, offset_pct outside [0, 100], a misaligned or too small workspace (INVALID);
 * K > 16, T > 2^20, B * T > 2^31 - 1 (UNSUPPORTED).
 */
long long iris_sed_workspace_bytes(int batch, int n_time, int n_classes, int n_thr, int hop, int seg_samples);
int iris_sed_counts(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes, const float* thresholds,
                    int n_thr, int hop, int seg_samples, int collar_samples, int offset_pct, void* workspace,
                    size_t workspace_bytes, long long* counts, void* stream);

/*
 * Intersection-based detection counts of one batch behind the polyphonic sound detection score (PSDS: Bilen et al., ICASSP 2020)
 * at n_thr thresholds, TWO launches on `stream`, capturable, no host synchronisation and no allocation; the rates, the curves and
 * the area are host arithmetic.  All arithmetic is integer; products are formed in 64 bits.
 *   y_true, y_pred [B, T, K] fp32 contiguous, DEVICE, at the same frame rate; 1 <= K <= 16, T <= 2^20, B * T <= 2^31 - 1.
 *   thresholds     [n_thr] fp32, HOST, finite and strictly increasing, 1 <= n_thr <= 64 (read before the launches).
 *   dtc_pct, gtc_pct in [1, 100]; cttc_pct in [1, 100], or 0 for none (no cross-triggers are counted).
 *   Label activity is y_true >= 0.5f, predicted activity at threshold h is y_pred >= h in fp32; a NaN is inactive.
 *   Events are the maximal runs [s, e) of active frames of one (clip, class) row; a run open at the row's end closes at T; the
 *     length is e - s frames.  Events are not joined across calls.
 *   For clip b, threshold j, class c and a detection d (a run of class c at h_j) let I_k(d) be the number of frames of d in
 *     which label k of that clip is active (the sum of |d ∩ g| over the ground-truth events g of class k).
 *     d PASSES if 100 I_c(d) >= dtc_pct len(d).  Otherwise FP[j][c] += 1, and for every class k != c, if cttc_pct is given and
 *     100 I_k(d) >= cttc_pct len(d), CT[j][c][k] += 1 (a failing detection is a false positive whether or not it is also a
 *     cross-trigger).  n_det[j][c] counts every detection.
 *     A ground-truth event g of class c is a true positive at j, TP[j][c] += 1, if 100 cov(g) >= gtc_pct len(g), cov(g) being
 *     the number of frames of g inside passing detections of class c at h_j in that clip.
 *   counts         [n_thr + 1][K][K + 2] int64, DEVICE, CUMULATIVE (the caller zeroes it).
 *                  Plane j < n_thr, row c: column c holds TP[j][c], column k != c (k < K) holds CT[j][c][k], column K holds
 *                  FP[j][c], column K + 1 holds n_det[j][c].
 *                  Plane n_thr, the threshold-independent totals: row k holds n_gt[k] (ground-truth events) in column 0 and
 *                  gt_frames[k] (active label frames) in column 1; row 0 holds n_frames (B * T summed over the calls) in column
 *                  K - for K = 1, where that is the gt_frames column, in column 2.  Every other entry of the plane stays 0.
 *   workspace      DEVICE, 8-byte aligned, at least iris_psds_workspace_bytes(...) bytes (0 for a shape that is refused); its
 *                  contents are scratch, rewritten by every call: calls that share one must be ordered on one stream.
 * Integer adds only: independent of the order, bitwise reproducible, and the counts of several ranks sum exactly.
 * Refused before any HIP call: NULL pointers, B / T / K / n_thr < 1, thresholds not finite or not increasing, dtc_pct or gtc_pct
 * outside [1, 100], cttc_pct outside [0, 100], a misaligned or too small workspace (INVALID); K > 16, n_thr > 64, T > 2^20,
 * B * T > 2^31 - 1 (UNSUPPORTED).
 */
long long iris_psds_workspace_bytes(int batch, int n_time, int n_classes, int n_thr);
int iris_psds_counts(const float* y_true, const float* y_pred, int batch, int n_time, int n_classes, const float* thresholds,
                     int n_thr, int dtc_pct, int gtc_pct, int cttc_pct /* 0: none */, void* workspace, size_t workspace_bytes,
                     long long* counts, void* stream);

/*
 * Window predictions of F files -> event lists (metrics.py:56-81 from the model's outputs on, then get_start_end_frame,
 * metrics.py:111-137), two launches, capturable:
 *   preds      [W_total, n_out, K] fp32, DEVICE: the model's outputs for every window of every file, file after file
 *   win_off    [F + 1] int32, DEVICE: file f owns windows win_off[f] .. win_off[f + 1] - 1
 *   frame_len  [F] int32, DEVICE: T_f, the file's STFT frames
 *   win_off_host, frame_len_host: the same values in host memory (checked here; they size the grid)
 * For file f, class k, frame t < T_f, with up = n_frame / n_out and 'same' pads al = (avg_pool - 1) / 2, ar = avg_pool - 1 - al
 * (ml, mr likewise for max_pool):
 *   p[t] = fp32 sum from 0, in ascending w over the windows with w * hop <= t < w * hop + n_frame, of
 *          preds[win_off[f] + w, (t - w * hop) / up, k], divided by (float) their count
 *   a[t] = fp32 sum from 0 of p[u], u in [t - al, t + ar] ∩ [0, T_f) ascending, divided by (float) the frames in range
 *   d[t] = some u in [t - ml, t + mr] ∩ [0, T_f) has a[u] >= threshold and none of them has a NaN a[u]
 *   events: the maximal runs of d as (first, last) frame pairs
 * Outputs (DEVICE):
 *   n_ev  [F, K] int32 event counts
 *   ev    int32 (first, last) pairs; (file f, class k) owns cap_f = ceil(T_f / 2) + 1 pairs starting at pair
 *         K * sum_{g < f} cap_g + k * cap_f, of which the first n_ev[f, k] are written, in time order
 *   bits  workspace of K * sum_f ceil(T_f / 64) uint64 words
 * 1 <= K <= 16, 1 <= avg_pool <= 127, 1 <= max_pool <= 256 (IRIS_E_UNSUPPORTED otherwise); IRIS_E_INVALID for
 * overlap_hop > n_frame, n_frame % n_out != 0, negative T_f, or T_f > (windows_f - 1) * overlap_hop + n_frame (frames no window
 * covers).  Deterministic: plain stores, no atomics; the same inputs give the same bits.
 * iris_decode_sweep below runs this decoder at every point of a grid of settings and scores each against ground truth.
 */
int iris_decode_events(const float* preds, const int* win_off, const int* frame_len, const int* win_off_host,
                       const int* frame_len_host, int n_files, int n_frame, int overlap_hop, int n_out, int n_classes,
                       int avg_pool, int max_pool, float threshold, unsigned long long* bits, int* ev, int* n_ev,
                       void* stream);

/*
 * The decoder above at G settings at once, scored against ground truth (metrics.output_to_metric + the per-class terms of
 * metrics.get_er), two launches whatever G and F are, capturable:
 *   preds, win_off, frame_len, win_off_host, frame_len_host, n_files, n_frame, overlap_hop, n_out, n_classes: as above
 *   threshold [G] fp32, avg_pool [G] int32, max_pool [G] int32, DEVICE: the grid.  It must be SORTED so that equal avg_pool
 *         values are adjacent and, among them, equal thresholds (compared as bit patterns) are adjacent; the *_host arrays hold
 *         the same values in host memory (checked here, IRIS_E_INVALID if the order is not kept)
 *   gt    [rows, 2] int32 (start_s, end_s), DEVICE: the ground-truth events grouped by (file, class); (file f, class k) owns
 *         rows gt_off[f K + k] .. gt_off[f K + k + 1] - 1, sorted by start_s (stable).  gt_off [F K + 1] int32 DEVICE,
 *         gt_off_host the same in host memory
 *   metric_hop, sample_rate: an event (s, e) in frames becomes the second (int)((((double)(s + e)) / 2) * metric_hop /
 *         sample_rate) - output_to_metric's expression, left to right in fp64
 *   p_ws  workspace of K * sum_f T_f floats (the overlap-add average p, which no setting changes)
 * Outputs (DEVICE, int32, every element written):
 *   n_pred  [G, F, K]  the number of events iris_decode_events yields with setting g (the same fp32 summation orders for p and
 *                      a, the same >= and NaN rules)
 *   matched [G, F, K]  get_er's greedy rule within the class: the ground-truth rows in order; each takes the first prediction
 *                      not yet taken, in time order, whose second lies in [start_s, end_s]
 * so that get_er of file f at one setting per class is sum_k (n_pred + n_gt - 2 matched) / sum_k n_gt.
 * Limits (IRIS_E_UNSUPPORTED, nothing is launched or written): 1 <= K <= 16; per grid point 1 <= avg_pool <= 127 and
 * 1 <= max_pool <= 256; G <= 4096; at most 256 distinct thresholds share one avg_pool; (distinct thresholds of one avg_pool + 1)
 * * ceil(max_f T_f / 64) <= 6144 (the threshold bit words of one (file, class, avg_pool) are held in LDS: 17 thresholds allow
 * 21,824 frames, a file of 1,900 frames 203 thresholds); at most 64 ground-truth rows per (file, class) (one per lane); F <= 65535;
 * K * sum_f T_f <= 2^31 - 1 (the workspace index) and G * F * K <= 2^31 - 1 (the output index).
 * IRIS_E_INVALID as for iris_decode_events.  Deterministic: integer outputs, plain stores, no atomics.
 */
int iris_decode_sweep(const float* preds, const int* win_off, const int* frame_len, const int* win_off_host,
                      const int* frame_len_host, int n_files, int n_frame, int overlap_hop, int n_out, int n_classes,
                      const float* threshold, const int* avg_pool, const int* max_pool, const float* threshold_host,
                      const int* avg_pool_host, const int* max_pool_host, int n_grid, const int* gt, const int* gt_off,
                      const int* gt_off_host, int metric_hop, int sample_rate, float* p_ws, int* n_pred, int* matched,
                      void* stream);

/*
 * The other decoder for the same window predictions: a two-state (off / on) HMM per class, decoded with Viterbi on integer
 * scores.  Where iris_decode_events widens and merges by a fixed morphological rule, this one keeps an event only if its
 * accumulated log-odds pay the class's event cost, and bridges a gap only if the gap's evidence against the event is weaker than
 * the price of a second event.  Opt-in; two launches, capturable.
 *   preds, win_off, frame_len, win_off_host, frame_len_host, n_files, n_frame, overlap_hop, n_out, n_classes, bits, ev, n_ev: as
 *         for iris_decode_events (the same layouts of bits, ev and n_ev)
 *   lut   [1024] int32, DEVICE: the score of each probability bucket, entries in [-2^15, 2^15].  The default table is
 *         lut[i] = rint(256 ln(c / (1 - c))), c = (i + 0.5) / 1024, computed by the caller in float64: log-odds in units of
 *         1/256 nat, in [-1952, 1952], lut[511] = -1, lut[512] = 1.  The device evaluates no logarithm
 *   bias  [K] int32, HOST: rint(256 ln(thr / (1 - thr))) of the class's threshold thr in (0, 1); 0 at 0.5; |bias| <= 2^20
 *   cost  [K] int32, HOST: the class's event cost C in [0, 2^19], rint(256 * nats)
 *   work  workspace of iris_decode_hmm_workspace_len = 2 K sum_f ceil(T_f / 64) uint64 words (the back-pointers), DEVICE
 * For file f, class k, frame t < T_f:
 *   1. p[t]: the overlap-add average of iris_decode_events (the same fp32 summation order)
 *   2. e[t], int32: b = clamp(floor(p[t] * 1024.0f), 0, 1023) - the multiply is exact in fp32; values below 0, above 1 and
 *      +-inf clamp - and e[t] = lut[b] - bias[k]; a NaN p[t] gives e[t] = -2^20
 *   3. Viterbi, int64: V0 = 0, V1 = -2^60; for t = 0 .. T_f - 1, from the values before frame t,
 *         b0[t] = (V1 > V0),  b1[t] = !(V0 - C > V1),  then  V0' = max(V0, V1),  V1' = e[t] + max(V1, V0 - C);
 *      at the end s[T_f - 1] = (V1 > V0) and s[t - 1] = s[t] ? b1[t] : b0[t].  Ties keep the state: stay off, stay on, end off.
 *      s maximises sum_{t: s[t] = 1} e[t] - C * (number of runs of s); since C <= 2^19 < 2^20 a NaN frame is always off
 *   4. events: the maximal runs of s as (first, last) frame pairs
 * No floating point after step 2's bucket.  The kernel cuts time into chunks, one per lane, and combines them with scans of
 * (max, +) 2 x 2 integer matrices and of maps on {0, 1}: both are exactly associative, so the result EQUALS the sequential
 * definition above whatever the order of the scans.  Deterministic: plain stores, no atomics.
 * IRIS_E_INVALID: NULL pointers (lut and work included), a cost outside [0, 2^19], |bias| > 2^20, and what iris_decode_events
 * refuses; IRIS_E_UNSUPPORTED: K > 16.  All refused before any launch.
 */
long long iris_decode_hmm_workspace_len(const int* frame_len_host, int n_files, int n_classes);
int iris_decode_events_hmm(const float* preds, const int* win_off, const int* frame_len, const int* win_off_host,
                           const int* frame_len_host, int n_files, int n_frame, int overlap_hop, int n_out, int n_classes,
                           const int* lut, const int* bias, const int* cost, unsigned long long* work,
                           unsigned long long* bits, int* ev, int* n_ev, void* stream);

/*
 * Inference epilogue of ConvMPBlock's Conv2D + BatchNormalization + ReLU (+ MaxPool2D 2x2 'same'), sj_train.py:191-201,
 * once the eval-mode BatchNorm is folded into the convolution (sj_train.fold_batchnorm): the convolution itself stays
 * MIOpen (PyTorch-ROCm, per north_star); these replace the separate bias-add, ReLU and pooling passes over its output.
 *   iris_bias_relu:          x[o, c] = max(x[o, c] + bias[c], 0) in place on a channels-last tensor [n_outer, channels]
 *   iris_bias_relu_maxpool:  y[b, i, j, c] = max over the 2x2 window (stride 2, clipped at the edges = Keras 'same' /
 *                            ceil mode) of max(x[b, 2i+di, 2j+dj, c] + bias[c], 0);  x [B, H, W, C] -> y [B, ceil(H/2), ceil(W/2), C]
 * channels must be a multiple of 4; x, y, bias DEVICE, 16-byte aligned.  Run on the current HIP device.
 */
int iris_bias_relu(float* x, const float* bias, size_t n_outer, int channels, void* stream);
/* the same on a CONTIGUOUS (NCHW) activation x [batch, channels, inner] (inner = H * W, a multiple of 4), and the pooling
 * variant reading NCHW x [B, C, H, W] and writing the pooled tensor channels-last y [B, ceil(H/2), ceil(W/2), C]: block 1 of
 * the CRNN runs its convolutions in NCHW (MIOpen is faster there for 32 -> 32 channels at 64 x 512) and hands over in NHWC */
int iris_bias_relu_nchw(float* x, const float* bias, size_t batch, int channels, size_t inner, void* stream);
int iris_bias_relu_maxpool_nchw(const float* x, const float* bias, float* y, int batch, int height, int width, int channels,
                                void* stream);
int iris_bias_relu_maxpool(const float* x, const float* bias, float* y, int batch, int height, int width, int channels,
                           void* stream);

/*
 * Training-mode Conv2D bias + BatchNormalization + ReLU of ConvMPBlock (sj_train.py:191-201; Keras BatchNormalization
 * momentum 0.99 / epsilon 1e-3 = torch momentum 0.01) on the channels-last convolution output z [rows = N H W, channels]
 * in two passes each way instead of MIOpen's / ATen's seven forward and nine backward (bias add, mean / variance,
 * normalise, ReLU; ReLU', dscale / dbias, dx, bias gradient).  The convolution stays MIOpen and is run WITHOUT bias:
 * batch normalisation removes the batch mean, so the output does not depend on the bias - it only shifts the running
 * mean (conv_bias, nullable, is added there) - and the bias gradient is identically zero.
 *   forward : iris_bn_stats (sums_zeroed: DEVICE double [iris_bn_sums_len(channels)], zero on entry: per-channel sum and sum
 *             of squares of z - K, K = the channel's value in row 0 of z - shifted sums, so that a channel whose |mean| is
 *             far above its spread keeps its variance; spread over several copies so that the blocks' atomics do not queue
 *             on one address; the consumers below add the copies up and read K back from z)
 *             iris_bn_relu_apply: y = max(gamma (z - mean) rstd + beta, 0), biased variance; running_mean / running_var
 *             updated in place ((1 - momentum) old + momentum new, unbiased variance); save_mean / save_rstd [channels] out
 *   backward: iris_bn_relu_bwd_reduce (sums_zeroed, same length: sum g, sum g xhat with g = dy [y > 0]; the mask is
 *             recomputed from z with the forward's own expression, y is not read)
 *             iris_bn_relu_bwd_dx: dz = gamma rstd (g - sum_g / M - xhat sum_gx / M); dgamma = sum g xhat, dbeta = sum g
 * channels: a multiple of 4, <= 4096; every pointer DEVICE, 16-byte aligned tensors.  Run on the current HIP device.
 * NOT in-place: y (and p below) must not overlap z - every block of the apply passes reads K back from row 0 of z while
 * others write their outputs (IRIS_E_INVALID otherwise).
 */
/* Round 6: the forward statistics can come out of the CONVOLUTION's epilogue instead (iris_conv3x3_wino_bn, iris_conv3x3_wino_b3_bn,
 * iris_conv3x3_c32_bn: the bare convolution + sum z / sum z^2 per output channel into a zeroed [iris_bn_sums_len] buffer, accumulated
 * from the registers z is stored from) - the iris_bn_stats pass over z disappears; the *_sums0 forms of the apply entry points
 * consume sums taken about zero (iris_bn_stats' are taken about row 0 of z).  Replaces the same layers of sj_train.py:191-201.
 * These sums repeat bit for bit from call to call: the buffer holds three exponent windows of the per-channel copies, inside which
 * the kernels' fp64 atomics are exact in any order (the statistics passes use the first window only). */
size_t iris_bn_sums_len(int channels);
int iris_bn_relu_apply_sums0(const float* z, float* y, size_t rows, int channels, const double* sums, const float* gamma,
                             const float* beta, const float* conv_bias, float eps, float momentum, float* running_mean,
                             float* running_var, float* save_mean, float* save_rstd, void* stream);
int iris_bn_relu_pool_apply_sums0(const float* z, float* p, int batch, int height, int width, int channels, const double* sums,
                                  const float* gamma, const float* beta, const float* conv_bias, float eps, float momentum,
                                  float* running_mean, float* running_var, float* save_mean, float* save_rstd, void* stream);
int iris_conv3x3_wino_bn(const float* x, const float* packed, float* y, int batch, int height, int width, int cin, int cout, int flags,
                         double* bn_sums_zeroed, void* stream);
int iris_conv3x3_wino_b3_bn(const float* x, const float* packed, float* y, int batch, int height, int width, int cin, int cout, int flags,
                            double* bn_sums_zeroed, void* stream);
int iris_conv3x3_c32_bn(const float* x, const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, float* y,
                        int batch, int height, int width, double* bn_sums_zeroed, void* stream);

/*
 * All the weight packings of a training step in ONE launch (round 6; replaces N calls of iris_wino_pack_weights_device /
 * iris_wino_b3_pack_weights_device - 23 per step of the CRNN, 0.16 ms of launches and tails).  jobs: HOST array (read during the
 * call, passed to the kernel by value: nothing device-side to keep alive, capturable into a hipGraph); per job the arguments of the
 * single-layer entry points; first_block is filled in by the call.  split_bf16 != 0: the iris_wino_b3 packing (cin % 16 == 0).
 * Any number of jobs (48 per launch).
 */
typedef struct iris_pack_job {
    const float* weight;
    float* packed;
    long stride_o, stride_i, stride_h, stride_w;
    int cin, cout, transposed, first_block;
} iris_pack_job;
int iris_wino_pack_weights_device_multi(iris_pack_job* jobs_host, int n_jobs, int split_bf16, void* stream);
int iris_bn_stats(const float* z, size_t rows, int channels, double* sums_zeroed, void* stream);
int iris_bn_relu_apply(const float* z, float* y, size_t rows, int channels, const double* sums, const float* gamma,
                       const float* beta, const float* conv_bias, float eps, float momentum, float* running_mean,
                       float* running_var, float* save_mean, float* save_rstd, void* stream);
int iris_bn_relu_bwd_reduce(const float* z, const float* dy, size_t rows, int channels, const float* save_mean,
                            const float* save_rstd, const float* gamma, const float* beta, double* sums_zeroed, void* stream);
int iris_bn_relu_bwd_dx(const float* z, const float* dy, float* dz, size_t rows, int channels, const float* save_mean,
                        const float* save_rstd, const float* gamma, const float* beta, const double* sums, float* dgamma,
                        float* dbeta, void* stream);

/*
 * The same passes for the LAST convolution of a ConvMPBlock, with its MaxPool2D(2, 2, 'same') folded in (sj_train.py:199-200:
 * pooling follows the block's last Conv-BN-ReLU): z [batch, height, width, channels] channels-last; p and dp
 * [batch, ceil(height / 2), ceil(width / 2), channels].  The full-size y is never written and the full-size dy never exists:
 *   forward : iris_bn_stats as above (the statistics are those of the full-size z), then
 *             iris_bn_relu_pool_apply: p = max over the window of max(gamma (z - mean) rstd + beta, 0)
 *   backward: iris_bn_relu_pool_bwd_reduce / iris_bn_relu_pool_bwd_dx: g = dp at the window's first maximum in (h, w) scan
 *             order (max_pool2d's index rule) where that maximum is > 0, 0 elsewhere; sums, dz, dgamma, dbeta as above.
 * Same constraints as above.
 */
int iris_bn_relu_pool_apply(const float* z, float* p, int batch, int height, int width, int channels, const double* sums,
                            const float* gamma, const float* beta, const float* conv_bias, float eps, float momentum,
                            float* running_mean, float* running_var, float* save_mean, float* save_rstd, void* stream);
int iris_bn_relu_pool_bwd_reduce(const float* z, const float* dp, int batch, int height, int width, int channels,
                                 const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                 double* sums_zeroed, void* stream);
int iris_bn_relu_pool_bwd_dx(const float* z, const float* dp, float* dz, int batch, int height, int width, int channels,
                             const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                             const double* sums, float* dgamma, float* dbeta, void* stream);

/*
 * Second layer of the CRNN's first block for inference: Conv2D(32 -> 32, 3x3 'same') + (BatchNorm-folded) bias + ReLU, and
 * with pool != 0 the block's MaxPool2D(2, 2, 'same') behind it (sj_train.py:191-201, 244), as an implicit GEMM on the fp32
 * matrix cores (exact fp32).  x [batch, height, width, 32] channels-last, weight [32, 32, 3, 3] contiguous, bias [32];
 * y [batch, height, width, 32] or, pooled, [batch, ceil(height / 2), ceil(width / 2), 32]; with out_chunked != 0 the same
 * values in the channel-chunked layout [batch][4][Ho][Wo][8] that iris_conv3x3_wino_bias_relu reads.  x 16-byte aligned.
 */
int iris_conv3x3_c32_bias_relu(const float* x, const float* weight, const float* bias, float* y, int batch, int height, int width,
                               int pool, int out_chunked, void* stream);
/* The same kernel as the bare convolution of a TRAINING pass (BatchNorm follows: no bias, no ReLU, no pooling): y = conv3x3_same(x, w)
 * with transposed == 0 (forward) or y = conv3x3_same(x, w') with w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx] (transposed != 0:
 * the backward-data pass, x = dz).  x, y channels-last [batch, height, width, 32]; weight [32, 32, 3, 3] with element strides
 * stride_o / _i / _h / _w (a channels_last parameter as it is). */
int iris_conv3x3_c32(const float* x, const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, int transposed,
                     float* y, int batch, int height, int width, void* stream);

/*
 * Conv2D(cin -> cout, 3x3 'same', stride 1) as a Winograd F(2x2, 3x3) transform on the fp32 matrix cores: 16 instead of 36
 * multiplies per 2 x 2 output tile and channel pair - MIOpen's implicit GEMMs already run these layers at the fp32 MFMA rate.
 * Blocks 2-5 of the CRNN (sj_train.py:191-201, 222-242): for inference with the (BatchNorm-folded) bias, ReLU and the block's
 * MaxPool2D(2, 2, 'same') fused; for training as the bare convolution of the deep layers' forward and backward-data passes.
 * fp32 throughout; against an fp64 convolution the error is that of a direct fp32 convolution (<= 1e-6 of the output's peak).
 * cin % 8 == 0, cout % 64 == 0.
 *   x      channel-chunked activation [batch][cin / 8][height][width][8] (8 channels of a pixel contiguous) - or, with
 *          IRIS_WINO_IN_NHWC, channels-last [batch][height][width][cin] (14 % slower: every gather touches 4x the cache lines);
 *          DEVICE, 16-byte aligned, fewer than 2^30 elements
 *   packed U = G g G^T in the kernel's LDS order, 16 cin cout floats (iris_wino_packed_len), DEVICE, 16-byte aligned:
 *          iris_wino_pack_weights (HOST buffers in and out, weight [cout][cin][3][3] contiguous; upload the result once per layer) or
 *          iris_wino_pack_weights_device (DEVICE, on `stream`, weight with arbitrary element strides - a channels_last parameter as
 *          it is -; transposed != 0 packs the weights of the backward-data pass, dx = conv(dz, W') with W'[ci][co][i][j] =
 *          W[co][ci][2 - i][2 - j]: `cin` then counts the original OUTPUT channels)
 *   bias   [cout] or NULL
 *   y      [batch][cout / 8][Ho][Wo][8] - the next layer's x - or, with IRIS_WINO_OUT_NHWC, channels-last [batch][Ho][Wo][cout];
 *          Ho x Wo = height x width, or ceil(height / 2) x ceil(width / 2) with IRIS_WINO_POOL
 *   flags  IRIS_WINO_POOL | IRIS_WINO_OUT_NHWC | IRIS_WINO_IN_NHWC | IRIS_WINO_RELU
 */
enum { IRIS_WINO_POOL = 1, IRIS_WINO_OUT_NHWC = 2, IRIS_WINO_IN_NHWC = 4, IRIS_WINO_RELU = 8 };
size_t iris_wino_packed_len(int cin, int cout);
int iris_wino_pack_weights(const float* weight_host, int cin, int cout, float* packed_host);
int iris_wino_pack_weights_device(const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, int cin, int cout,
                                  int transposed, float* packed, void* stream);
int iris_conv3x3_wino(const float* x, const float* packed, const float* bias, float* y, int batch, int height, int width, int cin,
                      int cout, int flags, void* stream);

/*
 * The same convolution with its 16 GEMMs on the BF16 matrix cores AT FP32 ACCURACY (round 6; opt-in: IRIS_WINO_SPLIT_BF16=1 on the
 * Python side): v_mfma_f32_32x32x16_bf16 delivers 16x the FLOP per clock of the fp32 MFMA that bounds iris_conv3x3_wino.  Every fp32
 * operand is the EXACT sum of three bf16 values (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)); U is split once per
 * layer when it is packed, V in registers; six of the nine partial products (all down to 2^-24 of the product) are accumulated in
 * fp32 by the matrix cores.  Against an fp64 convolution the error is 0.65 - 1.14x that of iris_conv3x3_wino on the CRNN's
 * geometries (profiles/r6/wino_b3_check_and_time.log; tests/test_transforms_gpu.py holds it to 1.5x and to 1e-6 of the peak), the twelve
 * layers of the forward run 1.13 - 1.57x faster.  Same contract as iris_conv3x3_wino (layouts, flags, bias, pooling) except:
 *   cin % 16 == 0 (one MFMA K-step), cout % 64 == 0
 *   packed  iris_wino_b3_pack_weights_device only: 24 cin cout floats = 96 cin cout bytes (iris_wino_b3_packed_len, in floats)
 * Replaces: the same Conv2D layers of define_keras_model (sj_train.py:191-201, 222-242).
 */
size_t iris_wino_b3_packed_len(int cin, int cout);
int iris_wino_b3_pack_weights_device(const float* weight, long stride_o, long stride_i, long stride_h, long stride_w, int cin, int cout,
                                     int transposed, float* packed, void* stream);
int iris_conv3x3_wino_b3(const float* x, const float* packed, const float* bias, float* y, int batch, int height, int width, int cin,
                         int cout, int flags, void* stream);

/*
 * The WEIGHT GRADIENT of the same convolution, y = conv3x3_same(x, w), as a Winograd F(2x2, 3x3) transform on the fp32 matrix
 * cores - model.fit's backward pass through blocks 2-5 (sj_train.py:191-201, 222-242, 408), which MIOpen runs as implicit
 * GEMMs at 82-127 TFLOP/s: dU[p] = sum over the tiles of the batch of (A dY A^T)[p] (B^T d B)[p] per position p, dW = G^T dU G -
 * 16 instead of 36 multiplies per 2 x 2 tile and channel pair.  Both free dimensions of that GEMM are channels, so with
 * channels-last activations a lane loads its channel's patch straight from memory into the MFMA operand layout (no LDS).
 * Deterministic (the tile rows are split over workgroups whose partial sums are added in a fixed order); against an fp64
 * gradient the error is that of a direct fp32 one (2e-7 .. 6e-7 of the gradient's peak).  cin % 32 == 0, cout % 32 == 0.
 *   x, dy      channels-last [batch][height][width][cin] / [...][cout], DEVICE, fewer than 2^31 bytes each
 *   dw         the gradient, element strides stride_o / _i / _h / _w over [cout][cin][3][3] (a channels_last parameter's
 *              gradient is written as it lies); accumulate != 0 adds to what is there
 *   workspace  DEVICE scratch of at least iris_wino_wrw_workspace_len(batch, height, width, cin, cout) floats (64 MiB on 256 CUs)
 */
size_t iris_wino_wrw_workspace_len(int batch, int height, int width, int cin, int cout);
int iris_conv3x3_wino_wrw(const float* x, const float* dy, float* dw, long stride_o, long stride_i, long stride_h, long stride_w,
                          int batch, int height, int width, int cin, int cout, int accumulate, float* workspace,
                          size_t workspace_len, void* stream);

/*
 * The CRNN's first layer in TRAINING mode - Conv2D(3x3 'same', 1 or 2 input channels) + BatchNormalization + ReLU
 * (sj_train.py:191-201, 244) - with the convolution recomputed from x wherever its output is needed (9-18 FMAs per value
 * against 4 bytes of traffic): z is never stored.  x [batch, in_channels, height, width] contiguous; weight
 * [out_channels, in_channels, 3, 3] contiguous; y / dy [batch, height, width, out_channels] (channels-last); out_channels
 * in {4, 8, ..., 256} dividing 1024.  The convolution runs WITHOUT bias (see iris_bn_stats); x gets no gradient.
 *   forward : iris_conv0_stats (sums_zeroed as for iris_bn_stats), then iris_conv0_bn_relu (arguments as iris_bn_relu_apply)
 *   backward: iris_conv0_bn_relu_backward: two launches (sum g / sum g xhat, then dz and the weight gradient);
 *             sums_zeroed [iris_bn_sums_len(out_channels)] and dweight_zeroed [iris_conv0_dweight_len(...)] DEVICE doubles,
 *             zero on entry; dweight = several partial copies [copies][out_channels][in_channels][3][3] that the caller
 *             adds up (the blocks' atomics are spread over them); dgamma, dbeta [out_channels] floats.
 *             iris_conv0_bn_relu_backward_dx: the same two launches, and the input gradient for a model whose first stage
 *             is trainable (the PCEN layer of a 'pcen_learn' run): the second launch also writes dz into dz_scratch
 *             [batch, height, width, out_channels] (DEVICE floats, 16-byte aligned), a third gathers
 *             dx [batch, in_channels, height, width] from it in a fixed order (no atomics).
 */
size_t iris_conv0_dweight_len(int in_channels, int out_channels);
int iris_conv0_stats(const float* x, const float* weight, int batch, int in_channels, int out_channels, int height, int width,
                     double* sums_zeroed, void* stream);
int iris_conv0_bn_relu(const float* x, const float* weight, float* y, int batch, int in_channels, int out_channels, int height,
                       int width, const double* sums, const float* gamma, const float* beta, const float* conv_bias, float eps,
                       float momentum, float* running_mean, float* running_var, float* save_mean, float* save_rstd, void* stream);
int iris_conv0_bn_relu_backward(const float* x, const float* weight, const float* dy, int batch, int in_channels,
                                int out_channels, int height, int width, const float* save_mean, const float* save_rstd,
                                const float* gamma, const float* beta, double* sums_zeroed, double* dweight_zeroed, float* dgamma,
                                float* dbeta, void* stream);
int iris_conv0_bn_relu_backward_dx(const float* x, const float* weight, const float* dy, int batch, int in_channels,
                                   int out_channels, int height, int width, const float* save_mean, const float* save_rstd,
                                   const float* gamma, const float* beta, double* sums_zeroed, double* dweight_zeroed, float* dgamma,
                                   float* dbeta, float* dz_scratch, float* dx, void* stream);

/*
 * First convolution of the CRNN (ConvMPBlock's Conv2D(32, 3, padding='same') on the n_chan-channel log-mel input,
 * sj_train.py:191-201, 244) with its (BatchNorm-folded) bias and ReLU in ONE pass, NCHW: x [batch, in_channels (1 or 2),
 * height, width], weight [out_channels, in_channels, 3, 3], bias [out_channels] -> y [batch, out_channels, height, width].
 * The layer writes 16-32x what it reads; every output byte is written once.  width a multiple of 4; x, y 16-byte aligned.
 */
int iris_conv3x3_small_bias_relu_nchw(const float* x, const float* weight, const float* bias, float* y, int batch,
                                      int in_channels, int out_channels, int height, int width, void* stream);
/* the same with a channels-last output y [batch, height, width, out_channels] (out_channels in {4, 8, ..., 256} dividing
 * 1024; width <= 2048; bias, y 16-byte aligned), which is what iris_conv3x3_c32_bias_relu reads */
int iris_conv3x3_small_bias_relu_nhwc(const float* x, const float* weight, const float* bias, float* y, int batch,
                                      int in_channels, int out_channels, int height, int width, void* stream);

/*
 * Recurrent half of the v9 CRNN's Bidirectional(LSTM(128, return_sequences=True)) (sj_train.py:252), one launch for all
 * time steps and both directions.  gx [batch, steps, 2, 512] = the input pre-activations x_t W_ih^T + b_ih + b_hh of
 * direction 0 (forward) and 1 (backward), gate rows in the order i, f, g, o (one GEMM for all steps, done by the caller);
 * w_hh [2, 512, 128] the recurrent matrices (16-byte aligned); out [batch, steps, 256] = (h forward, h backward) per step;
 * h_0 = c_0 = 0.  act: NULL for inference; for training [batch, steps, 2, 5, 128] receives (i, f, g, o, c) of every step.
 * iris_bilstm128_backward: dout [batch, steps, 256] and the saved act -> dgx [batch, steps, 2, 512], the gradient of the
 * pre-activations (back-propagation through time inside the launch); dW_ih, db, dx follow from dgx through the caller's GEMM,
 * dW_hh[d] = dgx[:, :, d, :]^T . h_prev with h_prev = out shifted by one step of direction d.
 * fp32, device pointers, current HIP device.
 */
int iris_bilstm128_forward(const float* gx, const float* w_hh, float* out, float* act, int batch, int steps, void* stream);
int iris_bilstm128_backward(const float* dout, const float* act, const float* w_hh, float* dgx, int batch, int steps,
                            void* stream);

/*
 * Sample synthesis in the complex-STFT domain, deterministic half of
 * merge_complex_specs (pipeline.py:6-110) for a whole batch: every output sample
 * is   background crop (tiled along time, pipeline.py:29-35)
 *    + sum over its voices of gain * crop(zero-padded voice) * no_overlap (:48-84)
 *    + sum over its noises of gain * crop(zero-padded noise)              (:86-106)
 * with the frame labels of the accepted voices (:55-66, :78-84).  All random draws
 * (which sources, offsets, gains) are made by the caller and passed in the source
 * table; the data-dependent parts - a voice frame is "active" when max over
 * (freq, chan2) of the frame is > 0 (:57), a voice is dropped when accepting it
 * would make two labels overlap (:78-80) - are evaluated here.
 * Additions happen in table order with separately rounded multiply and add, so
 * the result equals the reference's op-by-op evaluation bit for bit.
 *
 * srcs: DEVICE table, the sources of sample b are srcs[first[b] .. first[b+1]) in
 *       the order background, voices (by slot), noises.  first: DEVICE int32 [B + 1].
 *   src    DEVICE [F, T, C2] fp32 spectrogram (time axis 1, re block | im block last)
 *   active DEVICE [T] fp32 0/1 flags of a voice's frames from iris_mix_frame_active (kind 1;
 *          they depend on the source only, so they are computed once per corpus, not per use)
 *   T      frames in src;  pad: zero frames virtually added on both sides (>= 0);
 *   off    crop offset in the padded (voice, noise) or tiled (background) source;
 *   gain   linear gain (ignored for the background);  kind 0 background, 1 voice, 2 noise, -1 unused slot (skipped);
 *   slot   row of the labels output (kind 1);  label_row: row of label_vecs (kind 1).
 * label_vecs: DEVICE [n_label_rows, n_classes] fp32 (one-hot rows in the reference).
 * spec_out: DEVICE [B, F, n_frame, C2];  labels_out: DEVICE [B, V, n_frame, n_classes].
 * workspace: DEVICE scratch of iris_mix_workspace(n_srcs, n_frame) floats.
 * Runs on the current HIP device.
 */
typedef struct {
    const float* src;
    const float* active;
    int32_t T, pad, off;
    float gain;
    int32_t kind, slot, label_row, reserved;
} iris_mix_src;
/* active_out[t] = 1 when max over (freq, chan2) of src[:, t, :] is > 0, else 0 (pipeline.py:57) */
int iris_mix_frame_active(const float* src, int n_bins, int n_frames, int chan2, float* active_out,
                          void* stream);
size_t iris_mix_workspace(int n_srcs, int n_frame);
int iris_mix_specs(const iris_mix_src* srcs_dev, int n_srcs, const int32_t* first_dev,
                   const float* label_vecs_dev, float* spec_out, float* labels_out, int batch,
                   int n_bins, int n_frame, int chan2, int max_voices, int n_classes,
                   float* workspace, size_t workspace_floats, void* stream);

/*
 * Waveform-domain variant of the batched merge_complex_specs (the STFT is linear, so
 * mixing before it equals mixing after it up to frame-granular cropping - output frames whose window straddles a crop,
 * pad or tiling boundary differ, all others agree to fp32 rounding).  The corpus stays resident as waveforms (a
 * quarter of the bytes of its spectrograms at n_fft 1024 / hop 256) and the mixed batch goes straight into
 * iris_wav_to_logmel; no spectrum is ever materialised.
 * Same source table and the same label rule as iris_mix_specs, with these readings of the record:
 *   src      DEVICE [C, len] fp32 waveform;  reserved = len (samples per channel)
 *   T, pad, off   in FRAMES, as for spectrograms (T = 1 + len / hop); a frame is `hop` samples:
 *            voice / noise sample s of the output reads source sample s + (off - pad) * hop (zero outside [0, len)),
 *            background sample s reads (off * hop + s) mod len
 *   active   [T] flags from iris_mix_wave_frame_active: frame t is active when any sample under the support of its
 *            periodic-Hann window, [t*hop - n_fft/2 + 1, t*hop + n_fft/2 - 1] clipped to the clip, is non-zero in any
 *            channel.  Equivalent to the reference's rule (max over the frame's kept half-spectrum, re and im parts,
 *            > 0: pipeline.py:57) except for degenerate frames: a non-zero windowed frame whose half-spectrum has no
 *            strictly positive re / im component (e.g. x and the window such that every Re X[k], Im X[k], k <= n_fft/2,
 *            is <= 0) is inactive there and active here; tests/test_oracle.py compares the two rules on the synthetic
 *            corpus (they agree on every frame)
 * wav_out: DEVICE [B, C, out_len] with out_len = (n_frame - 1) * hop, i.e. n_frame STFT frames (center=True).
 */
int iris_mix_wave_frame_active(const float* wav, int channels, int len, int n_fft, int hop, float* active_out,
                               void* stream);
int iris_mix_waves(const iris_mix_src* srcs_dev, int n_srcs, const int32_t* first_dev,
                   const float* label_vecs_dev, float* wav_out, float* labels_out, int batch,
                   int channels, int hop, int n_frame, int max_voices, int n_classes,
                   float* workspace, size_t workspace_floats, void* stream);

/*
 * The random half of a batch drawn ON THE DEVICE (no host round trip, replayable from a hipGraph): which sources
 * merge_complex_specs mixes and with which offsets / gains (pipeline.py:29-106; source picking of the dataset graph,
 * :147-174), written as the source table iris_mix_specs / iris_mix_waves consume, and the SpecAugment bands of
 * `augment` (data_utils.py:58-61 -> transforms.py:25-26).  Generator: Philox4x32-10 keyed by `seed`, counter = (call
 * counter, sample, column, purpose); distributions as in the reference:
 *   background: the next source of a shuffled, repeated stream; crop offset ~ U{0 .. reps*T - n_frame}
 *   voices:     the next max_voices sources of their stream, padded to the longest of the group;
 *               n_voices ~ U{1 .. max_voices-1} (1 when max_voices == 1); gain = 10^-U[0, -snr/10);
 *               offset ~ U{0 .. padded_len - n_frame - 1} (0 when that range is empty)
 *   noises:     n_noises ~ U{0 .. max_noises-1}; gain = 10^-U[0, 2); offset ~ U{0 .. max(padded_len - n_frame, 0)}
 *   bands:      size ~ U{0 .. max_mask-1}, offset ~ U{0 .. axis_len - size - 1}
 * "Shuffled, repeated stream" = one keyed pseudo-random permutation of the corpus per epoch (every source exactly once
 * per epoch).  A corpus is described by DEVICE arrays of `n` entries: source addresses, (voices) addresses of their
 * frame-activity flags, frames per source, and - waveform corpora - samples per channel (NULL for spectrogram corpora).
 * state_dev: DEVICE uint64[4] {call counter, background / voice / noise stream positions} (iris_augment_draw: uint64[1]),
 * zero-initialised by the caller once and advanced by every call ON THE DEVICE.
 * table_out: DEVICE [batch * (1 + max_voices + max_noises)] records, FIXED stride per sample (first_out[b] = b * stride,
 * DEVICE int32 [batch + 1]); unused voice / noise slots carry kind = -1, which the mix kernels skip.  Pass
 * n_srcs = batch * stride to iris_mix_specs / iris_mix_waves.  t_bands_out / f_bands_out: DEVICE int32 [batch, n, 2].
 */
typedef struct {
    const float* const* src;    /* DEVICE [n] */
    const float* const* active; /* DEVICE [n] (voices) or NULL */
    const int32_t* T;           /* DEVICE [n] frames per source */
    const int32_t* len;         /* DEVICE [n] samples per channel (waveform corpora) or NULL */
    int32_t n;
} iris_mix_corpus;
int iris_mix_draw(const iris_mix_corpus* backgrounds, const iris_mix_corpus* voices, const iris_mix_corpus* noises /* nullable */,
                  int batch, int n_frame, int max_voices, int max_noises, float min_ratio, float min_noise_ratio, float snr,
                  uint64_t seed, uint64_t* state_dev, iris_mix_src* table_out, int32_t* first_out, void* stream);
int iris_augment_draw(int batch, int n_time, int n_time_masks, int max_time_mask, int n_freq, int n_freq_masks,
                      int max_freq_mask, uint64_t seed, uint64_t* state_dev, int32_t* t_bands_out, int32_t* f_bands_out,
                      void* stream);

/*
 * The draws of FilterAugment for a batch, on the device, in one launch: per sample a band count n ~ U{n_band_lo .. n_band_hi},
 * n + 1 band boundaries over the mel rows (uniform over every placement whose bands are at least min_bw rows wide), decibel
 * values ~ U[db_lo, db_hi) and the resulting gain row for iris_wav_to_logmel_gain / iris_magmel_gain.
 *   kind IRIS_FILTER_STEP:   band j (rows b_j .. b_{j+1} - 1) gets dB_j (n values)
 *   kind IRIS_FILTER_LINEAR: n + 1 values at the boundaries, row m of band j gets
 *                            dB_j + (dB_{j+1} - dB_j) (m - b_j) / (b_{j+1} - b_j)
 *   gain = 10^(dB / 20) (the features are mel magnitudes), evaluated in double from the stored fp32 dB values.
 * Generator: Philox4x32-10 keyed by `seed`, counter (call counter, sample * 64 + column, purpose 7) - the exact recipe is the
 * header comment of csrc/k_draw.h, restated in NumPy by tests/filtaug_ref.py.  state_dev: DEVICE uint64[1] of this
 * function's own, zero-initialised once by the caller, advanced by every call on the device.  Outputs (DEVICE):
 * bounds_out int32 [batch, n_band_hi + 1] (unused tail = n_mel), db_out fp32 [batch, n_band_hi + 1] (unused tail = 0),
 * gain_out fp32 [batch, n_mel].  No atomics, no allocation, no synchronisation: capturable.
 * Checked before any HIP call (IRIS_E_INVALID): batch < 0, n_mel or min_bw <= 0, unknown kind, n_band_lo < 1 or > n_band_hi,
 * n_band_hi > 32, n_mel < n_band_hi * min_bw, db_lo > db_hi or not finite, a NULL pointer with batch > 0.  batch == 0 launches
 * nothing.
 */
#define IRIS_FILTER_STEP 0
#define IRIS_FILTER_LINEAR 1
int iris_filter_draw(int batch, int n_mel, int kind, int n_band_lo, int n_band_hi, int min_bw, float db_lo, float db_hi,
                     uint64_t seed, uint64_t* state_dev, int32_t* bounds_out, float* db_out, float* gain_out, void* stream);

/*
 * Training windows cut from LABELLED RECORDINGS on the device: a ragged set of `n` recordings, each [channels, len_i] fp32
 * with its events as frame intervals, and per sample of a batch a draw (recording i, first frame q).
 *
 * iris_crop_windows gathers the batch in one launch.  recs_dev: DEVICE [n] records - `base` the DEVICE address of the
 * recording's first channel row, `row_stride` the floats between channel rows (>= len), `len` the samples per channel that
 * exist, `ev_first` / `ev_count` the recording's rows of the shared event table.  events_dev: DEVICE int32 [rows, 3] of
 * (class, start frame, end frame); it must be a valid address even when no recording has events.  draws_dev: DEVICE int32
 * [batch, 2] of (i, q).  With L = (n_frame - 1) * hop:
 *   wav_out  DEVICE fp32 [batch, channels, L]: sample s of channel c is base[c * row_stride + q * hop + s] where
 *            q * hop + s < len and exactly 0.0f otherwise - nothing at or beyond index len of a row is ever read, on either
 *            path, so whatever lies behind a row (another recording, padding, NaN) cannot reach the batch
 *   y_out    DEVICE fp32 [batch, n_frame, n_classes]: entry (f, k) is the NUMBER of the recording's events with class == k
 *            and start <= q + f < end (overlapping events add up, as eval.second2frame's labels do)
 * A draw with i outside [0, n) or q < 0 gives a zero window and zero labels.  The launch is a streaming copy: a (sample,
 * channel) row whose source address and destination address are both 16-byte aligned (and L % 4 == 0) moves as 16-byte loads
 * and stores; any other row takes a scalar path with the same result.  Rows that start on 16-byte boundaries with hop % 4 == 0
 * always take the wide path.  No atomics, no allocation, no synchronisation: capturable, bitwise reproducible.
 * Checked before any HIP call (IRIS_E_INVALID): batch < 0, n <= 0, hop <= 0, n_frame < 2, n_classes <= 0, channels not 1 or
 * 2, a NULL pointer with batch > 0; IRIS_E_UNSUPPORTED: a window or label row beyond 2^31 entries, batch * (channels + 1) >
 * 65535.  batch == 0 launches nothing.
 *
 * iris_crop_draw makes the draws in one small launch, every window of the corpus equally likely.  Recording i has
 * n_pos[i] = max((len_i - L) / hop, 0) + 1 positions (integer division; a recording shorter than a window has the one
 * position q = 0 and its tail comes out as zeros); prefix_dev: DEVICE int64 [n + 1], their prefix sums (prefix[0] = 0).
 * Per sample b: the words (x, y) of Philox4x32-10 keyed by `seed` at counter (call counter lo, hi, b * 64, purpose 8) make
 * the 64-bit word x << 32 | y; u = the high 64 bits of word * prefix[n] (uniform on [0, total), bias < total / 2^64); i is
 * found by binary search (prefix[i] <= u < prefix[i + 1]) and q = u - prefix[i].  The recipe is restated in the header
 * comment of csrc/k_crop.h and in NumPy by tests/crop_ref.py.  state_dev: DEVICE uint64[1] of this function's own,
 * zero-initialised once by the caller, advanced by every call on the device (a captured launch replays with fresh draws).
 * draws_out: DEVICE int32 [batch, 2].  One workgroup, no atomics: capturable.
 * Checked before any HIP call (IRIS_E_INVALID): batch < 0, n <= 0, a NULL pointer with batch > 0; IRIS_E_UNSUPPORTED:
 * batch > 2^25.  batch == 0 launches nothing (and does not advance the counter).
 */
typedef struct {
    const float* base;
    int64_t row_stride;
    int32_t len, ev_first, ev_count, reserved;
} iris_crop_rec;
int iris_crop_windows(const iris_crop_rec* recs_dev, int n, const int32_t* events_dev, const int32_t* draws_dev, int batch,
                      int channels, int hop, int n_frame, int n_classes, float* wav_out, float* y_out, void* stream);
int iris_crop_draw(const int64_t* prefix_dev, int n, int batch, uint64_t seed, uint64_t* state_dev, int32_t* draws_out,
                   void* stream);

/*
 * Time stretching of complex spectrograms: the reference's phase_vocoder (transforms.py:137-195) for a RAGGED BATCH of
 * sources, each with its own rate, in one launch.  Per record: src DEVICE [n_bins, n_in, chan2] fp32 (re block | im block
 * last), rate > 0, dst DEVICE buffer whose first n_bins * n_out * chan2 floats receive the contiguous [n_bins, n_out, chan2]
 * result (floats beyond are not written); n_out = ceil(n_in / rate), formed by the caller in double.  Output frame i sits at
 * ts = (double)i * rate (the grid of numpy.arange(0, n_in, rate) in float64): i0 = floor(ts), alpha = (float)(ts - i0);
 * frames >= n_in read as zeros;
 *     mag  = alpha |X[i0 + 1]| + (1 - alpha) |X[i0]|
 *     step = angle(X[j0 + 1]) - angle(X[j0]) - adv, reduced by 2 pi rint(step / 2 pi), + adv   (j0 = i0 of frame i - 1;
 *            frame 0 takes angle(X[0]);  adv = pi * bin, i.e. hop_length = n_bins - 1 as in the reference)
 *     out  = mag (cos, sin)(sum of the steps up to frame i)
 * The running phase is kept reduced to [-pi, pi] wherever it is stored or carried (the reference lets it grow to pi * bin * i
 * and loses ~1e-2 of the peak in fp32); against the float64 evaluation |out - ref| <= mag (1e-5 + 16 u pi (i + 1)), u = 2^-24.
 * mag == 0 gives exactly 0.  rate == 1 copies the source bit for bit.  A record with n_in <= 0, n_out <= 0, rate <= 0 or
 * n_out > max_out_frames is skipped (nothing written): the table lives on the device and cannot be checked here without a
 * synchronisation.  src and dst must not overlap.
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, n_bins < 2, chan2 odd or <= 0, NULL table with n_src > 0,
 * max_out_frames <= 0; IRIS_E_UNSUPPORTED: chan2 > 512, n_src > 65535.  n_src == 0 returns 0 and launches nothing.
 * One launch on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible.  Runs on the
 * current HIP device.
 */
typedef struct {
    const float* src;
    float* dst;
    int32_t n_in, n_out;
    double rate;
} iris_voc_src;
int iris_phase_vocoder(const void* table_dev, int n_src, int n_bins, int chan2, int max_out_frames, void* stream);

/*
 * Speed perturbation of waveforms (Ko et al., Interspeech 2015; Kaldi's 0.9 / 1.0 / 1.1): a RAGGED BATCH of waveforms, each
 * resampled by its own real-valued rate and played back at the old sample rate (tempo and pitch move together), in one launch.
 * Per record: src DEVICE [channels, len_in] fp32, rate > 0 (rate > 1 = faster and shorter, the convention of
 * iris_phase_vocoder), dst DEVICE buffer whose first channels * len_out floats receive the contiguous [channels, len_out]
 * result (floats beyond are not written); len_out = iris_speed_len(len_in, rate) = ceil(len_in / rate), formed in double.
 * Output sample m sits at pos = (double)m * rate: i0 = floor(pos), frac = (float)(pos - i0), and
 *     y[c, m] = sum_s x[c, s] * cut * g(cut * ((s - i0) - frac)),      cut = 0.99 * min(1, 1 / rate),
 *     g(t)    = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,     x[c, s] = 0 outside [0, len_in)
 * - the Hann-windowed sinc of torchaudio.functional.resample (lowpass_filter_width 6, rolloff 0.99) evaluated at a real-valued
 * position; for a rational rate = o / n it is iris_resample(orig_freq = o, new_freq = n) with no host-built tap table.
 * Against the float64 evaluation |y - ref| <= 8 u S, u = 2^-24, S = cut * (sum of |x[c, s]| over the support).  An output
 * sample whose whole support is zero input is exactly 0.  rate == 1 copies the source bit for bit (it does not low-pass at
 * 0.99).  A record with len_in <= 0, len_out <= 0, rate <= 0, len_out > max_out_len or a NULL pointer is skipped (nothing
 * written): the table lives on the device and cannot be checked here without a synchronisation.  src and dst must not overlap.
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, channels <= 0, NULL table with n_src > 0, max_out_len <= 0;
 * IRIS_E_UNSUPPORTED: n_src > 65535.  n_src == 0 returns 0 and launches nothing.
 * One launch on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible, and a record's
 * result does not depend on the records around it.  Runs on the current HIP device.
 *
 * iris_mix_wave_frame_active_batch: the frame activity (iris_mix_wave_frame_active, bit for bit) of every waveform
 * `dst` [channels, len_out] of the same table in one launch.  Only `dst` and `len_out` of a record are read.
 *   active_ptrs_dev  DEVICE [n_src] addresses of the DEVICE float vectors that receive the flags: record i writes
 *                    active_ptrs[i][t] for t < 1 + len_out_i / hop (the vector must hold that many floats); entries beyond
 *                    are not written
 *   max_frames       the largest frame count of the table (it sizes the grid, as max_out_len does): a record with
 *                    len_out <= 0, a NULL dst, a NULL vector or 1 + len_out / hop > max_frames is skipped
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, channels <= 0, n_fft <= 1, hop <= 0, NULL table or NULL
 * active_ptrs_dev with n_src > 0, max_frames <= 0; IRIS_E_UNSUPPORTED: n_src > 65535.  n_src == 0 launches nothing.
 */
typedef struct {
    const float* src;
    float* dst;
    int32_t len_in, len_out;
    double rate;
} iris_speed_src;
long long iris_speed_len(long long len, double rate); /* ceil(len / rate); 0 for len <= 0 or a rate that is not positive and finite */
int iris_speed_perturb(const void* table_dev, int n_src, int channels, int max_out_len, void* stream);
int iris_mix_wave_frame_active_batch(const void* table_dev, int n_src, int channels, int n_fft, int hop,
                                     const void* active_ptrs_dev, int max_frames, void* stream);

/*
 * Activity gate of a waveform corpus: per frame, is the voice speaking?  The samples of the other frames become exact zeros,
 * so that the mixers' label rule (iris_mix_wave_frame_active: a frame is active when any sample under its window is non-zero)
 * means something on clips that hold no exact zeros of their own.  A RAGGED BATCH of waveforms in three launches.
 * Per record: src DEVICE [channels, len] fp32 (contiguous, len >= 1), and with h2 = hop / 2, T = 1 + len / hop (the mixers'
 * frame count) and owner(s) = min((s + h2) / hop, T - 1):
 *   1. E[t] = sum_c sum_{s: owner(s) = t} (double)x[c, s]^2, accumulated in double (the products are exact); a frame that
 *      owns no sample has E = 0.  The order of the sum does not depend on the record's address.
 *   2. P = the maximum of the E[t] that are not NaN, 0 if there are none; thr = max(P * ratio, floor);
 *      m0[t] = (E[t] >= thr) && (E[t] > 0).  Comparisons are false on NaN; +inf follows IEEE.
 *   3. close: every maximal run of zeros of m0 of length <= min_gap with a one on both sides becomes ones (m1)
 *   4. drop:  every maximal run of ones of m1 shorter than min_event becomes zeros (m2)
 *   5. hang:  m[t] = OR of m2[u] over |u - t| <= hang, clipped to [0, T)
 *   6. dst[c, s] = src[c, s] bit for bit where m[owner(s)] is set, +0.0f elsewhere
 * Outputs per record: dst DEVICE [channels, len] (floats beyond are not written), mask DEVICE uint8 [T] (m), energy DEVICE
 * double [T] (E; 8-byte aligned).  dst == src gates in place: every energy is read before anything is written.  Otherwise
 * the buffers of a record, and of different records, must not overlap.  Rows need no alignment.
 *   ratio    10^(-range_db / 10), formed in double by the caller: in (0, 1)
 *   floor    an absolute energy below which no frame is active: >= 0
 *   max_len  the largest len of the table (it sizes the grids): a record with len <= 0, len > max_len or a NULL pointer is
 *            skipped (nothing written) - the table lives on the device and cannot be checked here without a synchronisation
 * Frames per record: at most IRIS_GATE_MAX_FRAMES = 131072 (the masks of steps 2 - 5 are bit words in LDS), checked here
 * through max_len (IRIS_E_UNSUPPORTED), as is n > 65535.  Checked before any HIP call (IRIS_E_INVALID): a NULL table, n <= 0,
 * channels <= 0, hop < 1, min_gap < 0, min_event < 1, hang < 0, ratio outside (0, 1), floor < 0 or NaN, max_len <= 0.
 * Three launches on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible, and a record's
 * result does not depend on the records around it.  Runs on the current HIP device.
 */
#define IRIS_GATE_MAX_FRAMES 131072
typedef struct {
    const float* src;      /* DEVICE [channels, len] */
    float*       dst;      /* DEVICE [channels, len]; may be src */
    uint8_t*     mask;     /* DEVICE [1 + len / hop] */
    double*      energy;   /* DEVICE [1 + len / hop] */
    int32_t      len, reserved;
} iris_gate_rec;
int iris_activity_gate(const void* table_dev, int n, int channels, int hop, int min_gap, int min_event, int hang, double ratio,
                       double floor, int max_len, void* stream);

/*
 * Reverberation of waveforms (Ko et al., ICASSP 2017; Kaldi's reverberate_data_dir): a RAGGED BATCH of waveforms, each channel
 * convolved with its own impulse response, in one launch - a direct-form FIR in fp32.
 * Per record: src DEVICE [channels, len] fp32, taps DEVICE [channels, n_taps] fp32, dst DEVICE [channels, len] (contiguous;
 * floats beyond channels * len are not written):
 *     y[c, m] = sum_{k = 0}^{n_taps - 1} taps[c, k] * x[c, m - k]      for 0 <= m < len,     x[c, i] = 0 for i < 0
 * - the causal convolution, cut at the input length: the direct sound sits at tap 0 and whatever rings past the end of the
 * input is dropped (Kaldi's default), so the length of a waveform, its frame count and its labels do not change.
 * Each output is one fp32 FMA chain in ascending k: against the float64 evaluation |y - ref| <= (n_taps + 2) u S[c, m],
 * u = 2^-24, S[c, m] = sum_k |taps[c, k]| |x[c, m - k]| (the forward bound of an fp32 inner product of n_taps terms).  An
 * output sample whose whole support is zero input is exactly 0.  taps = [1] copies the source bit for bit.  A record with a
 * NULL pointer, len <= 0, n_taps <= 0, len > max_len or n_taps > max_taps is skipped (nothing written): the table lives on the
 * device and cannot be checked here without a synchronisation.  dst must not overlap src or taps.
 *   max_len   the largest len of the table (it sizes the grid: tiles of max_len x channels x n_src)
 *   max_taps  the largest n_taps of the table
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, channels <= 0, NULL table with n_src > 0, max_len <= 0,
 * max_taps <= 0; IRIS_E_UNSUPPORTED: n_src > 65535, channels > 65535.  n_src == 0 returns 0 and launches nothing.
 * One launch on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible, and a record's
 * result does not depend on the records around it.  Runs on the current HIP device.
 */
typedef struct {
    const float* src;    /* DEVICE [channels, len] */
    float*       dst;    /* DEVICE [channels, len]; must not overlap src */
    const float* taps;   /* DEVICE [channels, n_taps] */
    int32_t      len, n_taps;
} iris_fir_src;
int iris_fir_batch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, void* stream);
/* The same with the rows of a record's taps `tap_pitch` floats apart (taps DEVICE [channels, tap_pitch], the first n_taps of
 * each row read): the layout iris_ism_rir writes.  tap_pitch == 0 is iris_fir_batch (rows n_taps apart); 0 < tap_pitch <
 * max_taps is IRIS_E_INVALID.  The results are those of iris_fir_batch on the same numbers, bit for bit. */
int iris_fir_batch_pitch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, int tap_pitch, void* stream);

/*
 * The same convolution for LONG impulse responses (a hall rings for a second and more: 16000+ taps at 16 kHz), as a uniformly
 * partitioned overlap-save convolution on the FFT core: block B = 1024 new samples, transform N = 2048, n_taps up to
 * IRIS_FFT_FIR_MAX_TAPS = 32768 (2 s at 16 kHz).  Per record src, dst, taps as for iris_fir_batch, the same definition
 *     y[c, m] = sum_{k < n_taps, k <= m} taps[c, k] * x[c, m - k]      for 0 <= m < len
 * and `ws_off`, the byte offset (a multiple of 16) of the record's own slice of `workspace`: iris_fft_fir_workspace(channels,
 * len, n_taps) = channels * (ceil(len / B) + ceil(n_taps / B)) * 8256 bytes (0 for channels, len or n_taps <= 0 or n_taps >
 * 32768), the spectra of its input frames x[(j - 1) B, (j + 1) B) and of its tap partitions taps[p B, (p + 1) B).  The slices
 * of the records of one call must not overlap.  Two launches on `stream`: the spectra (one wave per frame), then per output
 * block j the products summed over the partitions in ascending p in registers, one inverse transform and the store of
 * y[j B, min((j + 1) B, len)).  Floats of dst beyond channels * len are not written; rows need no alignment.
 * An FFT convolution is not bounded tap by tap: against the float64 evaluation the bound is norm-wise per output block,
 *     |y - ref| <= 8 u R[c, m],   u = 2^-24,   R[c, m] = sum_{p <= j} ||frame_{j - p}||_2 ||partition_p||_2,   j = m / B
 * (DESIGN.md K2f).  An all-zero input gives exactly 0.  A record with a NULL pointer, len <= 0, n_taps <= 0, len > max_len,
 * n_taps > max_taps, or a slice that is misaligned or does not fit `workspace_bytes` is skipped (nothing written).
 *   tap_pitch  floats between the rows of a record's taps; 0: the rows are n_taps apart (iris_fir_batch_pitch's meaning)
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, channels <= 0, tap_pitch < 0, and with n_src > 0 a NULL table,
 * max_len <= 0, max_taps <= 0, 0 < tap_pitch < max_taps, a NULL or misaligned workspace or one below the smallest record's
 * need; IRIS_E_UNSUPPORTED: n_src > 65535, channels > 65535, max_taps > 32768.  n_src == 0 returns 0 and launches nothing.
 * No atomics, no synchronisation: bitwise reproducible, a record's result does not depend on the records around it, and
 * both launches are capturable - except that the FIRST call on a device uploads the transform's twiddles (built on the host
 * in double); make that call outside any capture.  Runs on the current HIP device.
 */
#define IRIS_FFT_FIR_MAX_TAPS 32768
typedef struct {
    const float* src;    /* DEVICE [channels, len] */
    float*       dst;    /* DEVICE [channels, len]; must not overlap src */
    const float* taps;   /* DEVICE [channels, tap_pitch or n_taps] */
    int32_t      len, n_taps;
    int64_t      ws_off; /* byte offset of the record's slice of the workspace, a multiple of 16 */
} iris_fft_fir_src;
long long iris_fft_fir_workspace(int channels, int len, int n_taps);
int iris_fft_fir_batch(const void* table_dev, int n_src, int channels, int max_len, int max_taps, int tap_pitch, void* workspace,
                       long long workspace_bytes, void* stream);

/*
 * Shoebox room simulation (Allen & Berkley, JASA 1979: the image-source method, as pyroomacoustics and gpuRIR compute it): the
 * room impulse responses of a RAGGED BATCH of voices, each with its own room, source, microphones, wall reflection coefficient
 * and tap count, in one launch.  All microphones of a record sit in the same room with the same source, so every reflection
 * reaches them with its own delay and gain: the inter-channel time and level differences are those of the geometry.
 * Per record, with c = 343 m/s, fs = sample_rate, W = 16 and L = room: images n in [-N_a, N_a]^3, p in {0, 1}^3 at
 *     x_a = (1 - 2 p_a) src_a + 2 n_a L_a,      e = sum_a (|n_a - p_a| + |n_a|) reflections,
 * d = |x - mic[ch]|, tau = d fs / c samples; tau_min = the smallest DIRECT (n = 0, p = 0) delay over the channels of the record
 * and d_min its distance; t = tau - tau_min + W and
 *     h[ch][k] = sum_images beta^e (d_min / d) w(k - t)   for 0 <= k < n_taps,
 *     w(x)     = sinc(x) 0.5 (1 + cos(pi x / W)) for |x| < W, else 0;  sinc(x) = sin(pi x) / (pi x), sinc(0) = 1
 * - the nearest microphone's direct sound is a unit tap at k = W (1 ms at 16 kHz) and the delay between the channels is kept.
 * N_a = floor(D / (2 L_a)) + 1 with D = c (tau_min + n_taps) / fs: no image beyond can reach a tap below n_taps, and images
 * with t - W >= n_taps - 1 are skipped, so within its n_taps taps the response is the complete image sum, not an
 * order-truncated one.  normalize != 0: every channel of a record is multiplied by the SAME g = 1 / sqrt(mean_ch sum_k h^2)
 * (white input keeps its mean power, the level difference between the channels is untouched; an all-zero response, such as
 * n_taps <= W with integer delays, is left as it is).
 *   dst  DEVICE [channels, max_taps] fp32: row ch receives h[ch][0 .. n_taps); the floats beyond n_taps of a row are not written
 * Positions, d, tau, t, floor(t) and the fraction are formed in double, the window, the sinc and the products in fp32; each
 * contribution is rounded to a multiple of 2^-32 and accumulated as a 64-bit integer, so the result does not depend on the
 * order of the additions: bitwise reproducible run to run.  Against the float64 evaluation
 *     |h - ref| <= 3.6 u A_k + n_k 2^-33,    u = 2^-24, A_k = sum |beta^e d_min / d| and n_k = the number of images whose
 * window covers tap k (with normalize, (3.6 u A_k + n_k 2^-33 + 4 u |ref_k|) g against ref g).
 * Checked on the host before any HIP call, on `table_host` (IRIS_E_INVALID, the record named in iris_last_error): n_src < 0,
 * channels <= 0, NULL tables with n_src > 0, max_taps outside 1 .. 4096, a sample_rate that is not positive and finite; per
 * record a NULL dst, n_taps outside 1 .. 4096, max_taps < n_taps, non-finite or non-positive room sizes, a source or a
 * microphone outside [0, L_a] (NaN included), a source on the nearest microphone (d_min = 0), beta outside [0, 1), a lattice of
 * more than 2^31 - 1 images.  IRIS_E_UNSUPPORTED: channels > IRIS_ISM_MAX_CHAN, n_src > 65535.  n_src == 0 launches nothing.
 *   table_host  HOST copy of the records (what the checks read);  table_dev  the same bytes on the DEVICE (what the kernel reads)
 * One launch on `stream`; no workspace, no synchronisation: capturable, and a record's result does not depend on the records
 * around it.  Runs on the current HIP device.
 */
#define IRIS_ISM_MAX_CHAN 8
typedef struct {
    float*  dst;                         /* DEVICE [channels, max_taps] */
    double  room[3];                     /* L_x, L_y, L_z in metres */
    double  src[3];                      /* the source */
    double  beta;                        /* wall reflection coefficient, the same for the six walls, in [0, 1) */
    int32_t n_taps, reserved;
    double  mic[IRIS_ISM_MAX_CHAN][3];   /* the first `channels` rows are read */
} iris_ism_src;
int iris_ism_rir(const iris_ism_src* table_host, const void* table_dev, int n_src, int channels, int max_taps,
                 double sample_rate, int normalize, void* stream);

/*
 * Fly-by augmentation: a static source heard by a MOVING microphone array - the time-varying delay per channel (Doppler shift
 * and a changing inter-channel delay), the spherical-spreading level and one ground reflection - for a RAGGED BATCH of
 * waveforms, each with its own flight, in one launch.  The sample rate is 16 kHz, the sound speed 343 m/s.
 * Per record: src DEVICE [channels, len] fp32, dst DEVICE [channels, len] fp32 (output channel ch is made from row ch of the
 * source; what arrives later than the buffer is cut).  Ground plane z = 0, source at (0, 0, z_s), array centre p(t) = p0 + v t
 * with t = n / 16000, microphone ch at p(t) + mic[ch].  Paths: p = 0 direct (a_0 = 1), p = 1 - only with n_paths == 2 - the
 * image source (0, 0, -z_s) with a_1 = beta.  With d_p(n) the distance from the microphone at sample n to the (image) source:
 *     pos_p(n) = n - (d_p(n) - r_ref) * (16000 / 343),       g_p(n) = a_p * r_ref / d_p(n),
 *     y[ch, n] = sum_p g_p(n) * sum_s x[ch, s] * cut * w(cut * (s - pos_p(n))),      cut = 0.99 / (1 + |v| / 343),
 *     w(t)     = sinc(pi t) * cos^2(pi t / 12)  for |t| < 6, else 0,     x[ch, s] = 0 outside [0, len)
 * - the window of iris_speed_perturb at a position that moves with the flight; one cut per record is alias-safe for the whole
 * clip, because d pos / d n <= 1 + |v| / 343.  r_ref is the caller's reference distance (the smallest direct distance of the
 * flight: delay 0 and gain 1 at the nearest point).  d, pos, floor(pos) and the fraction are formed in double (dx, dy, dz by one
 * fma each, d^2 by two more); the fraction and the gain are rounded once, the taps (sinf / cosf per tap), the sum in ascending s
 * (an fma per tap) and y = fma(g_1, sum_1, g_0 * sum_0) are fp32: a fixed operation sequence per value that depends neither on
 * the tile nor on the staging.  Against the float64 evaluation |y - ref| <= 4 u S, u = 2^-24, S = cut * sum_p |g_p| * (sum of
 * |x[ch, s]| over the support).  An output sample whose whole support is zero input is exactly 0.  n_paths == 0 copies the
 * source bit for bit (the geometry is not read).
 * A record with a NULL pointer, len <= 0, len > max_len, n_paths outside 0 .. 2 or - at n_paths > 0 - a non-finite p0, v, z_s,
 * beta, r_ref or microphone, r_ref <= 0 or |v| >= 343 is skipped (nothing written): the table lives on the device and cannot be
 * checked here without a synchronisation.  src and dst must not overlap.
 * Checked before any HIP call (IRIS_E_INVALID): n_src < 0, channels <= 0, NULL table with n_src > 0, max_len <= 0;
 * IRIS_E_UNSUPPORTED: channels > IRIS_FLYBY_MAX_CHAN, n_src > 65535.  n_src == 0 returns 0 and launches nothing.
 * One launch on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible, and a record's
 * result does not depend on the records around it.  Runs on the current HIP device.
 */
#define IRIS_FLYBY_MAX_CHAN 8
typedef struct {
    const float* src;                      /* DEVICE [channels, len] */
    float*  dst;                           /* DEVICE [channels, len] */
    int32_t len, n_paths;                  /* n_paths: 0 the identity, 1 direct, 2 direct + ground reflection */
    double  p0[3], v[3];                   /* the array centre at t = 0 (m) and its velocity (m / s) */
    double  z_s, beta, r_ref;              /* source height, ground reflection coefficient, reference distance */
    double  mic[IRIS_FLYBY_MAX_CHAN][3];   /* offsets from the array centre; the first `channels` rows are read */
} iris_flyby_src;
int iris_flyby(const void* table_dev, int n_src, int channels, int max_len, void* stream);

/*
 * Inverse STFT of a RAGGED BATCH of complex spectrograms in the reference layout, in one launch: the inverse of iris_stft /
 * load_wav's Spectrogram(n_fft, power = None), i.e. torch.istft(n_fft, hop, window = periodic Hann, center = True, onesided,
 * normalized = False, length = len_out).  n_fft, hop, the channel count C and the constants come from the plan.
 * Per record: src DEVICE [F = n_fft / 2 + 1, n_frames, 2C] fp32 (re block | im block last), dst DEVICE buffer whose first
 * C * len_out floats receive the contiguous [C, len_out] result (floats beyond are not written), len_out <= (n_frames - 1) hop
 * = iris_istft_len(n_frames, hop).  With N = n_fft, w[i] = 0.5 - 0.5 cos(2 pi i / N) (formed in double, rounded once) and
 * p = n + N / 2:
 *     x_t[i]  = (1 / N) (Re S[0, t] + (-1)^i Re S[N/2, t] + 2 sum_{0 < f < N/2} (Re S[f, t] cos(2 pi f i / N) - Im S[f, t] sin(2 pi f i / N)))
 *     y[c, n] = (sum_t w[p - t hop] x_t[p - t hop]) / (sum_t w[p - t hop]^2)     over 0 <= t < n_frames with 0 <= p - t hop < N,
 *                                                                                  in ascending t
 * The imaginary parts of bins 0 and N / 2 are ignored.  Against the float64 evaluation |y - ref| <= 128 u S[c, n], u = 2^-24,
 * S = (sum_t w[p - t hop] rms_i(x_t)) / (sum_t w[p - t hop]^2).  A sample whose covering frames are all zero is exactly 0; a
 * NaN stays inside the samples its frame covers.  A record with n_frames < 2, len_out <= 0, len_out > (n_frames - 1) hop,
 * n_frames > max_frames (it sizes the grid) or a NULL pointer is skipped (nothing written): the table lives on the device and
 * cannot be checked here without a synchronisation.  src and dst must not overlap.
 * Checked before any HIP call: NULL plan, n_src < 0, NULL table with n_src > 0, max_frames < 2 -> IRIS_E_INVALID; a mel-only
 * plan, hop > n_fft / 2 (the envelope could vanish; with hop <= n_fft / 2 it is at least 0.5 inside the kept range), more
 * channels than the LDS holds (n_fft 512: 4), (max_frames - 1) hop near 2^31, n_src > 65535 -> IRIS_E_UNSUPPORTED.  Every
 * n_fft a plan can have (256 ... 2048) is supported.  n_src == 0 returns 0 and launches nothing.
 * One launch on `stream`; no workspace, no atomics, no synchronisation: capturable, bitwise reproducible, and a record's
 * result does not depend on the records around it.  Runs on the current HIP device (the plan's).
 */
typedef struct {
    const float* src;
    float* dst;
    int32_t n_frames, len_out;
} iris_istft_src;
long long iris_istft_len(long long n_frames, int hop); /* (n_frames - 1) * hop; 0 for n_frames < 2 or hop <= 0 */
int iris_istft(iris_plan* plan, const void* table_dev, int n_src, int max_frames, void* stream);

/*
 * Per-kernel timing for bench.py: with enable = n > 0 every n-th call of
 * iris_wav_to_logmel carries a start/stop hipEvent pair around each of its
 * kernels on the launch stream (n = 1: every call; an event pair costs a few
 * microseconds of stream time, so time throughput with timing off and the
 * kernels in a separate pass); 0 switches it off.  The first 4 calls after
 * enabling are never sampled (first dispatch on an idle GPU, clock ramp).
 * iris_timing_samples synchronises the events and copies the durations (ms) of
 * kernel 0 (the fused kernel) or 1 (the min-max / log kernel, when the call
 * ran it) recorded since the last enable / read to HOST memory; it does not
 * reset.  iris_timing_read returns count and mean of kernel 0 and resets both.
 */
int iris_timing_enable(iris_plan* plan, int enable);
int iris_timing_read(iris_plan* plan, int* n_launches, float* mean_ms);
int iris_timing_samples(iris_plan* plan, int kernel, float* out_ms_host, int capacity, int* n_samples);

#ifdef __cplusplus
}
#endif
#endif /* IRIS_FRONTEND_H */
