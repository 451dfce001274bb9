// iris_frontend.hip -- HIP kernels + C ABI of the MI355X audio feature frontend.
// Written for gfx950 (CDNA4) only: 64-lane wavefronts, 160 KiB LDS per CU,
// 8 XCDs with private L2s.  See include/iris_frontend.h for the contract and
// DESIGN.md for the data layout and the roofline of each kernel.
//
// One translation unit, split by subject:
//   common.h         includes, diagnostics switches, error plumbing, the plan, small device helpers
//   iris_fft.h       the wave-per-frame FFT core (registers + private LDS exchanges)
//   spectrum.h       frame loads, untangle (+ magnitude), the per-lane constant block
//   k_fused.h        K1: waveform -> mel magnitudes (the hot path)
//   k_fused_mfma.h   K1m: the same with the mel contraction on the matrix cores (fp16 MFMA variant)
//   k_stft.h         STFT in the reference layout
//   k_istft.h        inverse STFT of a ragged set of spectrograms in that layout (pickled spectrum corpora -> waveforms), one launch
//   k_magmel.h       spectrum -> mel
//   k_ipd.h         stereo spectrum -> mel-band inter-channel phase difference (cos, sin), its own streaming kernel (opt-in)
//   k_whiten.h      stereo spectrum -> spatially whitened mel-band energy x^H (R + d I)^-1 x, two launches (opt-in)
//   k_locate.h      stereo spectrum + whitening factors + events -> the noise-whitened steered response over a lag grid: which
//                    inter-channel delay, hence bearing, fits each detected event (two launches, double)
//   k_beamform.h    stereo spectrum + whitening factors + events + delays -> the MVDR-beamformed spectrum of each event, one
//                    [F, T_e, 2] slab per event in iris_istft's record layout (one streaming launch)
//   k_postfilter.h  those slabs + the factors of noise="quiet" -> the decision-directed Wiener post-filter's slabs: one sequential
//                    chain per (event, bin), transposed through LDS (one launch, double)
//   k_elementwise.h  min-max / log, normalize, magnitude-phase, mask, adaptive gradient clipping
//   k_mix.h          batched sample synthesis (merge_complex_specs)
//   k_draw.h         the random half of a batch drawn on the device (source table, SpecAugment bands)
//   k_crop.h         training windows cut from labelled recordings: the draws (recording, first frame) and the gather of the
//                    windows and their frame labels, one launch each
//   k_lstm.h         the CRNN's bidirectional LSTM: forward and backward through time, one launch each
//   k_conv_small.h   the CRNN's first convolution (1-2 input channels) with bias + ReLU, one pass (inference)
//   k_conv0_bn.h     the same layer in training mode: convolution recomputed inside the BatchNorm + ReLU passes
//   k_conv_c32.h     the 32 -> 32 convolution of block 1 on the fp32 matrix cores, bias + ReLU (+ MaxPool) fused (inference)
//   k_conv_wino.h    blocks 2-5 (64 ... 512 channels) as Winograd F(2x2, 3x3) on the fp32 matrix cores (inference; the training
//                    step's forward and backward-data passes)
//   k_conv_wino_b3.h   the same convolution on the BF16 matrix cores at fp32 accuracy: three-term split of both operands (opt-in)
//   host_wino.h        the host side of both: the device packers' entry points and one launch path over the two kernel families
//   k_conv_wino_wrw.h  the same layers' weight gradient as Winograd F(2x2, 3x3) on the fp32 matrix cores (training)
//   k_metrics.h      the training metrics er_score / cos_sim / F1 counts of a batch in one launch
//   k_curves.h       the validation score histogram per (class, label): integer counts behind ROC-AUC / average precision / best F1
//   k_psds.h         intersection-based detection counts at up to 64 thresholds behind the polyphonic sound detection score (two launches)
//   decode_core.h    the event decoder's arithmetic (overlap-add average, smoothing, dilation, run boundaries), written once
//   k_detect.h       window predictions of many files -> smoothed, thresholded event lists (two launches)
//   k_hmm.h          the opt-in other decoder: a two-state HMM per class, exact integer Viterbi as a (max, +) scan along time (two
//                    launches; shares step 1 and the run search with k_detect.h)
//   k_tune.h         k_detect.h's decoder (decode_core.h) at every point of a settings grid, scored against ground truth: event and match
//                    counts per (grid point, file, class) in two launches
//   k_pcen.h         per-channel energy normalisation: a chunked scan of the IIR smoother along time, then the compression
//                    (host scalars, or per-band parameters from a device array: the trainable layer's forward)
//   k_pcen_grad.h    the trainable layer's backward: gradient with respect to the per-band parameters, two launches, no atomics
//   k_vocoder.h      time stretching: a batched phase vocoder over a ragged set of spectrograms, the running phase as the same
//                    chunked scan modulo 2 pi
//   k_speed.h        speed perturbation: a batched band-limited resampler over a ragged set of waveforms, each at its own
//                    real-valued rate, and the frame activity of the results, one launch each
//   k_flyby.h        fly-by augmentation: a static source heard by a moving array - a time-varying fractional delay per channel
//                    (Doppler, inter-channel delay), spreading level and one ground reflection over a ragged set of waveforms,
//                    one launch
//   k_gate.h         activity gate of a waveform corpus: frame energies in double, the mask (threshold, close, drop, hang) and
//                    the gated copy of a ragged set of waveforms, one launch each
//   k_fir.h          reverberation: a batched direct-form FIR over a ragged set of waveforms, each channel with its own taps,
//                    one launch
//   k_fft_fir.h      the same convolution for long impulse responses (up to 32768 taps): partitioned overlap-save on the FFT
//                    core, two launches
//   k_ism.h          shoebox room simulation: image-source room impulse responses of a ragged set of voices, fixed-point LDS
//                    accumulators, one launch (its entry point and checks: host_ops.h)
//   host_plan.h      mel matrix, constant tables, plan create / destroy
//   host_ops.h       the operators' C-ABI entry points
#include "common.h"
#include "spectrum.h"
#include "k_fused.h"
#include "k_fused_mfma.h"
#include "k_stft.h"
#include "k_istft.h"
#include "k_magmel.h"
#include "k_ipd.h"
#include "k_whiten.h"
#include "k_locate.h"
#include "k_beamform.h"
#include "k_postfilter.h"
#include "k_track.h"
#include "k_elementwise.h"
#include "host_plan.h"
#include "k_ism.h"
#include "host_ops.h"
#include "k_mix.h"
#include "k_draw.h"
#include "k_crop.h"
#include "k_lstm.h"
#include "k_conv_small.h"
#include "k_conv0_bn.h"
#include "k_conv_c32.h"
#include "k_conv_wino.h"
#include "k_conv_wino_b3.h"
#include "host_wino.h"
#include "k_conv_wino_wrw.h"
#include "k_resample.h"
#include "k_agc_adam.h"
#include "k_agc_optim.h"
#include "k_metrics.h"
#include "k_curves.h"
#include "k_sedeval.h"
#include "k_psds.h"
#include "decode_core.h"
#include "k_detect.h"
#include "k_hmm.h"
#include "k_tune.h"
#include "k_pcen.h"
#include "k_pcen_grad.h"
#include "k_vocoder.h"
#include "k_speed.h"
#include "k_flyby.h"
#include "k_gate.h"
#include "k_fir.h"
#include "k_fft_fir.h"
