// k_fused.h -- K1, the fused hot path: waveform -> (log-)mel in one kernel.
// Part of the single translation unit iris_frontend.hip.
#pragma once
// ---------------------------------------------------------------------------
// K1: fused wav -> mel magnitudes -> (FUSE) per-sample min-max and log, or (!FUSE) per-wave min/max partials for K2
//   work unit = chunk: consecutive frames of one clip, all C channels
//   grid      = min(#chunks, #CUs) workgroups looping over chunks; one workgroup per CU with every
//               wave the registers allow (16 at n_fft <= 1024, 12 with SpecAugment bands at 1024 and at 2048, 8
//               for the other 2048 variants: fused_waves)
//   per wave  = one frame at a time, claimed from the chunk's LDS queue, software-pipelined:
//                 frame i is windowed, transformed (registers + private padded LDS exchanges),
//                 untangled with the magnitude fused in, |X| goes to LDS; then - its sample
//                 registers now dead - frame i+1 is loaded into them straight from global memory
//                 and frame i+2 claimed, both in flight behind the banded mel reduction of frame i;
//                 lane m puts band m of the frame into the chunk's LDS tile (FUSE) or stores it straight to
//                 out[b, m, t, c] (the L2 merges the 4-byte stores).
//   LDS       = staging area of the constant block (re-read at the top of every chunk by the FUSE variants) |
//               exchange buffers [waves] (also |X|) | frame queue | mel table (mode 1) | time-band bitmap (BANDS) |
//               mel tile [M][pitch] + reduction scratch (FUSE); between prologue and epilogue the waves share
//               nothing but the queue
//   MELMODE 0 = band weights in registers (M <= 64, aligned band span <= 20, half spectrum): each lane
//               reads a 16-byte-aligned window of 20 magnitudes with 5 ds_read_b128
//           3 = band weights in registers, two bands per lane (64 < M <= 128, aligned band span <= 8
//               bins - e.g. the reference's 80 mel over 257 bins): 2 x 2 ds_read_b128 per frame
//           1 = band table staged in LDS as float4 rows, 2 = band table read from global (L1/L2)
//   HI        = some band needs bins above n_fft/4 (both halves of the untangle)
//   BANDS     = SpecAugment / filter bands present (time bands: per-chunk bitmap, masked frames skip
//               the transform; frequency bands: folded into the chunk's band weights)
//   S         = frames in flight per wave (1; 2 exists in diagnostic builds for n_fft 512 / 1024 and measured slower)
//   FUSE      = min-max / log inside the kernel (clip-level granule exchange, see the epilogue) instead of per-wave
//               partials for a second kernel: 1 = the chunk's mel values wait in an LDS tile and reach HBM once, finished;
//               2 = no tile (chunks of any size; round-5 experiment, selectable, never the default): the raw mel goes
//               to `out` as in the unfused form and the SAME workgroup finishes its chunk's rows in place once the clip's
//               range is known - its own stores, a barrier apart, read back through L2 / Infinity Cache.  Same bits; 3-5 %
//               slower than the two-kernel form at the batch sizes whose tile does not fit (EXPERIMENTS.md)
// ---------------------------------------------------------------------------
// One workgroup per CU holding every wave of the CU: all waves are of one age class for the issue
// arbiter (which favours older waves) and share one frame queue.
// waves per workgroup: 4 per SIMD at n_fft <= 1024 (<= 128 VGPRs: a twiddle takes one register pair, see
// cmul_tw) - except the n_fft 1024 variants with bands, which need 134 and stay at 3 per SIMD rather than
// spill (a kernel with scratch pays ~5 us more per dispatch); 2 when a wave keeps two frames in flight or at
// n_fft 2048.  (A/B at c2, both HBM-rotating and cache-resident: 16 waves = 12 waves within 0.3 %.)
#ifndef IRIS_W1024
#define IRIS_W1024 16
#endif
#ifndef IRIS_W2048
#define IRIS_W2048 0  // 0 = automatic: 12 where the registers allow it (see fused_waves), else 8
#endif
#ifndef IRIS_S2_WAVES
#define IRIS_S2_WAVES 8
#endif
// Round-5 occupancy experiment (A/B builds only, the defaults are the product; EXPERIMENTS.md): IRIS_EXP_WIN_LDS reads the
// window from the LDS staging area every frame instead of keeping it in 16 registers, IRIS_EXP_MELMODE1 (host_plan.h) takes
// the LDS band table instead of 20 register weights - together the n_fft 1024 kernel without epilogue fits 96 VGPRs = five
// waves per SIMD -, IRIS_WGS_PER_CU launches that many workgroups per CU (two of 10 waves: 1,024 threads cap one workgroup
// at 16 waves) for the two-kernel form
#ifndef IRIS_EXP_WIN_LDS
#define IRIS_EXP_WIN_LDS 0
#endif
#ifndef IRIS_WGS_PER_CU
#define IRIS_WGS_PER_CU 1
#endif
// frames go global -> registers up to this n_fft (log2); above it through LDS-DMA landing buffers.  Round 2: n_fft
// 2048 too - the prefetch targets the sample registers themselves (dead during the mel phase), so it costs no
// registers, frees 8 KB of landing buffer per wave, and the variant without bands and without the upper spectrum half
// then fits 168 VGPRs = 12 waves per CU (c5: 34.3 us LDS-DMA / 8 waves -> 32.5 direct / 8 -> 30.7 direct / 12).
#ifndef IRIS_DIRECT_MAX
#define IRIS_DIRECT_MAX 11
#endif
constexpr bool fused_direct(int log2n) { return IRIS_DIRECT_LOAD && log2n <= IRIS_DIRECT_MAX; }
// hi: the variant computes both halves of the untangle (n_fft 2048: 12 waves would spill, so 8)
#ifndef IRIS_FUSE2048_12
#define IRIS_FUSE2048_12 1
#endif
#define IRIS_FUSE12(fuse, mel_mode) (!(fuse) || (IRIS_FUSE2048_12 && (mel_mode) != 2 && (fuse) != 2))
// fuse: the variant applies min-max / log itself; its epilogue-only kernel arguments are loaded late (late_arg*), which
// keeps twelve waves at n_fft 2048 free of scratch - except with the global band table (mel_mode 2) and in the in-place
// form (fuse 2: the frame loop also keeps the output row addressing live), which stay at 8
// (bands: SpecAugment bands or - k_wav_to_mel_gain - FilterAugment gains: either costs the registers that decide the count)
constexpr int fused_waves(int log2n, int streams = 1, bool bands = false, bool hi = false, int fuse = 0, int mel_mode = 1) {
    return streams > 1 ? IRIS_S2_WAVES
                       : (log2n >= 11 ? ((IRIS_W2048 == 0 && fused_direct(11) && !bands && !hi && IRIS_FUSE12(fuse, mel_mode)) ? 12 : (IRIS_W2048 ? IRIS_W2048 : 8))
                                      : (log2n == 10 ? (bands ? 12 : IRIS_W1024) : 16));
}

struct FusedArgs {
    const float* wav;    // [B, C, L]
    float* out;          // [B, M, T, C]
    float* partial;      // [B, chunks_per_clip * waves, 2] (min, max) per wave of each chunk
    const float* sumsq;  // nullable [B, n_sq] partial sums of squares (normalize)
    int n_sq;
    const float* consts;  // per-lane constant block (ConstLayout)
    const int* band_lo;   // [M] first bin read by band m (clamped so lo + rows <= limit)
    const float* wband;   // [rows][M], 0.5 * W[lo + i][m]
    int rows;
    const int* t_bands;  // nullable [B, n_tb, 2]
    int n_tb;
    const int* f_bands;  // nullable [B, n_fb, 2]
    int n_fb;
    int B, C, L, T, hop, M;
    int chunk_frames, chunks_per_clip, n_chunks;
    int chunk_base, chunk_rem;  // T = chunks_per_clip * chunk_base + chunk_rem; the first chunk_rem chunks take one more
    // fp16-MFMA mel variant (k_fused_mfma.h): A fragments [tiles][8 k-steps][64 lanes][8 halfs], per tile
    // (first k-step, k-step count), bins staged per frame (multiple of 32)
    const void* wfrag;
    const int* tile_ks;
    int kb;
    // fused epilogue (FUSE): min-max / log applied inside the kernel.  The chunk's mel values are collected in an LDS
    // tile [M][pitch] at byte offset tile_off; the workgroups of a clip exchange their (min, max) through 8-byte
    // {epoch, value} granules slots[chunk][2] (agent-scope sc1 stores / loads; epoch = the plan's launch counter,
    // never 0); a wait that does not complete within ~2 s sets *status and fills the chunk with NaN
    unsigned long long* slots;
    unsigned* status;  // device address of the plan's host-resident status word
    unsigned long long timeout_ticks;
    unsigned epoch;
    int tile_off, pitch, do_minmax, do_log;
    int ablate;  // diagnostic only (IRIS_ABLATE): skip phases, results are wrong when non-zero
    unsigned long long* dbg;  // diagnostic only: [4] shader-clock / 100 MHz stamps of workgroup 0
};
// Arguments of the FilterAugment sibling k_wav_to_mel_gain: the same block first (the late_arg offsets hold), then the
// [B, M] per-sample mel-band gains.  A struct of its own: FusedArgs - and with it the kernarg layout of k_wav_to_mel - stays
// byte for byte what it was.
struct FusedGainArgs {
    FusedArgs a;
    const float* mel_gain;
};

// LDS-DMA of one frame.  Inline asm on purpose: hipcc drains an LDS-DMA it knows about
// (s_waitcnt vmcnt(0)) before the next DS access that might alias it, which would
// serialise the prefetch with the FFT.  Hidden from the compiler the DMA stays in flight
// across the whole frame computation; the kernel waits for it by hand right before it
// reads the frame buffer.  M0 = wave-uniform LDS byte address (saved / restored inside
// the statement); the instruction offset applies to the global and the LDS address alike.
//   dma_frame_x4: frame interior and 16-byte aligned -> N/256 pieces of 16 B per lane,
//                 source = SGPR base + lane*16 + imm
//   dma_frame_x1: any frame -> N/64 pieces of 4 B per lane with per-lane source
//                 addresses (reflect padding costs nothing extra)
template <int LOG2N>
__device__ __forceinline__ void dma_frame_x4(const float* src /*uniform*/, unsigned fbuf_lds, unsigned lane16) {
    static_assert(LOG2N >= 8 && LOG2N <= 11, "");
    unsigned keep;
    if constexpr (LOG2N == 8)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane16), "s"(src), "s"(fbuf_lds) : "memory");
    else if constexpr (LOG2N == 9)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane16), "s"(src), "s"(fbuf_lds) : "memory");
    else if constexpr (LOG2N == 10)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane16), "s"(src), "s"(fbuf_lds) : "memory");
    else {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane16), "s"(src), "s"(fbuf_lds) : "memory");
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %2\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(lane16), "s"(src + 1024), "s"(fbuf_lds + 4096) : "memory");
    }
}

__device__ __forceinline__ void glds4(const float* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

template <int LOG2N>
__device__ __forceinline__ void dma_frame_x1(const float* clip, int len, int start, unsigned fbuf_lds, int lane) {
    constexpr int N = 1 << LOG2N;
#pragma clang loop unroll(disable)
    for (int i = 0; i < N / 64; ++i)
        glds4(clip + reflect_idx(start + 64 * i + lane, len), __builtin_amdgcn_readfirstlane(fbuf_lds + 256 * i));
}

template <int LOG2N>
__device__ __forceinline__ void dma_frame(const float* clip, int len, int start, unsigned fbuf_lds, int lane) {
    constexpr int N = 1 << LOG2N;
    // clip/start are wave-uniform by construction; make that provable for the "s" operands
    const uint64_t u = reinterpret_cast<uint64_t>(clip + start);
    const uint32_t ulo = __builtin_amdgcn_readfirstlane((uint32_t)u);
    const uint32_t uhi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    const float* src = reinterpret_cast<const float*>(((uint64_t)uhi << 32) | ulo);
    start = __builtin_amdgcn_readfirstlane(start);
    if ((start >= 0) && (start + N <= len) && ((ulo & 15u) == 0))
        dma_frame_x4<LOG2N>(src, fbuf_lds, (unsigned)lane * 16u);
    else
        dma_frame_x1<LOG2N>(clip, len, start, fbuf_lds, lane);
}

typedef __attribute__((address_space(1))) unsigned long long gu64;

// Kernel arguments that only the epilogue reads, fetched from the kernarg segment WHERE THEY ARE USED: the compiler
// loads every field of the by-value argument struct at kernel entry and keeps it in scalar registers across the frame
// loop, which has none to spare (spilled SGPRs take a VGPR, and at n_fft 2048 that VGPR pushed mel weights to scratch).
// `asm volatile` keeps the load out of reach of loop-invariant code motion.
__device__ __forceinline__ unsigned late_arg32(unsigned offset) {
    unsigned v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "s"(offset) : "memory");
    return v;
}
__device__ __forceinline__ unsigned long long late_arg64(unsigned offset) {
    unsigned long long v;
    asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
                 : "=s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "s"(offset) : "memory");
    return v;
}
// The epilogue's arguments in ONE round trip to the scalar cache (five separate late loads, each with its own wait, stood
// on the critical path between a workgroup's last frame and its publication / write-out: ~0.1 us each)
struct LateEpilogueArgs {
    unsigned long long out, slots;
    unsigned epoch, do_minmax, do_log;
};
template <unsigned OFF_OUT, unsigned OFF_SLOTS, unsigned OFF_EPOCH, unsigned OFF_MM, unsigned OFF_LG>
__device__ __forceinline__ LateEpilogueArgs late_epilogue_args() {
    LateEpilogueArgs r;
    asm volatile("s_load_dwordx2 %0, %5, %6\n\t"
                 "s_load_dwordx2 %1, %5, %7\n\t"
                 "s_load_dword %2, %5, %8\n\t"
                 "s_load_dword %3, %5, %9\n\t"
                 "s_load_dword %4, %5, %10\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(r.out), "=&s"(r.slots), "=&s"(r.epoch), "=&s"(r.do_minmax), "=&s"(r.do_log)
                 : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(OFF_OUT), "n"(OFF_SLOTS), "n"(OFF_EPOCH), "n"(OFF_MM), "n"(OFF_LG)
                 : "memory");
    return r;
}
#define LATE32(field) late_arg32((unsigned)offsetof(FusedArgs, field))
#define LATE64(field) late_arg64((unsigned)offsetof(FusedArgs, field))
constexpr unsigned long long kEpilogueTimeoutTicks = 200000000ull;  // s_memrealtime runs at 100 MHz: 2 s

// K1 itself lives in k_fused_kernel.h, expanded twice: k_wav_to_mel, and k_wav_to_mel_gain (FilterAugment)
#define IRIS_K_GAIN 0
#include "k_fused_kernel.h"
#undef IRIS_K_GAIN
#define IRIS_K_GAIN 1
#include "k_fused_kernel.h"
#undef IRIS_K_GAIN
