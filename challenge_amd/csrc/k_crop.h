// k_crop.h -- training windows cut from LABELLED RECORDINGS on the device: which window of which recording (one small
// launch, iris_crop_draw) and the gather of the windows and their frame labels into a batch (one launch,
// iris_crop_windows).  Part of the single translation unit iris_frontend.hip; the generator is k_draw.h's.
//
// The draw, identical here and in tests/crop_ref.py (the NumPy restatement).  Recording i of n has
// n_pos[i] = max((len[i] - L) / hop, 0) + 1 window positions (integer division, L = (n_frame - 1) * hop); the caller passes
// their int64 prefix sums prefix[0 .. n] (prefix[0] = 0, prefix[n] = total).  Per sample b:
//   1. words   r = philox4x32_10(call counter lo, hi, b * 64 + 0, kDrawCrop; key = seed lo, hi)
//   2. w64     = (r.x << 32) | r.y                      (word x is the high half)
//   3. u       = high 64 bits of the 128-bit product w64 * total: uniform on [0, total), bias < total / 2^64
//   4. i       = the recording with prefix[i] <= u < prefix[i + 1] (binary search), q = u - prefix[i]
//   5. draws[b] = (i, q): the window starts at sample q * hop of recording i
// so every window of the corpus is equally likely.  The call counter is state[0] of a DEVICE uint64[1] of this function's
// own (zero-initialised once by the caller) and is advanced by the kernel: a captured launch replays with fresh draws.
//
// The gather.  Sample s of channel c of window b is sample q * hop + s of the recording's channel row where that index is
// below len, and exactly 0.0f otherwise WHATEVER the memory behind the row holds (it is never read).  One workgroup copies
// kCropChunk samples of one (sample, channel) row: a streaming copy, so a row whose source and destination are both
// 16-byte aligned (and L % 4 == 0) moves as dwordx4 loads and stores, four independent ones in flight per lane; the last
// float4 of a row that straddles len is assembled from scalar loads of the samples below len.  Every other row takes the
// scalar path (coalesced dword accesses).  The choice is per row, hence wave-uniform.  Label entry (f, k) of window b is
// the NUMBER of the recording's events (class, start, end) with class == k and start <= q + f < end (overlaps add up, as
// eval.second2frame does); the label rows are further rows of the same grid.  A draw that names no recording
// (i outside [0, n), q < 0) gives a zero window and zero labels.  No atomics, no allocation, no synchronisation.
#pragma once

constexpr int kCropThreads = 256;
constexpr int kCropVecPerLane = 4;                                  // independent 16-byte loads in flight per lane
constexpr int kCropChunk = kCropThreads * kCropVecPerLane * 4;      // samples of a row per workgroup (16 KiB)
// a recording's address comes out of the record table, i.e. out of memory: said to be global memory here, so that the rows are
// read with global_load (a pointer of unknown address space is read with flat_load)
typedef __attribute__((address_space(1))) const float crop_gfloat;
typedef float crop_float4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const crop_float4 crop_gfloat4;

__global__ __launch_bounds__(kCropThreads) void k_crop_windows(const iris_crop_rec* __restrict__ recs, int n,
                                                                const int32_t* __restrict__ events,
                                                                const int32_t* __restrict__ draws, int batch, int channels, int L,
                                                                int hop, int n_frame, int n_classes, float* __restrict__ wav_out,
                                                                float* __restrict__ y_out) {
    const int row = blockIdx.y, wav_rows = batch * channels;
    const int b = row < wav_rows ? row / channels : row - wav_rows;
    const int i = draws[2 * b], q = draws[2 * b + 1];
    const bool known = i >= 0 && i < n && q >= 0;
    if (row >= wav_rows) {  // label rows: n_frame * n_classes counts of window b
        const int total = n_frame * n_classes;
        const int ev_first = known ? recs[i].ev_first : 0, ev_count = known ? recs[i].ev_count : 0;
        float* y = y_out + (size_t)b * total;
        for (int e = blockIdx.x * kCropThreads + threadIdx.x; e < total; e += gridDim.x * kCropThreads) {
            const int f = e / n_classes, k = e - f * n_classes;
            const long long t = (long long)q + f;
            int count = 0;
            for (int j = 0; j < ev_count; ++j) {
                const int32_t* ev = events + 3 * (size_t)(ev_first + j);
                count += (ev[0] == k && (long long)ev[1] <= t && t < (long long)ev[2]) ? 1 : 0;
            }
            y[e] = (float)count;
        }
        return;
    }
    const int c = row - b * channels;
    const int s0 = blockIdx.x * kCropChunk;  // first sample of this workgroup's chunk (< L by the grid's size)
    float* dst = wav_out + (size_t)row * L;
    const long long first = (long long)q * hop;                              // the window's first sample in the recording
    const long long len = known ? (long long)recs[i].len : 0;                // samples of the row that exist
    crop_gfloat* src = (crop_gfloat*)(known ? recs[i].base + (long long)c * recs[i].row_stride + first : nullptr);
    const long long avail = known ? len - first : 0;                         // window samples below this are copied
    const bool vec = (L & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    if (vec) {
        float4 v[kCropVecPerLane];
#pragma unroll
        for (int u = 0; u < kCropVecPerLane; ++u) {
            const int s = s0 + 4 * (u * kCropThreads + threadIdx.x);
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s < L) {
                if ((long long)s + 4 <= avail) {
                    const crop_float4 t = *(crop_gfloat4*)(src + s);
                    v[u] = make_float4(t.x, t.y, t.z, t.w);
                } else {  // the float4 that straddles len: only the samples below it are read
                    if ((long long)s + 0 < avail) v[u].x = src[s];
                    if ((long long)s + 1 < avail) v[u].y = src[s + 1];
                    if ((long long)s + 2 < avail) v[u].z = src[s + 2];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kCropVecPerLane; ++u) {
            const int s = s0 + 4 * (u * kCropThreads + threadIdx.x);
            if (s < L) *reinterpret_cast<float4*>(dst + s) = v[u];
        }
        return;
    }
    const int end = min(s0 + kCropChunk, L);
    for (int s = s0 + threadIdx.x; s < end; s += kCropThreads) dst[s] = (long long)s < avail ? src[s] : 0.f;
}

__global__ __launch_bounds__(256) void k_crop_draw(const long long* __restrict__ prefix, int n, int batch, uint32_t k0, uint32_t k1,
                                                   unsigned long long* state, int32_t* __restrict__ draws) {
    const unsigned long long ctr = state[0];
    const uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32);
    const long long total = prefix[n];
    __syncthreads();  // every thread has read the state before thread 0 advances it
    for (int b = threadIdx.x; b < batch; b += blockDim.x) {
        const Philox4 r = philox4x32_10(c0, c1, (uint32_t)b * 64u, kDrawCrop, k0, k1);
        const unsigned long long w = ((unsigned long long)r.x << 32) | r.y;
        const long long u = total > 0 ? (long long)__umul64hi(w, (unsigned long long)total) : 0;
        int lo = 0, hi = n;  // prefix[lo] <= u < prefix[hi]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (prefix[mid] <= u) lo = mid;
            else hi = mid;
        }
        draws[2 * b] = lo;
        draws[2 * b + 1] = (int32_t)(u - prefix[lo]);
    }
    if (threadIdx.x == 0) state[0] = ctr + 1;
}

extern "C" int iris_crop_windows(const iris_crop_rec* recs_dev, int n, const int32_t* events_dev, const int32_t* draws_dev, int batch,
                                 int channels, int hop, int n_frame, int n_classes, float* wav_out, float* y_out, void* stream) {
    if (batch < 0) return fail(IRIS_E_INVALID, "iris_crop_windows: batch = %d is negative", batch);
    if (n <= 0) return fail(IRIS_E_INVALID, "iris_crop_windows: n = %d recordings", n);
    if (hop <= 0 || n_frame < 2 || n_classes <= 0)
        return fail(IRIS_E_INVALID, "iris_crop_windows: hop = %d, n_classes = %d must be positive and n_frame = %d at least 2", hop,
                    n_classes, n_frame);
    if (channels != 1 && channels != 2) return fail(IRIS_E_INVALID, "iris_crop_windows: channels = %d (1 or 2)", channels);
    if (batch > 0 && (!recs_dev || !events_dev || !draws_dev || !wav_out || !y_out))
        return fail(IRIS_E_INVALID, "iris_crop_windows: NULL argument");
    if ((long long)(n_frame - 1) * hop > 2147483647ll - kCropChunk || (long long)n_frame * n_classes > 2147483647ll)
        return fail(IRIS_E_UNSUPPORTED, "iris_crop_windows: a window of (n_frame - 1) * hop samples or n_frame * n_classes labels exceeds 2^31");
    if ((long long)batch * (channels + 1) > 65535)
        return fail(IRIS_E_UNSUPPORTED, "iris_crop_windows: batch * (channels + 1) = %lld rows exceed the grid's 65535",
                    (long long)batch * (channels + 1));
    if (batch == 0) return IRIS_OK;
    const int L = (n_frame - 1) * hop;
    dim3 grid((unsigned)((L + kCropChunk - 1) / kCropChunk), (unsigned)(batch * (channels + 1)));
    k_crop_windows<<<grid, kCropThreads, 0, (hipStream_t)stream>>>(recs_dev, n, events_dev, draws_dev, batch, channels, L, hop, n_frame,
                                                                  n_classes, wav_out, y_out);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}

extern "C" int iris_crop_draw(const int64_t* prefix_dev, int n, int batch, uint64_t seed, uint64_t* state_dev, int32_t* draws_out,
                              void* stream) {
    if (batch < 0) return fail(IRIS_E_INVALID, "iris_crop_draw: batch = %d is negative", batch);
    if (n <= 0) return fail(IRIS_E_INVALID, "iris_crop_draw: n = %d recordings", n);
    if (batch > 0 && (!prefix_dev || !state_dev || !draws_out)) return fail(IRIS_E_INVALID, "iris_crop_draw: NULL argument");
    if (batch > (1 << 25)) return fail(IRIS_E_UNSUPPORTED, "iris_crop_draw: batch = %d exceeds 2^25 (the counter holds sample * 64 + column)", batch);
    if (batch == 0) return IRIS_OK;
    k_crop_draw<<<1, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const long long*>(prefix_dev), n, batch, (uint32_t)seed,
                                                    (uint32_t)(seed >> 32), reinterpret_cast<unsigned long long*>(state_dev), draws_out);
    HIP_TRY(hipGetLastError());
    return IRIS_OK;
}
