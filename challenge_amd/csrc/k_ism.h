// k_ism.h -- shoebox room simulation (Allen & Berkley 1979; what pyroomacoustics and gpuRIR compute): the image-source room
// impulse responses of a ragged set of voices, every voice with its own room, source, microphones, wall reflection coefficient
// and tap count, in one launch.  Part of the single translation unit iris_frontend.hip; the C entry point iris_ism_rir and its
// argument checks are in host_ops.h.
//
// Per record (iris_ism_src): images n in [-N_a, N_a]^3, p in {0, 1}^3 at x_a = (1 - 2 p_a) s_a + 2 n_a L_a with
// e = sum_a |n_a - p_a| + |n_a| reflections; per microphone the distance d, tau = d fs / c samples, t = tau - tau_min + W and
//     h[c][k] = sum_images beta^e (d_min / d) w(k - t),    w(x) = sinc(x) 0.5 (1 + cos(pi x / W)) for |x| < W, else 0
// (tau_min, d_min: the smallest direct delay over the channels of the voice and its distance; W = 16).  N_a =
// floor(D / (2 L_a)) + 1 with D = c (tau_min + K) / fs holds every image that can reach a tap below K; images with
// t - W >= K - 1 are skipped.
//   blockIdx.x = record.  One 256-thread workgroup takes the channels in turn: the K taps sit in LDS as 64-bit fixed-point
//   accumulators (32 KiB at K = 4096; with the reduction buffer 34.3 KiB: 4 workgroups, 16 waves, per CU), the threads stride
//   over the linear image index, cull by distance before touching LDS, and add each contribution a w (|a w| <= 1) rounded to
//   a multiple of 2^-32 with an integer LDS atomic (ds_add_u64).  Integer addition is order-free, so the taps are bitwise
//   reproducible whatever the order the waves arrive in.
// Precision: positions, d, tau, t, floor(t) and the fraction are double (at t ~ 4096 an fp32 delay would be 2.4e-4 samples
// off), the fraction folded into g in [-0.5, 0.5] about the nearest tap, and the gain is formed in double and rounded once; the
// sinc, the window and the products are fp32: sin(pi (m - g)) = -(-1)^m sin(pi g) - one sine per image serves its 2 W taps -
// and cos(pi (m - g) / W) by the angle-addition formula from one sine / cosine pair per image and a 33-entry table.
// normalize: every channel of a voice times the same g = 1 / sqrt(mean_c sum_k h^2) (sum of squares in double, a fixed
// reduction tree; an all-zero response is left as it is), so the level difference between the channels is kept.
#pragma once

constexpr int kIsmThreads = 256;
constexpr int kIsmW = 16;           // half width of the fractional-delay filter, taps
constexpr int kIsmMaxTaps = 4096;   // taps of the LDS accumulator
constexpr double kIsmSound = 343.0; // speed of sound, m / s

static_assert(sizeof(iris_ism_src) == 72 + 24 * IRIS_ISM_MAX_CHAN, "iris_ism_src: pointer, 7 doubles, 2 ints, the microphones");

struct IsmGeom {
    double tau_min, d_min;   // the nearest microphone's direct delay (samples) and distance (m)
    double n_max[3];         // N_a, as doubles (they are checked against 2^31 before they become ints)
    double images;           // (2 N_x + 1)(2 N_y + 1)(2 N_z + 1) 8
};

// the lattice of one record; the same statements on the host (the checks) and in the kernel
__host__ __device__ inline IsmGeom ism_geometry(const iris_ism_src& r, int channels, double fs) {
    IsmGeom g;
    g.tau_min = 0, g.d_min = 0;
    for (int c = 0; c < channels; ++c) {
        const double dx = r.src[0] - r.mic[c][0], dy = r.src[1] - r.mic[c][1], dz = r.src[2] - r.mic[c][2];
        const double d = sqrt(dx * dx + dy * dy + dz * dz), tau = d * fs / kIsmSound;
        if (c == 0 || tau < g.tau_min) g.tau_min = tau, g.d_min = d;
    }
    const double reach = kIsmSound * (g.tau_min + r.n_taps) / fs;
    g.images = 8;
    for (int a = 0; a < 3; ++a) {
        g.n_max[a] = floor(reach / (2.0 * r.room[a])) + 1.0;
        g.images *= 2.0 * g.n_max[a] + 1.0;
    }
    return g;
}

__global__ __launch_bounds__(kIsmThreads) void k_ism_rir(const iris_ism_src* __restrict__ table, int channels, int max_taps,
                                                         double fs, int normalize) {
    __shared__ unsigned long long acc[kIsmMaxTaps];   // tap k as a signed multiple of 2^-32 (two's complement)
    __shared__ double red[kIsmThreads];
    __shared__ float ct[2 * kIsmW + 1], st[2 * kIsmW + 1];   // cos / sin (pi m / W), m = -W .. W
    const iris_ism_src& d = table[blockIdx.x];
    const int K = d.n_taps, tid = threadIdx.x;
    // a record the checks of iris_ism_rir would have refused (the uploaded table is not the checked one): nothing written
    if (K < 1 || K > max_taps || K > kIsmMaxTaps || !d.dst || channels < 1 || channels > IRIS_ISM_MAX_CHAN) return;
    const IsmGeom g = ism_geometry(d, channels, fs);
    if (!(g.images <= 2147483647.0) || !(g.d_min > 0)) return;
    const unsigned wx = 2u * (unsigned)g.n_max[0] + 1u, wy = 2u * (unsigned)g.n_max[1] + 1u;
    const int nx0 = (int)g.n_max[0], ny0 = (int)g.n_max[1], nz0 = (int)g.n_max[2];
    const unsigned images = (unsigned)g.images;
    const double beta = d.beta, sx = d.src[0], sy = d.src[1], sz = d.src[2], lx = d.room[0], ly = d.room[1], lz = d.room[2];
    if (tid <= 2 * kIsmW) {
        ct[tid] = cospif((float)(tid - kIsmW) * (1.0f / kIsmW));
        st[tid] = sinpif((float)(tid - kIsmW) * (1.0f / kIsmW));
    }
    double sumsq = 0;   // this thread's share of sum_c sum_k h^2, in the order it writes the taps
    for (int c = 0; c < channels; ++c) {
        __syncthreads();   // the previous channel has been written out (and the table above is in place)
        for (int k = tid; k < K; k += kIsmThreads) acc[k] = 0;
        __syncthreads();
        const double mx = d.mic[c][0], my = d.mic[c][1], mz = d.mic[c][2];
        for (unsigned i = tid; i < images; i += kIsmThreads) {
            const unsigned par = i & 7u, q = i >> 3;
            const int px = par & 1, py = (par >> 1) & 1, pz = par >> 2;
            const int nx = (int)(q % wx) - nx0, ny = (int)((q / wx) % wy) - ny0, nz = (int)(q / (wx * wy)) - nz0;
            const double dx = (1 - 2 * px) * sx + 2.0 * nx * lx - mx, dy = (1 - 2 * py) * sy + 2.0 * ny * ly - my;
            const double dz = (1 - 2 * pz) * sz + 2.0 * nz * lz - mz;
            const double dist = sqrt(dx * dx + dy * dy + dz * dz);
            const double t = dist * fs / kIsmSound - g.tau_min + kIsmW;
            if (t - kIsmW >= K - 1) continue;   // no tap below K under its window
            unsigned e = (unsigned)(abs(nx - px) + abs(nx) + abs(ny - py) + abs(ny) + abs(nz - pz) + abs(nz));
            double gain = 1.0, b = beta;        // beta^e by squaring (beta = 0: 1 for the direct image, else 0)
            for (; e; e >>= 1, b *= b)
                if (e & 1) gain *= b;
            const float a = (float)(gain * g.d_min / dist);
            if (a == 0.f) continue;
            const double fl = floor(t);
            double frac = t - fl;
            int k0 = (int)fl;                   // 0 <= t < K + W: it fits
            if (frac > 0.5) frac -= 1.0, k0 += 1;
            const float gf = (float)frac;
            const float s = sinpif(gf), cw = cospif(gf * (1.0f / kIsmW)), sw = sinpif(gf * (1.0f / kIsmW));
#pragma unroll 1
            for (int m = -kIsmW; m <= kIsmW; ++m) {
                const int k = k0 + m;
                const float x = (float)m - gf;
                if (k < 0 || k >= K || !(fabsf(x) < (float)kIsmW)) continue;
                const float sinc = x == 0.f ? 1.0f : ((m & 1) ? s : -s) / (3.14159265358979323846f * x);
                const float win = 0.5f * (1.0f + fmaf(ct[m + kIsmW], cw, st[m + kIsmW] * sw));
                const float v = a * (sinc * win);
                const long long fixed = __double2ll_rn((double)v * 4294967296.0);
                atomicAdd(&acc[k], (unsigned long long)fixed);
            }
        }
        __syncthreads();
        float* __restrict__ row = d.dst + (size_t)c * max_taps;
        for (int k = tid; k < K; k += kIsmThreads) {
            const float h = (float)((double)(long long)acc[k] * (1.0 / 4294967296.0));
            row[k] = h;
            sumsq += (double)h * (double)h;
        }
    }
    if (!normalize) return;
    red[tid] = sumsq;
    __syncthreads();
    for (int step = kIsmThreads / 2; step > 0; step >>= 1) {   // a fixed tree: the same bits every run
        if (tid < step) red[tid] += red[tid + step];
        __syncthreads();
    }
    const double energy = red[0] / channels;
    if (!(energy > 0)) return;
    const float scale = (float)(1.0 / sqrt(energy));
    for (int c = 0; c < channels; ++c) {
        float* __restrict__ row = d.dst + (size_t)c * max_taps;
        for (int k = tid; k < K; k += kIsmThreads) row[k] *= scale;   // the thread's own stores: no fence needed
    }
}
