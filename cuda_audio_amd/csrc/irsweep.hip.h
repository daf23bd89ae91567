// irsweep.hip.h — an impulse response from a recorded exponential sine sweep (mc_load_ir_sweep; Farina's method): the
// recording is correlated with the sweep under a 6 dB/octave envelope on the device.  No reference equivalent: the reference
// convolves with the frames of a WAV file that some other program deconvolved.
//
// include/mcconv.h has the definition and tests/ir_sweep_np.py states it in float64:
//   s64[n]  = amplitude w(n) sin(phi(n)), phi(n) = (2 pi f1 Ls / rate) expm1(n / Ls), Ls = (N - 1) / ln(f2 / f1);
//   u[j]    = (4 f2 / (amplitude^2 Ls rate)) s64[j] exp(-(N - 1 - j) / Ls);
//   h_c[m]  = sum over j = 0 .. N - 1, ascending, of u[j] (double) r_c[m + j + offset], r = 0 outside [0, M),
//             one double accumulator per output updated by fma, rounded to float once.
// swp_s64 and swp_u are the one statement of the sweep: mc_sweep_generate (host) and k_sweep_weights (device) both call them.
//
// k_sweep_corr is the hot path, 2 F N double fma.  SWP_T = 2048 outputs per workgroup, SWP_J = 256 weights per LDS tile.
// A thread owns SWP_R = 8 consecutive outputs and keeps the 8 frames of the recording that the current weight meets in
// registers (a window that moves one frame per weight; the loop is unrolled by 8 so that the move is a renaming).  Per
// weight a thread reads u[j] (8 bytes, one address for the whole workgroup: a broadcast) and one new frame (16 bytes: the tile
// holds L and R already converted to double, which is exact) and does 16 fma: 2 LDS reads per 16 fma, 1/8 per fma.  A lane's
// frames lie 8 apart, a stride of 128 bytes that would put every lane of a read's group on two banks' worth of addresses;
// the tile is therefore skewed by one frame in eight, slot(i) = i + i / 8.  Lane t at i = 8 t + c reads slot 9 t + c + c / 8,
// c the same in every lane, and 9 t covers the sixteen 16-byte columns of the LDS once in each lane group of ds_read_b128.
// The tile of the recording (SWP_T + SWP_J frames) is loaded as float2 with everything outside [0, M) filled with zeros, never
// read from memory; a tile that misses the recording altogether is skipped, which changes no bit (fma(u, 0, h) == h).
// Weights past N - 1 in the last group of 8 are zero: up to 7 terms u = 0 times a sample are added, exact for a finite
// recording.  No atomics and no split over j: every output is summed in ascending j by one thread, so the bits do not depend
// on the grid.  The outputs are stored as float2 (the destination is 8-byte aligned, no more, as k_synth's).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/mcconv.h"
#include "owned.h"

constexpr int SWP_THREADS = 256;
constexpr int SWP_R = 8;                                // consecutive outputs per thread
constexpr int SWP_T = SWP_THREADS * SWP_R;              // outputs per workgroup
constexpr int SWP_J = 256;                              // weights per tile
constexpr int SWP_SPAN = SWP_T + SWP_J;                 // frames of the recording per tile (the last 1 + 7 feed zero weights at most)
constexpr int SWP_SLOTS = SWP_SPAN + SWP_SPAN / SWP_R;  // with the skew
constexpr uint64_t SWP_MAX_N = 1ull << 22;
constexpr uint64_t SWP_MAX_FRAMES = 1ull << 24;  // M, F and |offset|
constexpr uint64_t SWP_MAX_WORK = 1ull << 40;    // F * N of one correlation launch

// a checked mc_sweep, every float field as double
struct SweepPlan {
    uint64_t N, fade_in, fade_out;
    double Ls;    // (N - 1) / ln(f2 / f1)
    double K;     // 2 pi f1 Ls / rate
    double A;     // amplitude
    double norm;  // 4 f2 / (A^2 Ls rate)
};

// the unrounded sweep, s64[n], n < N
__host__ __device__ inline double swp_s64(const SweepPlan& p, uint64_t n) {
    double w = 1.0;
    if (n < p.fade_in) w *= 0.5 * (1.0 - cos(M_PI * ((double)n + 1.0) / ((double)p.fade_in + 1.0)));
    if (n >= p.N - p.fade_out) {
        const double k = (double)(n - (p.N - p.fade_out));
        w *= 0.5 * (1.0 + cos(M_PI * (k + 1.0) / ((double)p.fade_out + 1.0)));
    }
    return p.A * w * sin(p.K * expm1((double)n / p.Ls));
}

// the deconvolution weight u[j], j < N
__host__ __device__ inline double swp_u(const SweepPlan& p, uint64_t j) {
    return p.norm * swp_s64(p, j) * exp(-(double)(p.N - 1 - j) / p.Ls);
}

__global__ __launch_bounds__(SWP_THREADS) void k_sweep_weights(double* __restrict__ u, SweepPlan p) {
    const uint64_t j = (uint64_t)blockIdx.x * SWP_THREADS + threadIdx.x;
    if (j < p.N) u[j] = swp_u(p, j);
}

__device__ inline int swp_slot(int i) { return i + (i >> 3); }

// x[m] = h[m] for m < F.  r: M frames; u: N weights; gridDim.x * SWP_T >= F.
__global__ __launch_bounds__(SWP_THREADS) void k_sweep_corr(const float2* __restrict__ r, uint64_t M, const double* __restrict__ u, uint64_t N,
                                                            int64_t offset, float2* __restrict__ x, uint64_t F) {
    __shared__ double su[SWP_J];
    __shared__ double2 sr[SWP_SLOTS];
    const int t = threadIdx.x;
    const uint64_t m0 = (uint64_t)blockIdx.x * SWP_T;
    double hL[SWP_R], hR[SWP_R];
#pragma unroll
    for (int k = 0; k < SWP_R; k++) hL[k] = hR[k] = 0.0;
    for (uint64_t j0 = 0; j0 < N; j0 += SWP_J) {
        const int64_t g0 = (int64_t)(m0 + j0) + offset;  // the recording's frame at the tile's entry 0
        if (g0 >= (int64_t)M || g0 + SWP_SPAN <= 0) continue;  // (the same in every thread of the workgroup)
        __syncthreads();  // the tile before this one has been read
        su[t] = j0 + t < N ? u[j0 + t] : 0.0;
        for (int i = t; i < SWP_SPAN; i += SWP_THREADS) {
            const int64_t g = g0 + i;
            const float2 v = g >= 0 && g < (int64_t)M ? r[g] : make_float2(0.f, 0.f);
            sr[swp_slot(i)] = make_double2((double)v.x, (double)v.y);
        }
        __syncthreads();
        double2 w[SWP_R];  // w[(k + j) % 8] = the tile's frame 8 t + k + j
#pragma unroll
        for (int k = 0; k < SWP_R; k++) w[k] = sr[9 * t + k];
        const int jn = N - j0 < (uint64_t)SWP_J ? (int)(N - j0) : SWP_J;
        for (int jb = 0; jb < jn; jb += SWP_R) {
#pragma unroll
            for (int jj = 0; jj < SWP_R; jj++) {
                const double uj = su[jb + jj];
#pragma unroll
                for (int k = 0; k < SWP_R; k++) {
                    hL[k] = fma(uj, w[(k + jj) & (SWP_R - 1)].x, hL[k]);
                    hR[k] = fma(uj, w[(k + jj) & (SWP_R - 1)].y, hR[k]);
                }
                w[jj] = sr[9 * t + jb + jj + SWP_R + ((jb + jj + SWP_R) >> 3)];  // frame 8 t + jb + jj + 8 <= SWP_SPAN - 1
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SWP_R; k++) {
        const uint64_t m = m0 + (uint64_t)(SWP_R * t + k);
        if (m < F) x[m] = make_float2((float)hL[k], (float)hR[k]);
    }
}

// Every field of a sweep, in field order, checked without touching an engine or HIP; the message names the field.  Null when
// it is good.
inline const char* swp_check(const mc_sweep* s) {
    static thread_local char msg[200];
    if (!s) return "null sweep";
    if (s->struct_size != sizeof(mc_sweep)) return "mc_sweep struct_size mismatch";
    msg[0] = 0;
    if (s->rate < 8000 || s->rate > 384000)
        std::snprintf(msg, sizeof(msg), "rate %u outside [8000, 384000]", s->rate);
    else if (s->frames < 2 || s->frames > SWP_MAX_N)
        std::snprintf(msg, sizeof(msg), "frames %llu outside [2, %llu]", (unsigned long long)s->frames, (unsigned long long)SWP_MAX_N);
    else if (!(std::isfinite(s->f1_hz) && s->f1_hz >= 1.f))
        std::snprintf(msg, sizeof(msg), "f1_hz %g must be finite and >= 1", (double)s->f1_hz);
    else if (!(std::isfinite(s->f2_hz) && s->f2_hz > s->f1_hz && (double)s->f2_hz <= 0.5 * (double)s->rate))
        std::snprintf(msg, sizeof(msg), "f2_hz %g outside (f1_hz %g, half the rate %g]", (double)s->f2_hz, (double)s->f1_hz, 0.5 * (double)s->rate);
    else if (!(std::isfinite(s->amplitude) && s->amplitude > 0.f))
        std::snprintf(msg, sizeof(msg), "amplitude %g must be finite and > 0", (double)s->amplitude);
    else if ((uint64_t)s->fade_in + (uint64_t)s->fade_out > s->frames)
        std::snprintf(msg, sizeof(msg), "fade_in %u + fade_out %u above frames %llu", s->fade_in, s->fade_out, (unsigned long long)s->frames);
    else if (s->reserved)
        std::snprintf(msg, sizeof(msg), "reserved %u must be 0", s->reserved);
    return msg[0] ? msg : nullptr;
}

// M, F, offset and F * N of a load from a checked sweep, in that order; null when they are good
inline const char* swp_check_load(const mc_sweep* s, uint64_t M, uint64_t F, int64_t offset) {
    static thread_local char msg[200];
    msg[0] = 0;
    const int64_t lim = (int64_t)SWP_MAX_FRAMES;
    if (M < 1 || M > SWP_MAX_FRAMES)
        std::snprintf(msg, sizeof(msg), "frames %llu of the recording outside [1, %llu]", (unsigned long long)M, (unsigned long long)SWP_MAX_FRAMES);
    else if (F < 1 || F > SWP_MAX_FRAMES)
        std::snprintf(msg, sizeof(msg), "ir_frames %llu outside [1, %llu]", (unsigned long long)F, (unsigned long long)SWP_MAX_FRAMES);
    else if (offset < -lim || offset > lim)
        std::snprintf(msg, sizeof(msg), "offset %lld outside [-%lld, %lld]", (long long)offset, (long long)lim, (long long)lim);
    else if (F * s->frames > SWP_MAX_WORK)  // (F <= 2^24 and N <= 2^22: the product fits)
        std::snprintf(msg, sizeof(msg), "ir_frames %llu * sweep frames %llu above %llu", (unsigned long long)F, (unsigned long long)s->frames,
                      (unsigned long long)SWP_MAX_WORK);
    return msg[0] ? msg : nullptr;
}

inline SweepPlan swp_plan(const mc_sweep& s) {
    SweepPlan p{};
    p.N = s.frames;
    p.fade_in = s.fade_in;
    p.fade_out = s.fade_out;
    const double f1 = (double)s.f1_hz, f2 = (double)s.f2_hz, rate = (double)s.rate;
    p.Ls = (double)(p.N - 1) / std::log(f2 / f1);
    p.K = 2.0 * M_PI * f1 * p.Ls / rate;
    p.A = (double)s.amplitude;
    p.norm = 4.0 * f2 / (p.A * p.A * p.Ls * rate);
    return p;
}

// the source of mc_load_ir_sweep as load_ir takes it: a checked sweep and the recording on the host
struct SweepSource {
    SweepPlan plan;
    const float* lr;  // M interleaved frames
    uint64_t M, F;
    int64_t offset;
};

// The F frames of the deconvolved IR into d_x (8-byte aligned, F float2), on `stream`.  The recording and the weight table
// live in two temporary buffers that the caller frees once the stream has finished with them (d_rec, d_u).
inline hipError_t swp_generate(hipStream_t stream, const SweepSource& s, float2* d_x, DevArray<float2>& d_rec, DevArray<double>& d_u) {
    hipError_t er = d_rec.alloc(s.M);
    if (er == hipSuccess) er = d_u.alloc(s.plan.N);
    if (er == hipSuccess) er = hipMemcpy(d_rec, s.lr, sizeof(float2) * s.M, hipMemcpyHostToDevice);
    if (er != hipSuccess) return er;
    hipLaunchKernelGGL(k_sweep_weights, dim3((unsigned)((s.plan.N + SWP_THREADS - 1) / SWP_THREADS)), dim3(SWP_THREADS), 0, stream, d_u, s.plan);
    hipLaunchKernelGGL(k_sweep_corr, dim3((unsigned)((s.F + SWP_T - 1) / SWP_T)), dim3(SWP_THREADS), 0, stream, d_rec, s.M, d_u, s.plan.N, s.offset,
                       d_x, s.F);
    return hipGetLastError();
}
