// resample.hip.h — sample-rate conversion of an impulse response on load (mc_load_ir_resampled).  No reference
// equivalent: the reference hands WAV frames to its transforms at whatever rate they were recorded.
//
// An IR at `src` Hz goes into a session at `dst` Hz (g = gcd, p = dst / g, q = src / g, s = min(1, dst / src)):
// output frame m sits at input time x_m = m q / p, kept exact as n0 = (m q) div p and frac = ((m q) mod p) / p, and
//     y[m] = (src / dst) * sum_n x[n] k(x_m - n),
//     k(d) = rho s sinc(rho s d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta)  for |d| < W = Z / s, 0 otherwise,
// Z = 64 zero crossings, beta = 9, rho = 0.955.  The src / dst factor keeps sum h (and the wet level of a steady tone):
// a converted IR has dst / src times as many taps.  Pre-ringing before m = 0 is dropped; ceil(frames p / q) frames.
// tests/resample_np.py states the same in float64.
//
// Output m reads input frames n0 - Wi + 1 .. n0 + Wi (Wi = ceil(W), L = 2 Wi taps): tap j at distance d = Wi - 1 - j + frac.
// One thread per output frame (float2 = L, R), accumulated in double; a 256-thread workgroup stages its input window
// (about 256 q / p + L frames) in LDS and reduces its outputs' share of the four sums mc_ir_info reports.  Coefficients come
// from a per-phase table built on the device in double when it is small and no larger than the output, otherwise each lane
// evaluates them in double (ratios such as 44100 -> 47999).  The table is stored tap-major, [L][p]: the lanes of a wave sit
// at phases q apart (mod p), so one tap of a wave's 64 outputs falls within a row of p floats instead of 64 rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "owned.h"

constexpr int RS_Z = 64;                  // zero crossings of the sinc on each side (at s = 1)
constexpr double RS_BETA = 9.0;           // Kaiser window
constexpr double RS_RHO = 0.955;          // passband fraction of the new Nyquist frequency
constexpr uint32_t RS_MIN_RATE = 8000, RS_MAX_RATE = 384000;
constexpr int RS_THREADS = 256;
constexpr int RS_STAGE = 2048;            // frames of input window staged per workgroup (16 KB of LDS); wider windows read global memory
constexpr uint64_t RS_TABLE_MAX = 1u << 21;  // coefficients of the per-phase table (8 MB)

struct RsGeom {
    uint64_t p, q;
    int Wi, L;          // ceil(W), taps per output frame
    double W, a, gain;  // half-width (input frames), rho * s, src / dst
    double inv_i0b;     // 1 / I0(beta)
};

__host__ __device__ inline double rs_i0(double x) {
    // modified Bessel function of the first kind, order 0: sum ((x / 2)^2)^k / (k!)^2 (x <= 9 here: 30-odd terms)
    const double t = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 80; k++) {
        term *= t / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

__host__ __device__ inline double rs_coef(const RsGeom& g, double d) {
    if (fabs(d) >= g.W) return 0.0;
    const double x = g.a * d, px = M_PI * x;
    const double sinc = x == 0.0 ? 1.0 : sin(px) / px;
    const double u = d / g.W;
    return g.gain * g.a * sinc * rs_i0(RS_BETA * sqrt(1.0 - u * u)) * g.inv_i0b;
}

inline RsGeom rs_geom(uint32_t src, uint32_t dst) {
    RsGeom g;
    const uint64_t c = std::gcd((uint64_t)src, (uint64_t)dst);
    g.p = dst / c;
    g.q = src / c;
    const double s = std::min(1.0, (double)dst / (double)src);
    g.W = RS_Z / s;
    g.Wi = (int)std::ceil(g.W);
    g.L = 2 * g.Wi;
    g.a = RS_RHO * s;
    g.gain = (double)src / (double)dst;
    g.inv_i0b = 1.0 / rs_i0(RS_BETA);
    return g;
}

// frames of a converted IR of `frames` input frames: ceil(frames p / q)
inline uint64_t rs_out_frames(const RsGeom& g, uint64_t frames) { return (frames * g.p + g.q - 1) / g.q; }

// tab[j][ph] = coefficient of tap j at phase ph (frac = ph / p)
__global__ __launch_bounds__(RS_THREADS) void k_rs_table(RsGeom g, float* __restrict__ tab) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= g.p * (uint64_t)g.L) return;
    const int j = (int)(i / g.p);
    const uint64_t ph = i % g.p;
    tab[i] = (float)rs_coef(g, (double)(g.Wi - 1 - j) + (double)ph / (double)g.p);
}

// part[blockIdx][0..3] = the workgroup's share of sum h_L, sum h_R, sum h_L (-1)^m, sum h_R (-1)^m
template <bool TABLE>
__global__ __launch_bounds__(RS_THREADS) void k_resample(const float2* __restrict__ x, uint64_t frames, float2* __restrict__ y, uint64_t nout,
                                                         RsGeom g, const float* __restrict__ tab, double* __restrict__ part) {
    __shared__ float2 win[RS_STAGE];
    __shared__ double red[4][RS_THREADS];
    const uint64_t m0 = (uint64_t)blockIdx.x * RS_THREADS;
    const uint64_t m = m0 + threadIdx.x;
    const uint64_t mlast = m0 + RS_THREADS - 1 < nout ? m0 + RS_THREADS - 1 : nout - 1;
    const int64_t base = (int64_t)(m0 * g.q / g.p) - g.Wi + 1;          // first input frame of the workgroup's window
    const int64_t span = (int64_t)(mlast * g.q / g.p) + g.Wi + 1 - base;  // its length: through n0(mlast) + Wi
    const bool staged = span <= RS_STAGE;                                 // (uniform over the workgroup)
    if (staged) {
        for (int64_t i = threadIdx.x; i < span; i += RS_THREADS) {
            const int64_t n = base + i;
            win[i] = n >= 0 && n < (int64_t)frames ? x[n] : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    float2 out = make_float2(0.f, 0.f);
    if (m < nout) {
        const uint64_t mq = m * g.q;
        const uint64_t ph = mq % g.p;
        const int64_t first = (int64_t)(mq / g.p) - g.Wi + 1;
        const double frac = (double)ph / (double)g.p;
        const float* c = TABLE ? tab + ph : nullptr;
        double accL = 0.0, accR = 0.0;
        for (int j = 0; j < g.L; j++) {
            float2 v;
            if (staged) {
                v = win[first - base + j];
            } else {
                const int64_t n = first + j;
                v = n >= 0 && n < (int64_t)frames ? x[n] : make_float2(0.f, 0.f);
            }
            const double k = TABLE ? (double)c[(uint64_t)j * g.p] : rs_coef(g, (double)(g.Wi - 1 - j) + frac);
            accL = fma(k, (double)v.x, accL);
            accR = fma(k, (double)v.y, accR);
        }
        out = make_float2((float)accL, (float)accR);
        y[m] = out;
    }
    // (m0 is a multiple of 256: the parity of m is the lane's)
    const double sg = (threadIdx.x & 1) ? -1.0 : 1.0;
    red[0][threadIdx.x] = out.x;
    red[1][threadIdx.x] = out.y;
    red[2][threadIdx.x] = sg * out.x;
    red[3][threadIdx.x] = sg * out.y;
    __syncthreads();
    for (int w = RS_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 4; k++) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4) part[4 * (uint64_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// Converts `frames` interleaved host frames at src Hz into the first n frames of the device buffer d_out at dst Hz (n <= the
// converted length) on `stream`, and returns the four sums of those taps.  Synchronises the stream; temporaries are freed.
inline hipError_t rs_convert(hipStream_t stream, uint32_t src, uint32_t dst, const float* lr, uint64_t frames, float2* d_out, uint64_t n,
                             double sums[4]) {
    const RsGeom g = rs_geom(src, dst);
    // input frames any of the n outputs reads: through n0(n - 1) + Wi
    const uint64_t need = std::min<uint64_t>(frames, (n - 1) * g.q / g.p + (uint64_t)g.Wi + 1);
    const bool table = g.p <= n && g.p * (uint64_t)g.L <= RS_TABLE_MAX;
    DevArray<float2> d_in;
    const unsigned grid = (unsigned)((n + RS_THREADS - 1) / RS_THREADS);
    DevArray<float> d_tab;
    DevArray<double> d_part;
    std::vector<double> part(4 * (size_t)grid);
    hipError_t er = d_in.alloc(need);
    if (er == hipSuccess) er = d_part.alloc(part.size());
    if (er == hipSuccess && table) er = d_tab.alloc(g.p * (uint64_t)g.L);
    if (er == hipSuccess) er = hipMemcpy(d_in, lr, sizeof(float2) * need, hipMemcpyHostToDevice);
    if (er == hipSuccess) {
        if (table) {
            hipLaunchKernelGGL(k_rs_table, dim3((unsigned)((g.p * (uint64_t)g.L + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, stream, g, d_tab);
            hipLaunchKernelGGL(k_resample<true>, dim3(grid), dim3(RS_THREADS), 0, stream, (const float2*)d_in, need, d_out, n, g, (const float*)d_tab, d_part);
        } else {
            hipLaunchKernelGGL(k_resample<false>, dim3(grid), dim3(RS_THREADS), 0, stream, (const float2*)d_in, need, d_out, n, g, (const float*)nullptr, d_part);
        }
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    for (int k = 0; k < 4; k++) sums[k] = 0.0;
    for (unsigned b = 0; b < grid; b++)
        for (int k = 0; k < 4; k++) sums[k] += part[4 * (size_t)b + k];
    return er;
}
