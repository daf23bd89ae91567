// irshape.hip.h — shaping of an impulse response on load (mc_load_ir_shaped): trim, reverse, decay, fade, normalise.  No
// reference equivalent: the reference convolves with the WAV's frames as they are.
//
// The frames are at the session's rate already (converted by resample.hip.h when the rates differ) and lie on the device;
// they stay there.  With F frames, s0 = min(start, F) and cap = n_ref - nframes:
//   1. trim_db < 0: a[m] = max(|L|, |R|) of frame s0 + m (float), peak = max a (k_shape_peak), t = peak * (float)10^(trim_db / 20),
//      onset = the first m with a[m] >= t (k_shape_onset).  first = s0 + max(0, onset - pre_roll).
//   2. n = min(F - first, length or unlimited, cap) frames are stored; everything below acts on those n.
//   3. tap m = frame first + m, or first + n - 1 - m when reversed, carried in double and multiplied by
//      exp2(-m 3 log2(10) / decay_t60) and, over the last f = min(fade_out, n) taps, by (1 + cos(pi (k + 1) / (f + 1))) / 2
//      for k = m - (n - f).
//   4. k_shape_apply<false> reduces max |tap| and sum (L^2 + R^2) of that; gain = target / peak or target / sqrt(sum / 2);
//      k_shape_apply<true> stores (float)(tap * gain) and reduces the four sums mc_ir_info reports.
// tests/ir_shape_np.py states the same in float64.
//
// Every reduction ends in one partial per workgroup, combined on the host in index order (as rs_convert does): the same
// frames and shape give the same bits.  Within a workgroup a wave reduces by cross-lane shuffles and the four waves meet in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mcconv.h"
#include "owned.h"

constexpr int ISH_THREADS = 256;
constexpr int ISH_WAVES = ISH_THREADS / 64;
constexpr unsigned ISH_SCAN_GRID = 512;            // workgroups of the peak and onset walks, at most
constexpr double ISH_DECAY_K = 9.965784284662087;  // 3 log2(10): 60 dB in octaves
constexpr uint64_t ISH_NONE = ~0ull;

// the load as ish_shape resolved it
struct IshPlan {
    uint64_t F, s0, onset, first, n;
    bool reverse;
    uint64_t t60, fade;
};

template <typename T, typename Op>
__device__ inline T ish_wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

// the workgroup's result in thread 0 (red: ISH_WAVES elements of LDS; reusable after the call)
template <typename T, typename Op>
__device__ inline T ish_block_reduce(T v, T* red, Op op) {
    v = ish_wave_reduce(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < ISH_WAVES; w++) v = op(v, red[w]);
    return v;
}

__device__ inline float ish_amp(float2 v) { return fmaxf(fabsf(v.x), fabsf(v.y)); }

// The walk the peak and the onset kernels share: frames [0, n) of x, two per lane as one 16-byte load.  x is 8-byte
// aligned; when it is not 16-byte aligned frame 0 is taken alone (`head`), and so is a last odd frame.
struct IshWalk {
    uint64_t head, pairs;
    const float4* x2;
};
__device__ inline IshWalk ish_walk(const float2* x, uint64_t n) {
    IshWalk w;
    w.head = ((uintptr_t)x & 8) && n ? 1 : 0;
    w.pairs = (n - w.head) / 2;
    w.x2 = reinterpret_cast<const float4*>(x + w.head);
    return w;
}

// part[blockIdx] = max over the workgroup's frames of max(|L|, |R|)
__global__ __launch_bounds__(ISH_THREADS) void k_shape_peak(const float2* __restrict__ x, uint64_t n, float* __restrict__ part) {
    __shared__ float red[ISH_WAVES];
    const IshWalk w = ish_walk(x, n);
    const uint64_t gid = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * ISH_THREADS;
    float a = 0.f;
    for (uint64_t i = gid; i < w.pairs; i += stride) {
        const float4 v = w.x2[i];
        a = fmaxf(a, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    if (gid == 0) {
        if (w.head) a = fmaxf(a, ish_amp(x[0]));
        if (w.head + 2 * w.pairs < n) a = fmaxf(a, ish_amp(x[n - 1]));
    }
    a = ish_block_reduce(a, red, [](float p, float q) { return fmaxf(p, q); });
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// part[blockIdx] = the smallest m among the workgroup's frames with max(|L|, |R|) >= t, ISH_NONE when there is none
__global__ __launch_bounds__(ISH_THREADS) void k_shape_onset(const float2* __restrict__ x, uint64_t n, float t,
                                                             unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[ISH_WAVES];
    const IshWalk w = ish_walk(x, n);
    const uint64_t gid = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * ISH_THREADS;
    unsigned long long at = ISH_NONE;
    for (uint64_t i = gid; i < w.pairs && at == ISH_NONE; i += stride) {
        const float4 v = w.x2[i];
        if (fmaxf(fabsf(v.x), fabsf(v.y)) >= t)
            at = w.head + 2 * i;
        else if (fmaxf(fabsf(v.z), fabsf(v.w)) >= t)
            at = w.head + 2 * i + 1;
    }
    if (gid == 0) {
        if (w.head && ish_amp(x[0]) >= t) at = 0;
        if (w.head + 2 * w.pairs < n && at == ISH_NONE && ish_amp(x[n - 1]) >= t) at = n - 1;
    }
    at = ish_block_reduce(at, red, [](unsigned long long p, unsigned long long q) { return p < q ? p : q; });
    if (threadIdx.x == 0) part[blockIdx.x] = at;
}

// Tap m < n of the shaped IR before the gain (steps 3 to 6 of the header's order), in double: the one expression every kernel
// that shapes goes through (k_shape_apply here, k_eq_fill in ireq.hip.h)
__device__ inline void ish_tap(const float2* __restrict__ x, const IshPlan& pl, uint64_t m, double& L, double& R) {
    const float2 v = x[pl.first + (pl.reverse ? pl.n - 1 - m : m)];
    L = (double)v.x;
    R = (double)v.y;
    if (pl.t60) {
        const double d = exp2(-((double)m * ISH_DECAY_K) / (double)pl.t60);
        L *= d;
        R *= d;
    }
    if (m >= pl.n - pl.fade) {
        const double k = (double)(m - (pl.n - pl.fade));
        const double f = 0.5 * (1.0 + cos(M_PI * (k + 1.0) / ((double)pl.fade + 1.0)));
        L *= f;
        R *= f;
    }
}

// Tap m of the shaped IR, one per thread.  WRITE = false: part[2 b] = max |tap|, part[2 b + 1] = sum (L^2 + R^2) of workgroup
// b, before the gain.  WRITE = true: y[m] = (float)(tap * gain), part[4 b ..] = the workgroup's share of sum h_L, sum h_R,
// sum h_L (-1)^m, sum h_R (-1)^m of what it stored.
template <bool WRITE>
__global__ __launch_bounds__(ISH_THREADS) void k_shape_apply(const float2* __restrict__ x, IshPlan pl, double gain, float2* __restrict__ y,
                                                             double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t m = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x;
    double L = 0.0, R = 0.0;
    if (m < pl.n) ish_tap(x, pl, m, L, R);
    const auto add = [](double p, double q) { return p + q; };
    if (WRITE) {
        float2 out = make_float2(0.f, 0.f);
        if (m < pl.n) {
            out = make_float2((float)(L * gain), (float)(R * gain));
            y[m] = out;
        }
        // (the workgroup's first m is a multiple of 256: the parity of m is the lane's)
        const double sg = (threadIdx.x & 1) ? -1.0 : 1.0;
        const double s[4] = {(double)out.x, (double)out.y, sg * (double)out.x, sg * (double)out.y};
        for (int k = 0; k < 4; k++) {
            const double r = ish_block_reduce(s[k], red, add);
            if (threadIdx.x == 0) part[4 * (uint64_t)blockIdx.x + k] = r;
        }
    } else {
        const double pk = ish_block_reduce(fmax(fabs(L), fabs(R)), red, [](double p, double q) { return fmax(p, q); });
        const double sq = ish_block_reduce(L * L + R * R, red, add);
        if (threadIdx.x == 0) {
            part[2 * (uint64_t)blockIdx.x] = pk;
            part[2 * (uint64_t)blockIdx.x + 1] = sq;
        }
    }
}

// Every field of a shape, checked without touching an engine or HIP; the message names the field.  Null when it is good.
inline const char* ish_check(const mc_ir_shape* s) {
    if (!s) return "null shape";
    if (s->struct_size != sizeof(mc_ir_shape)) return "mc_ir_shape struct_size mismatch";
    if (s->flags & ~MC_SHAPE_REVERSE) return "unknown bit in mc_ir_shape flags";
    if (!(s->trim_db >= -120.f && s->trim_db <= 0.f)) return "trim_db outside [-120, 0]";
    if (s->normalize > MC_NORM_ENERGY) return "normalize is not an MC_NORM_* value";
    if (s->normalize != MC_NORM_NONE && !(std::isfinite(s->target) && s->target > 0.f)) return "target must be finite and > 0";
    return nullptr;
}

// a shape that changes nothing: the load is mc_load_ir(_resampled) itself
inline bool ish_is_off(const mc_ir_shape& s) {
    return !s.flags && !s.start && s.trim_db == 0.f && !s.length && !s.decay_t60 && !s.fade_out && s.normalize == MC_NORM_NONE;
}

// ireq.hip.h: the bands of a load with EQ and what finishes such a load once the plan stands (steps 3 to 8 with 6b)
// (damp: irdamp.hip.h, step 6a of a damped load; null = none)
struct IeqCascade;
struct DampPlan;
inline hipError_t ieq_finish(hipStream_t stream, const float2* d_x, const IshPlan& pl, const mc_ir_shape& sh, const IeqCascade& eq,
                             float2** d_out, uint64_t* n_out, double sums[4], double info[8], const DampPlan* damp = nullptr);

// Shapes the F device frames d_x (at the session's rate) into a new device buffer of n <= cap taps, *d_out, which the caller
// owns.  sums = the four mc_ir_info sums of the stored taps, info = what mc_ir_shape_info reports.  Synchronises the stream.
// *n_out == 0 (and no buffer) when the shape leaves no frame.  eq = the bands of mc_load_ir_eq (null: none): the selection is
// this function's, everything after it ieq_finish's.  damp = the damping of mc_load_ir_damped (null: none; needs eq, which may
// hold no band).
inline hipError_t ish_shape(hipStream_t stream, const float2* d_x, uint64_t F, uint64_t cap, const mc_ir_shape& sh, float2** d_out,
                            uint64_t* n_out, double sums[4], double info[8], const IeqCascade* eq = nullptr, const DampPlan* damp = nullptr) {
    *d_out = nullptr;
    *n_out = 0;
    IshPlan pl;
    pl.F = F;
    pl.s0 = std::min<uint64_t>(sh.start, F);
    pl.onset = 0;
    const uint64_t rest = F - pl.s0;
    hipError_t er = hipSuccess;
    if (sh.trim_db < 0.f && rest) {
        const unsigned grid = (unsigned)std::min<uint64_t>(ISH_SCAN_GRID, (rest / 2 + ISH_THREADS) / ISH_THREADS);
        DevArray<unsigned long long> d_part;  // (the peaks as floats first, then the positions)
        er = d_part.alloc(grid);
        std::vector<float> pk(grid);
        std::vector<unsigned long long> at(grid);
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_shape_peak, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x + pl.s0, rest, reinterpret_cast<float*>(d_part.get()));
            er = hipGetLastError();
        }
        if (er == hipSuccess) er = hipMemcpyAsync(pk.data(), d_part, sizeof(float) * grid, hipMemcpyDeviceToHost, stream);
        if (er == hipSuccess) er = hipStreamSynchronize(stream);
        if (er == hipSuccess) {
            float peak = 0.f;
            for (float v : pk) peak = std::max(peak, v);
            const float t = peak * (float)std::pow(10.0, (double)sh.trim_db / 20.0);
            hipLaunchKernelGGL(k_shape_onset, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x + pl.s0, rest, t, (unsigned long long*)d_part);
            er = hipGetLastError();
        }
        if (er == hipSuccess) er = hipMemcpyAsync(at.data(), d_part, sizeof(unsigned long long) * grid, hipMemcpyDeviceToHost, stream);
        if (er == hipSuccess) er = hipStreamSynchronize(stream);
        if (er != hipSuccess) return er;
        uint64_t onset = ISH_NONE;
        for (unsigned long long v : at) onset = std::min<uint64_t>(onset, v);
        pl.onset = onset == ISH_NONE ? 0 : onset;  // (frames that compare false with everything: nothing is trimmed)
    }
    pl.first = pl.s0 + (pl.onset > sh.pre_roll ? pl.onset - sh.pre_roll : 0);
    pl.n = std::min<uint64_t>(F - pl.first, cap);
    if (sh.length) pl.n = std::min<uint64_t>(pl.n, sh.length);
    if (!pl.n) return hipSuccess;
    pl.reverse = (sh.flags & MC_SHAPE_REVERSE) != 0;
    pl.t60 = sh.decay_t60;
    pl.fade = std::min<uint64_t>(sh.fade_out, pl.n);
    if (eq) return ieq_finish(stream, d_x, pl, sh, *eq, d_out, n_out, sums, info, damp);

    const unsigned grid = (unsigned)((pl.n + ISH_THREADS - 1) / ISH_THREADS);
    DevArray<float2> d_y;
    DevArray<double> d_part;
    std::vector<double> part(4 * (size_t)grid);
    er = d_y.alloc(pl.n);
    if (er == hipSuccess) er = d_part.alloc(part.size());
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_shape_apply<false>, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x, pl, 1.0, (float2*)nullptr, d_part);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * 2 * grid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    double peak = 0.0, sq = 0.0, gain = 1.0;
    if (er == hipSuccess) {
        for (unsigned b = 0; b < grid; b++) {
            peak = std::max(peak, part[2 * (size_t)b]);
            sq += part[2 * (size_t)b + 1];
        }
        const double energy = std::sqrt(sq / 2.0);
        const double measure = sh.normalize == MC_NORM_PEAK ? peak : (sh.normalize == MC_NORM_ENERGY ? energy : 0.0);
        if (measure > 0.0) gain = (double)sh.target / measure;
        hipLaunchKernelGGL(k_shape_apply<true>, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x, pl, gain, d_y, d_part);
        er = hipGetLastError();
        const double inf[8] = {(double)F, (double)pl.onset, (double)pl.first, (double)pl.n, gain, peak, energy, 0.0};
        std::copy(inf, inf + 8, info);
    }
    if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * 4 * grid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    if (er != hipSuccess) return er;
    for (int k = 0; k < 4; k++) sums[k] = 0.0;
    for (unsigned b = 0; b < grid; b++)
        for (int k = 0; k < 4; k++) sums[k] += part[4 * (size_t)b + k];
    *d_out = d_y.release();  // the caller owns the taps from here (load_ir adopts them)
    *n_out = pl.n;
    return hipSuccess;
}
