// irphase.hip.h — the phase step of an impulse-response load (mc_load_ir_phase, mc_load_ir_sweep_phase): the F frames are
// replaced by the minimum-phase IR of the same magnitude response, found by the homomorphic (cepstral) method.  No reference
// equivalent.  Step 1b of the shaped load (include/mcconv.h has the definition, DESIGN.md 2.19 the reasons): shape_stage runs
// phase_run on the F frames that the source and the tail step left and hands irshape.hip.h the F frames it makes.
// tests/ir_phase_np.py states the same with numpy's FFT, one channel at a time.
//
// Per channel, in double, Nfft = max(16, (smallest power of two >= F) << over_log2):
//   X = FFT(x padded to Nfft), p = |X|^2, pm = max p; p = max(p, pm 10^(-floor_db / 10)); L = ln(p) / 2;
//   c = Re IFFT(L), folded: c[0] and c[Nfft / 2] kept, c[1 .. Nfft / 2) doubled, the rest zero;
//   C = FFT(c); Y = exp(Re C) (cos Im C + i sin Im C); y = Re IFFT(Y); the first F of y, rounded to float once.
//
// Both channels ride one complex transform (fft64.hip.h), four transforms in all:
//   z = x_L + i x_R -> Z; X_L[k] = (Z[k] + conj Z[N - k]) / 2, X_R[k] = (Z[k] - conj Z[N - k]) / (2 i)      (k_ph_power)
//   L_L + i L_R -> IFFT: both log spectra are real and even, so Re is c_L and Im is c_R                      (k_ph_log, k_ph_fold)
//   c_L + i c_R (folded) -> FFT, separated as Z was; Y_L + i Y_R -> IFFT: Re is y_L, Im is y_R                (k_ph_exp)
// A channel's bits therefore depend on the other channel below the last place of a double: each transform's rounding error
// is relative to the larger channel.  A channel whose frames are all zero (pm = 0) is stored as zeros and takes no part: its
// log spectrum rides as zeros.
//
// Kernels apart from the transform's passes, each one element per lane, 256 lanes per workgroup, grids that depend on F and
// Nfft alone: k_ph_pack (pad and pack, the sums of the input), k_ph_power (|X|^2 of both channels and its maximum),
// k_ph_log (floor, log and the count of clamped bins; the count needs the maximum, so it lives here), k_ph_fold, k_ph_exp,
// k_ph_unpack (round, store, the sums of the output).  Every reduction ends in one partial per workgroup, which always covers
// the same 256 elements, added on the host in index order (as irshape.hip.h does): the same frames give the same bits.
#pragma once
#include <cstdio>
#include <cstring>

#include "irspectral.hip.h"

constexpr uint64_t PH_MAX_FRAMES = 1ull << 21;
constexpr int PH_MAX_LOG2 = F64_MAX_LOG2;  // Nfft <= 2^22
constexpr int PH_THREADS = ISH_THREADS;

// a checked mc_ir_phase that is on, over F frames
struct PhaseStep {
    uint64_t F, Nfft;
    double floor_db;
    Fft64Plan fft;
};

// z[i] = (x[i].L, x[i].R) as double for i < F, zero up to N.  Workgroups that hold a frame: part[2 b] = sum e, part[2 b + 1] =
// sum i e over their frames, e = L^2 + R^2.
__global__ __launch_bounds__(PH_THREADS) void k_ph_pack(const float2* __restrict__ x, uint64_t F, uint64_t N, double2* __restrict__ z,
                                                        double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    double2 v = make_double2(0.0, 0.0);
    if (i < F) {
        const float2 f = x[i];
        v = make_double2((double)f.x, (double)f.y);
    }
    if (i < N) z[i] = v;
    if ((uint64_t)blockIdx.x * PH_THREADS >= F) return;  // (the whole workgroup)
    const auto add = [](double p, double q) { return p + q; };
    const double e = v.x * v.x + v.y * v.y;
    const double s0 = ish_block_reduce(e, red, add), s1 = ish_block_reduce((double)i * e, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = s0;
        part[2 * (uint64_t)blockIdx.x + 1] = s1;
    }
}

// P[k] = (|X_L[k]|^2, |X_R[k]|^2); part[2 b], part[2 b + 1] = the workgroup's maxima
__global__ __launch_bounds__(PH_THREADS) void k_ph_power(const double2* __restrict__ Z, uint64_t N, double2* __restrict__ P, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t k = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    double2 p = make_double2(0.0, 0.0);
    if (k < N) {
        double2 l, r;
        fl_split(Z[k], Z[(N - k) & (N - 1)], l, r);
        p = make_double2(l.x * l.x + l.y * l.y, r.x * r.x + r.y * r.y);
        P[k] = p;
    }
    const auto mx = [](double a, double b) { return fmax(a, b); };
    const double m0 = ish_block_reduce(p.x, red, mx), m1 = ish_block_reduce(p.y, red, mx);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = m0;
        part[2 * (uint64_t)blockIdx.x + 1] = m1;
    }
}

// P[k] <- (ln max(p_L, thr_L) / 2, ln max(p_R, thr_R) / 2), zero for a channel that is off (pm = 0); part[2 b], part[2 b + 1] =
// the workgroup's bins below the threshold
__global__ __launch_bounds__(PH_THREADS) void k_ph_log(double2* __restrict__ P, uint64_t N, double thr_l, double thr_r, int on_l, int on_r,
                                                      unsigned long long* __restrict__ part) {
    __shared__ unsigned long long red[ISH_WAVES];
    const uint64_t k = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    unsigned long long nl = 0, nr = 0;
    if (k < N) {
        const double2 p = P[k];
        nl = on_l && p.x < thr_l, nr = on_r && p.y < thr_r;
        P[k] = make_double2(on_l ? 0.5 * log(fmax(p.x, thr_l)) : 0.0, on_r ? 0.5 * log(fmax(p.y, thr_r)) : 0.0);
    }
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    const unsigned long long c0 = ish_block_reduce(nl, red, add), c1 = ish_block_reduce(nr, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = c0;
        part[2 * (uint64_t)blockIdx.x + 1] = c1;
    }
}

// the fold of both cepstra: [0] and [N / 2] kept, [1, N / 2) doubled, the rest zero
__global__ __launch_bounds__(PH_THREADS) void k_ph_fold(double2* __restrict__ c, uint64_t N) {
    const uint64_t n = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    if (n >= N || n == 0 || n == N / 2) return;
    const double2 v = c[n];
    c[n] = n < N / 2 ? make_double2(2.0 * v.x, 2.0 * v.y) : make_double2(0.0, 0.0);
}

__device__ inline double2 ph_cexp(double2 c) {
    double sn, cs;
    sincos(c.y, &sn, &cs);
    const double m = exp(c.x);
    return make_double2(m * cs, m * sn);
}

// Y[k] = exp(C_L[k]) + i exp(C_R[k]) from Z = FFT(c_L + i c_R)
__global__ __launch_bounds__(PH_THREADS) void k_ph_exp(const double2* __restrict__ Z, uint64_t N, double2* __restrict__ Y) {
    const uint64_t k = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    if (k >= N) return;
    double2 l, r;
    fl_split(Z[k], Z[(N - k) & (N - 1)], l, r);
    const double2 yl = ph_cexp(l), yr = ph_cexp(r);
    Y[k] = make_double2(yl.x - yr.y, yl.y + yr.x);
}

// y[m] = ((float) Re z[m], (float) Im z[m]) for m < F, zero for a channel that is off; part as k_ph_pack's, of what was stored
__global__ __launch_bounds__(PH_THREADS) void k_ph_unpack(const double2* __restrict__ z, uint64_t F, int on_l, int on_r, float2* __restrict__ y,
                                                          double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t m = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    float2 f = make_float2(0.f, 0.f);
    if (m < F) {
        const double2 v = z[m];
        f = make_float2(on_l ? (float)v.x : 0.f, on_r ? (float)v.y : 0.f);
        y[m] = f;
    }
    const auto add = [](double p, double q) { return p + q; };
    const double e = (double)f.x * (double)f.x + (double)f.y * (double)f.y;
    const double s0 = ish_block_reduce(e, red, add), s1 = ish_block_reduce((double)m * e, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = s0;
        part[2 * (uint64_t)blockIdx.x + 1] = s1;
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a phase step that is on, in the struct's order, checked without touching an engine or HIP; the message
// (thread-local) names the field.  Null when it is good.
inline const char* phase_check(const mc_ir_phase* p) {
    static thread_local char msg[160];
    if (p->struct_size != sizeof(mc_ir_phase)) return "mc_ir_phase struct_size mismatch";
    if (p->mode > MC_PHASE_MINIMUM) {
        std::snprintf(msg, sizeof(msg), "mode %u is not an MC_PHASE_* value", p->mode);
        return msg;
    }
    if (!(p->floor_db >= 40.f && p->floor_db <= 300.f)) {
        std::snprintf(msg, sizeof(msg), "floor_db %g outside [40, 300]", (double)p->floor_db);
        return msg;
    }
    if (p->over_log2 < 1 || p->over_log2 > 6) {
        std::snprintf(msg, sizeof(msg), "over_log2 %u outside [1, 6]", p->over_log2);
        return msg;
    }
    return nullptr;
}

// the limits of a checked phase step over F frames: F <= 2^21 and Nfft <= 2^22 (F = 0 is the load's own "empty IR")
inline const char* phase_check_frames(const mc_ir_phase* p, uint64_t F) {
    static thread_local char msg[200];
    if (F > PH_MAX_FRAMES) {
        std::snprintf(msg, sizeof(msg), "the phase step takes at most %llu frames at the session's rate, not %llu", (unsigned long long)PH_MAX_FRAMES,
                      (unsigned long long)F);
        return msg;
    }
    if (F && spec_ceil_log2(F) + (int)p->over_log2 > PH_MAX_LOG2) {
        std::snprintf(msg, sizeof(msg), "over_log2 %u with %llu frames needs a transform of 2^%d points, above 2^%d", p->over_log2,
                      (unsigned long long)F, spec_ceil_log2(F) + (int)p->over_log2, PH_MAX_LOG2);
        return msg;
    }
    return nullptr;
}

// a checked phase step that is on, over F frames within the limits
inline PhaseStep phase_step(const mc_ir_phase& p, uint64_t F) {
    const int lg = std::max(F64_MIN_LOG2, spec_ceil_log2(std::max<uint64_t>(F, 1)) + (int)p.over_log2);
    return PhaseStep{F, 1ull << lg, (double)p.floor_db, fft64_plan(lg)};
}

// what phase_run allocates on the device: two buffers of Nfft double2, a third when the transform has two passes, and the partials
inline uint64_t phase_device_bytes(const PhaseStep& s) { return spec_work_bytes(s.fft, s.Nfft); }

// Step 1b: the s.F frames d_y from the s.F frames d_x, on the stream, after what the stream already holds.  Allocates the work
// buffers (SpectralWork), waits for the kernels and frees them.  info = mc_ir_phase_info's eight numbers.
inline hipError_t phase_run(hipStream_t stream, const float2* d_x, float2* d_y, const PhaseStep& s, double info[8]) {
    const uint64_t F = s.F, N = s.Nfft, gF = spec_groups(F), gN = spec_groups(N);
    SpectralWork wk;
    hipError_t er = wk.alloc(s.fft, N);
    double2 *const d_a = wk.d_a, *const d_b = wk.d_b, *const d_w = wk.d_w;
    double* const d_part = wk.d_part;
    const std::vector<double>& part = wk.part;
    // sum e and sum m e over `groups` partial pairs, in index order
    const auto sums = [&](uint64_t groups, double& E, double& T) {
        E = T = 0.0;
        for (uint64_t b = 0; b < groups; b++) E += part[2 * b], T += part[2 * b + 1];
    };
    double Ein = 0.0, Tin = 0.0, Eout = 0.0, Tout = 0.0, pm[2] = {0.0, 0.0};
    unsigned long long clamped[2] = {0, 0};
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_ph_pack, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_x, F, N, d_a, d_part);
        er = wk.fetch(stream, 2 * gF);
    }
    if (er == hipSuccess) {
        sums(gF, Ein, Tin);
        er = fft64_run(stream, s.fft, d_a, d_a, d_w, false);
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_ph_power, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_a, N, d_b, d_part);
        er = wk.fetch(stream, 2 * gN);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gN; b++) pm[0] = std::max(pm[0], part[2 * b]), pm[1] = std::max(pm[1], part[2 * b + 1]);
        const double rel = std::pow(10.0, -s.floor_db / 10.0);
        hipLaunchKernelGGL(k_ph_log, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_b, N, pm[0] * rel, pm[1] * rel, (int)(pm[0] > 0.0),
                           (int)(pm[1] > 0.0), reinterpret_cast<unsigned long long*>(d_part));
        er = wk.fetch(stream, 2 * gN);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < 2 * gN; b++) {
            unsigned long long v;
            std::memcpy(&v, &part[b], sizeof(v));
            clamped[b & 1] += v;
        }
        er = fft64_run(stream, s.fft, d_b, d_b, d_w, true);
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_ph_fold, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_b, N);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_b, d_b, d_w, false);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_ph_exp, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_b, N, d_a);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_a, d_a, d_w, true);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_ph_unpack, dim3((unsigned)gF), dim3(PH_THREADS), 0, stream, d_a, F, (int)(pm[0] > 0.0), (int)(pm[1] > 0.0), d_y, d_part);
        er = wk.fetch(stream, 2 * gF);
    }
    if (er == hipSuccess) {
        sums(gF, Eout, Tout);
        const double inf[8] = {(double)F, (double)N, Ein, Eout, Ein > 0.0 ? Tin / Ein : 0.0, Eout > 0.0 ? Tout / Eout : 0.0, (double)clamped[0], (double)clamped[1]};
        std::copy(inf, inf + 8, info);
    } else {
        (void)hipStreamSynchronize(stream);
    }
    return er;
}
