// irspring.hip.h — a spring reverberation tank's IR on the device (mc_synth_ir_spring): the parametric spring model (a cascade
// of stretched all-pass sections in a feedback loop with a delay) evaluated as a transfer function, one lane per frequency
// bin, on a circle of radius rho > 1; one inverse transform in double; the radius undone frame by frame.  No reference
// equivalent: the reference convolves with the frames of a WAV file.
//
// include/mcconv.h has the definition and tests/ir_spring_np.py states it in float64:
//   bins      z_k^-1 = rho^-1 e^(-2 pi i k / N), rho = R^(1/N), R = 1e8; X[k] = H_L(z_k) + i H_R(z_k), k <= N / 2, and the
//             mirrored bin from H(conj z) = conj H(z) (k_spring_bins);
//   frames    x = the inverse transform of X (fft64.hip.h, in place); y[t] = x[t] rho^t = sum_m h[t + m N] R^-m;
//   store     llrint(y 2^40) into acc[t][channel], one lane per frame, plain stores (k_spring_acc);
//   frame     (float)(late + direct + reflections + acc 2^-40): irroom.hip.h's k_synth_room, which reads any such accumulator.
//
// spring_check is the one host function behind the load, the plan and the response: it makes SpringConst, the block of
// constants the kernel takes by value.  spring_eval is the transfer function itself, host and device from one text: what
// differs between the two is only where z^-q comes from (the kernel: an angle reduced in 64-bit integers, one sincospi and one
// exp; mc_ir_spring_response: the unit circle at a frequency in Hz).
//
// Cost.  A bin needs 2 + 2 S (4 S with the high loop) z^-q, each one sincospi and one exp in double, a complex division per
// section kind, biquad and loop, and about 1.5 log2 M complex multiplications per power, N / 2 + 1 lanes.  No LDS, no atomics.
// The bins and the transform take about the same time (profiles/irspring.md: 25 and 32 us at N = 2^19, 125 and 142 us at 2^22).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/mcconv.h"
#include "fft64.hip.h"
#include "irroom.hip.h"

constexpr int SPRING_THREADS = 256;
constexpr int SPRING_MAX_BIQUADS = 6;

// the constants of a checked mc_ir_spring as the kernel and the response take them
struct SpringConst {
    uint32_t S, K, M, Mh, nb, high;          // springs, stretch, sections, high sections, biquads of B, 1 = the high loop is on
    uint32_t L[MC_SPRING_MAX][2], Lh[MC_SPRING_MAX][2];
    double g[MC_SPRING_MAX][2], gh[MC_SPRING_MAX][2];
    double a, c, ah, hg, scale;              // dispersion, damping, high dispersion, high gain, gain / sqrt(S)
    double bq[SPRING_MAX_BIQUADS][3];        // b0, a1, a2 (b1 = 2 b0, b2 = b0)
    double lnrho;                            // ln(R) / N; 0 on the unit circle
};

// a checked mc_ir_spring: the constants, and what the reports need
struct SpringPlan {
    SpringConst k;
    uint64_t N, E, F;
    int lgN;
    double ft, alias_db;
};

__host__ __device__ inline double2 sp_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline double2 sp_div(double2 a, double2 b) {
    const double d = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
// a^m by square-and-multiply from m's highest bit down (m = 0: 1)
__host__ __device__ inline double2 sp_pow(double2 a, uint32_t m) {
    if (!m) return make_double2(1.0, 0.0);
    int top = 31;
    while (!(m >> top)) top--;
    double2 r = a;
    for (int b = top - 1; b >= 0; b--) {
        r = sp_mul(r, r);
        if ((m >> b) & 1u) r = sp_mul(r, a);
    }
    return r;
}
// u / (1 - g u)
__host__ __device__ inline double2 sp_loop(double2 u, double g) { return sp_div(u, make_double2(1.0 - g * u.x, -(g * u.y))); }

// H_L and H_R at the z whose powers zp(q) = z^-q hands out
template <class ZPow>
__host__ __device__ inline void spring_eval(const SpringConst& k, ZPow&& zp, double2& HL, double2& HR) {
    const double2 z1 = zp(1u), zK = k.K == 1 ? z1 : zp(k.K);
    // C P: the cascade and the loop's one-pole, the same for every spring and channel
    const double2 A = sp_div(make_double2(k.a + zK.x, zK.y), make_double2(1.0 + k.a * zK.x, k.a * zK.y));
    const double2 P = sp_div(make_double2(1.0 - k.c, 0.0), make_double2(1.0 - k.c * z1.x, -(k.c * z1.y)));
    const double2 CP = sp_mul(sp_pow(A, k.M), P);
    double2 B = make_double2(1.0, 0.0);
    if (k.nb) {
        const double2 z2 = sp_mul(z1, z1);
        for (uint32_t i = 0; i < k.nb; i++) {
            const double b0 = k.bq[i][0], a1 = k.bq[i][1], a2 = k.bq[i][2];
            const double2 num = make_double2(b0 * ((1.0 + 2.0 * z1.x) + z2.x), b0 * (2.0 * z1.y + z2.y));
            const double2 den = make_double2((1.0 + a1 * z1.x) + a2 * z2.x, a1 * z1.y + a2 * z2.y);
            B = sp_mul(B, sp_div(num, den));
        }
    }
    double2 Ch = make_double2(0.0, 0.0);
    if (k.high) Ch = sp_pow(sp_div(make_double2(k.ah + z1.x, z1.y), make_double2(1.0 + k.ah * z1.x, k.ah * z1.y)), k.Mh);
    double2 sum[2] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
    for (uint32_t s = 0; s < k.S; s++)
        for (int c = 0; c < 2; c++) {
            double2 h = sp_loop(sp_mul(CP, zp(k.L[s][c])), k.g[s][c]);
            if (k.nb) h = sp_mul(B, h);
            if (k.high) {
                const double2 hh = sp_loop(sp_mul(Ch, zp(k.Lh[s][c])), k.gh[s][c]);
                h = make_double2(h.x + k.hg * hh.x, h.y + k.hg * hh.y);
            }
            sum[c] = make_double2(sum[c].x + h.x, sum[c].y + h.y);
        }
    HL = make_double2(k.scale * sum[0].x, k.scale * sum[0].y);
    HR = make_double2(k.scale * sum[1].x, k.scale * sum[1].y);
}

// Bin b <= N / 2 and its mirror.  X: N double2.  grid * SPRING_THREADS >= N / 2 + 1.
__global__ __launch_bounds__(SPRING_THREADS) void k_spring_bins(double2* __restrict__ X, SpringConst k, int lgN) {
    const uint64_t N = 1ull << lgN, b = (uint64_t)blockIdx.x * SPRING_THREADS + threadIdx.x;
    if (b > N / 2) return;
    const double inv_half_N = 2.0 / (double)N;
    const auto zp = [&](uint32_t q) {
        double sn, cs;
        sincospi((double)((b * (uint64_t)q) & (N - 1)) * inv_half_N, &sn, &cs);  // (the argument is exact in double)
        const double mag = exp(-((double)q * k.lnrho));
        return make_double2(mag * cs, -(mag * sn));
    };
    double2 HL, HR;
    spring_eval(k, zp, HL, HR);
    X[b] = make_double2(HL.x - HR.y, HL.y + HR.x);
    if (b && b < N / 2) X[N - b] = make_double2(HL.x + HR.y, HR.x - HL.y);
}

// Frame t < E: x[t] rho^t 2^40, rounded to nearest even, into acc[t] = (L, R).  grid * SPRING_THREADS >= E.
__global__ __launch_bounds__(SPRING_THREADS) void k_spring_acc(long long* __restrict__ acc, const double2* __restrict__ x, uint64_t E, double lnrho) {
    const uint64_t t = (uint64_t)blockIdx.x * SPRING_THREADS + threadIdx.x;
    if (t >= E) return;
    const double up = exp((double)t * lnrho);
    const double2 v = x[t];
    acc[2 * t] = llrint((v.x * up) * ROOM_Q);
    acc[2 * t + 1] = llrint((v.y * up) * ROOM_Q);
}

// -- host ------------------------------------------------------------------------------------------------------------
// E of the definition
inline uint64_t spring_last(const mc_ir_spring& s, uint64_t F) { return s.last ? std::min<uint64_t>(s.last, F) : F; }

// g of the definition for the period T
inline double spring_gain(float t60, double T) { return t60 != 0.f ? -std::pow(10.0, (-3.0 * T) / (double)t60) : 0.0; }

// Every field of a spring, in the struct's order, then what follows from them and from the session's rate and F (a checked
// synthesis's; F = 0: no frames are involved, N and E are not looked at and lnrho stays 0: the unit circle), without touching an
// engine or HIP; the message names the field.  Null when it is good, and then *plan (when given) is the plan.
inline const char* spring_check(const mc_ir_spring* sp, uint32_t rate, uint64_t F, SpringPlan* plan = nullptr) {
#pragma clang fp contract(off)
    static thread_local char msg[240];
    if (!sp) return "null spring";
    if (sp->struct_size != sizeof(mc_ir_spring)) return "mc_ir_spring struct_size mismatch";
    msg[0] = 0;
    const auto outside = [](const char* name, int j, float v, double lo, double hi) {
        if (std::isfinite(v) && (double)v >= lo && (double)v <= hi) return false;
        if (j < 0)
            std::snprintf(msg, sizeof(msg), "%s %g outside [%g, %g]", name, (double)v, lo, hi);
        else
            std::snprintf(msg, sizeof(msg), "%s[%d] %g outside [%g, %g]", name, j, (double)v, lo, hi);
        return true;
    };
    const auto decay = [&](const char* name, float v) {
        if (v == 0.f || !outside(name, -1, v, 0.001, 1000.0)) return false;
        std::snprintf(msg, sizeof(msg), "%s %g must be 0 or in [0.001, 1000]", name, (double)v);
        return true;
    };
    if (sp->sections > 512) {
        std::snprintf(msg, sizeof(msg), "sections %u outside [0, 512]", sp->sections);
        return msg;
    }
    if (!(std::isfinite(sp->transition_hz) && sp->transition_hz > 0.f)) {
        std::snprintf(msg, sizeof(msg), "transition_hz %g must be finite and above 0", (double)sp->transition_hz);
        return msg;
    }
    if (outside("dispersion", -1, sp->dispersion, 0.0, 0.95)) return msg;
    uint32_t S = 0;
    for (int s = 0; s < MC_SPRING_MAX; s++) {
        if (sp->delay_ms[s] != 0.f && outside("delay_ms", s, sp->delay_ms[s], 0.0, 10000.0)) {
            std::snprintf(msg, sizeof(msg), "delay_ms[%d] %g must be 0 (no spring) or in (0, 10000]", s, (double)sp->delay_ms[s]);
            return msg;
        }
        if (sp->delay_ms[s] != 0.f) {
            if ((int)S != s) {
                std::snprintf(msg, sizeof(msg), "delay_ms[%d] %g follows an absent spring: the present springs come first", s, (double)sp->delay_ms[s]);
                return msg;
            }
            S++;
        }
    }
    if (!S) {
        std::snprintf(msg, sizeof(msg), "delay_ms[0] 0: at least one spring must be present");
        return msg;
    }
    if (decay("t60_s", sp->t60_s)) return msg;
    if (outside("damping", -1, sp->damping, 0.0, 0.95)) return msg;
    if (sp->lowpass_order > 12 || (sp->lowpass_order & 1u)) {
        std::snprintf(msg, sizeof(msg), "lowpass_order %u must be 0 or even in [2, 12]", sp->lowpass_order);
        return msg;
    }
    if (outside("high_gain", -1, sp->high_gain, 0.0, 16.0)) return msg;
    if (sp->high_sections > 1024) {
        std::snprintf(msg, sizeof(msg), "high_sections %u outside [0, 1024]", sp->high_sections);
        return msg;
    }
    if (outside("high_dispersion", -1, sp->high_dispersion, -0.95, 0.0)) return msg;
    if (!(std::isfinite(sp->high_delay) && sp->high_delay > 0.f && sp->high_delay <= 1.f)) {
        std::snprintf(msg, sizeof(msg), "high_delay %g outside (0, 1]", (double)sp->high_delay);
        return msg;
    }
    if (decay("high_t60_s", sp->high_t60_s)) return msg;
    if (outside("stereo", -1, sp->stereo, 0.0, 0.25)) return msg;
    if (!(std::isfinite(sp->gain) && sp->gain > 0.f && sp->gain <= 16.f)) {
        std::snprintf(msg, sizeof(msg), "gain %g outside (0, 16]", (double)sp->gain);
        return msg;
    }
    if (sp->log2_points && (sp->log2_points < 10 || sp->log2_points > MC_SPRING_MAX_LOG2)) {
        std::snprintf(msg, sizeof(msg), "log2_points %u must be 0 or in [10, %d]", sp->log2_points, MC_SPRING_MAX_LOG2);
        return msg;
    }
    if (rate < 8000 || rate > 384000) {
        std::snprintf(msg, sizeof(msg), "rate %u outside [8000, 384000]: the spring needs the session's rate", rate);
        return msg;
    }
    // what follows from the fields and the rate
    if (!((double)sp->transition_hz <= (double)rate / 2.0)) {
        std::snprintf(msg, sizeof(msg), "transition_hz %g above half the rate %u", (double)sp->transition_hz, rate);
        return msg;
    }
    const double Kd = std::max(1.0, std::nearbyint((double)rate / (2.0 * (double)sp->transition_hz)));
    if (Kd > (double)MC_SPRING_MAX_STRETCH) {
        std::snprintf(msg, sizeof(msg), "transition_hz %g at rate %u stretches the sections by K = %.0f, more than %d", (double)sp->transition_hz, rate, Kd,
                      MC_SPRING_MAX_STRETCH);
        return msg;
    }
    SpringPlan local;
    SpringPlan& pl = plan ? *plan : local;
    pl = SpringPlan{};
    SpringConst& k = pl.k;
    k.S = S, k.K = (uint32_t)Kd, k.M = sp->sections, k.Mh = sp->high_sections, k.high = sp->high_gain != 0.f;
    k.a = (double)sp->dispersion, k.c = (double)sp->damping, k.ah = (double)sp->high_dispersion, k.hg = (double)sp->high_gain;
    k.scale = (double)sp->gain / std::sqrt((double)S);
    const double MK = (double)k.M * Kd;
    const double own = std::nearbyint((MK * (1.0 - k.a)) / (1.0 + k.a));  // the cascade's delay at 0 Hz
    double gmax = 0.0, trip = 0.0, ghmax = 0.0, htrip = 0.0;
    for (uint32_t s = 0; s < S; s++)
        for (int c = 0; c < 2; c++) {
            const double T0 = (double)sp->delay_ms[s] / 1000.0, T = c ? T0 * (1.0 + (double)sp->stereo) : T0;
            const double L = std::nearbyint(T * (double)rate) - own;
            if (L < 1.0) {
                std::snprintf(msg, sizeof(msg), "delay_ms[%u] %g is shorter than the dispersion's own delay (channel %c: %.0f frames less %.0f)", s,
                              (double)sp->delay_ms[s], c ? 'R' : 'L', std::nearbyint(T * (double)rate), own);
                return msg;
            }
            k.L[s][c] = (uint32_t)L;
            k.g[s][c] = spring_gain(sp->t60_s, T);
            if (std::fabs(k.g[s][c]) > 0.9999) {
                std::snprintf(msg, sizeof(msg), "t60_s %g makes the loop gain of delay_ms[%u] %g, beyond 0.9999", (double)sp->t60_s, s, k.g[s][c]);
                return msg;
            }
            k.Lh[s][c] = (uint32_t)std::max(1.0, std::nearbyint(((double)sp->high_delay * T) * (double)rate));
            k.gh[s][c] = spring_gain(sp->high_t60_s, T);
            if (k.high && std::fabs(k.gh[s][c]) > 0.9999) {
                std::snprintf(msg, sizeof(msg), "high_t60_s %g makes the loop gain of delay_ms[%u] %g, beyond 0.9999", (double)sp->high_t60_s, s, k.gh[s][c]);
                return msg;
            }
            // the alias bound takes the largest gain with the longest round trip: an upper estimate
            gmax = std::max(gmax, std::fabs(k.g[s][c])), trip = std::max(trip, L + (MK * (1.0 + k.a)) / (1.0 - k.a));
            ghmax = std::max(ghmax, std::fabs(k.gh[s][c]));
            htrip = std::max(htrip, (double)k.Lh[s][c] + ((double)k.Mh * (1.0 - k.ah)) / (1.0 + k.ah));
        }
    pl.ft = (double)rate / (2.0 * Kd);
    k.nb = k.K > 1 ? sp->lowpass_order / 2 : 0;
    if (k.nb) {
        const double W = std::tan(M_PI / (2.0 * Kd)), n = (double)sp->lowpass_order;
        for (uint32_t i = 0; i < k.nb; i++) {
            const double q = (2.0 * std::sin((M_PI * (2.0 * (double)i + 1.0)) / (2.0 * n))) * W;
            const double a0 = (1.0 + q) + W * W;
            k.bq[i][0] = (W * W) / a0;
            k.bq[i][1] = (2.0 * (W * W - 1.0)) / a0;
            k.bq[i][2] = ((1.0 - q) + W * W) / a0;
        }
    }
    pl.F = F;
    if (!F) return nullptr;
    const uint64_t E = spring_last(*sp, F);
    int lg = (int)sp->log2_points;
    if (!lg) {
        lg = 10;
        while ((1ull << lg) < 2 * E && lg <= MC_SPRING_MAX_LOG2) lg++;
        if (lg > MC_SPRING_MAX_LOG2) {
            std::snprintf(msg, sizeof(msg), "%llu frames need more than 2^%d points: a spring renders at most 2^%d frames, set last",
                          (unsigned long long)E, MC_SPRING_MAX_LOG2, MC_SPRING_MAX_LOG2 - 1);
            return msg;
        }
    } else if (E > (1ull << lg) / 2) {
        std::snprintf(msg, sizeof(msg), "log2_points %d renders at most %llu frames and %llu are asked for: set last", lg,
                      (unsigned long long)((1ull << lg) / 2), (unsigned long long)E);
        return msg;
    }
    pl.lgN = lg, pl.N = 1ull << lg, pl.E = E;
    k.lnrho = std::log(MC_SPRING_RADIUS) / (double)pl.N;
    const double room = (double)(pl.N - E);
    double bound = std::pow(gmax, std::floor(room / trip));
    if (k.high) bound = std::max(bound, std::pow(ghmax, std::floor(room / htrip)));
    bound /= MC_SPRING_RADIUS;
    pl.alias_db = bound > 0.0 ? std::max(-400.0, 20.0 * std::log10(bound)) : -400.0;
    return nullptr;
}

// the plan's twenty-four numbers (mc_ir_spring_plan, mc_ir_spring_info)
inline void spring_numbers(const SpringPlan& p, double out[24]) {
    const SpringConst& k = p.k;
    std::fill(out, out + 24, 0.0);
    out[0] = (double)p.N, out[1] = (double)k.K, out[2] = p.ft, out[3] = (double)k.S, out[4] = (double)k.M, out[5] = k.nb ? 1.0 : 0.0;
    out[6] = (double)p.E, out[7] = p.alias_db;
    for (uint32_t s = 0; s < k.S; s++)
        for (int c = 0; c < 2; c++) out[8 + 2 * s + c] = (double)k.L[s][c], out[14 + 2 * s + c] = k.g[s][c];
}

// H_L and H_R on the unit circle at hz, by spring_eval (mc_ir_spring_response)
inline void spring_response(const SpringConst& k, uint32_t rate, double hz, double out[4]) {
    const double nu = hz / (double)rate;
    const auto zp = [&](uint32_t q) {
        const double turn = nu * (double)q;
        const double frac = turn - std::floor(turn);
        return make_double2(std::cos(2.0 * M_PI * frac), -std::sin(2.0 * M_PI * frac));
    };
    double2 HL, HR;
    spring_eval(k, zp, HL, HR);
    out[0] = HL.x, out[1] = HL.y, out[2] = HR.x, out[3] = HR.y;
}

// The syn.F frames with the spring's term into d_x (8-byte aligned), on `stream`, which is waited for.  The bins, the
// transform's work buffer and the accumulator live only inside this call: 32 N + 16 E bytes.
inline hipError_t spring_generate(hipStream_t stream, const SynPlan& syn, const SpringPlan& plan, float2* d_x) {
    const uint64_t N = plan.N, E = plan.E;
    const size_t pts = sizeof(double2) * N, acc_bytes = sizeof(long long) * 2 * E;
    DevArray<char> d_all;
    hipError_t er = d_all.alloc(2 * pts + acc_bytes);
    if (er != hipSuccess) return er;
    double2* d_X = reinterpret_cast<double2*>(d_all.get());
    double2* d_w = reinterpret_cast<double2*>(d_all + pts);
    long long* d_acc = reinterpret_cast<long long*>(d_all + 2 * pts);
    {
        const unsigned grid = (unsigned)((N / 2 + 1 + SPRING_THREADS - 1) / SPRING_THREADS);
        hipLaunchKernelGGL(k_spring_bins, dim3(grid), dim3(SPRING_THREADS), 0, stream, d_X, plan.k, plan.lgN);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = fft64_run(stream, fft64_plan(plan.lgN), d_X, d_X, d_w, true);
    if (er == hipSuccess) {
        const unsigned grid = (unsigned)((E + SPRING_THREADS - 1) / SPRING_THREADS);
        hipLaunchKernelGGL(k_spring_acc, dim3(grid), dim3(SPRING_THREADS), 0, stream, d_acc, d_X, E, plan.k.lnrho);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        const unsigned grid = (unsigned)((std::max<uint64_t>(syn.F / 2, 1) + SYN_THREADS - 1) / SYN_THREADS);
        hipLaunchKernelGGL(k_synth_room, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, d_acc, E);
        er = hipGetLastError();
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (also after a failed launch: earlier kernels may still be running)
    if (er == hipSuccess) er = waited;
    return er;
}
