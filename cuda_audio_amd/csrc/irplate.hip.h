// irplate.hip.h — a plate reverberator's IR on the device (mc_synth_ir_plate): the modes of a simply supported rectangular
// plate, every one an exponentially damped cosine, summed in 64-bit integers.  No reference equivalent: the reference convolves
// with the frames of a WAV file.
//
// include/mcconv.h has the definition and tests/ir_plate_np.py states it in float64:
//   modes     m, n >= 1: f = (pi kappa / 2) ((m / Lx)^2 + (n / Ly)^2), kept when low <= f <= high, m ascending, n within m;
//             sigma = s0 + (s1 - s0) f / damp_hz; a_c = gain 4 sqrt(2 / M) Phi(driver) Phi(pickup c);
//   term      y_c[t] = sum_j a_jc exp(-sigma_j t / rate) cos(2 pi frac(nu_j t)) for t < E;
//   sum       q = llrint(a exp cos 2^40) added into acc[t][channel], int64: the sum does not depend on the order of arrival;
//   frame     (float)(late + direct + reflections + acc 2^-40): irsynth.hip.h's three terms and this one, rounded once
//             (irroom.hip.h's k_synth_room, which reads any such accumulator).
//
// The evaluation rule (plate_seed, plate_turn) makes exp cos at (row, t) a pure function of the row and t: the first frame
// of every group of MC_PLATE_GROUP frames, aligned in t, is evaluated directly (one exp, one sincospi of a phase reduced in
// turns), the others by complex multiplication with the row's r.  Nothing of it looks at the grid, at F or at M.
//
// k_plate is the work, E x M pairs in double.  A workgroup owns PLATE_THREADS groups of frames and walks `per` slabs of
// MC_PLATE_SLAB rows.  It stages a slab in LDS, from where every lane reads the same row (a broadcast); a lane seeds z at its
// group's first frame and turns it MC_PLATE_GROUP - 1 times, and rounds a_c Re z 2^40 by adding 1.5 2^52 (one fma per
// channel; exact below 2^51, and a 2^40 is below 2^47), whose bit pattern is added as it stands into the lane's integer sums:
// the constant's own bits are taken off once, times the rows, before the sums leave.  They leave by one
// atomicAdd(unsigned long long*) per frame and channel (global_atomic_add_x2, as in k_room).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mcconv.h"
#include "irroom.hip.h"

constexpr int PLATE_THREADS = 256;
constexpr int PLATE_K = MC_PLATE_GROUP;
constexpr int PLATE_SLAB = MC_PLATE_SLAB;
constexpr uint64_t PLATE_TILE = (uint64_t)PLATE_THREADS * PLATE_K;  // frames of a workgroup
constexpr int PLATE_MAX_PER = 8;                                    // slabs a workgroup walks at most
constexpr double PLATE_MAX_SUM = 4194304.0;                         // 2^22, as ROOM_MAX_SUM
constexpr double PLATE_ROUND = 6755399441055744.0;                  // 1.5 2^52
constexpr long long PLATE_ROUND_BITS = 0x4338000000000000ll;        // its bit pattern

// a row of the mode table as mc_ir_plate_modes hands it out
struct PlateMode {
    double m, n, f, sigma, aL, aR;
};

// a row as the kernel takes it: nu = f / rate, dec = sigma / rate, r = exp(-dec) (cos, sin)(2 pi nu), A_c = a_c 2^40
struct PlateRow {
    double nu, dec, rr, ri, AL, AR;
};

// a checked mc_ir_plate: what the reports need, and the table
struct PlatePlan {
    uint64_t M, E, F;
    uint64_t nonzero[2];
    double kappa, density, lo, hi;  // Weyl's modal density; the lowest and the highest kept mode
    double t60_lo, t60_hi;          // 3 ln 10 / sigma at low_hz and at the highest kept mode; 0 = no loss
    std::vector<PlateMode> modes;
    std::vector<PlateRow> rows;
};

// z at frame t0 (a multiple of MC_PLATE_GROUP) of a row: the evaluation rule's direct value
__device__ inline double2 plate_seed(const PlateRow& r, double t0) {
    const double p = r.nu * t0;
    const double turn = fma(r.nu, t0, -rint(p));  // (nu t0 - rint(nu t0) with one rounding: |turn| <= 1/2 and a bit)
    double s, c;
    sincospi(2.0 * turn, &s, &c);
    const double env = exp(-(r.dec * t0));
    return make_double2(env * c, env * s);
}

// z one frame later
__device__ inline double2 plate_turn(const PlateRow& r, double2 z) { return make_double2(z.x * r.rr - z.y * r.ri, z.x * r.ri + z.y * r.rr); }

// grid (tiles of PLATE_TILE frames over E, ceil(slabs / per)).  acc: E frames of two int64, zero.
__global__ __launch_bounds__(PLATE_THREADS) void k_plate(unsigned long long* __restrict__ acc, const PlateRow* __restrict__ rows, uint32_t M, uint64_t E, int per) {
    __shared__ PlateRow slab[PLATE_SLAB];
    const uint64_t t0 = ((uint64_t)blockIdx.x * PLATE_THREADS + threadIdx.x) * PLATE_K;
    const bool live = t0 < E;
    unsigned long long sumL[PLATE_K], sumR[PLATE_K];  // (sums of bit patterns: they wrap, and the bias below brings them back)
#pragma unroll
    for (int k = 0; k < PLATE_K; k++) sumL[k] = sumR[k] = 0;
    uint32_t done = 0;
    for (int s = 0; s < per; s++) {
        const uint32_t first = ((uint32_t)blockIdx.y * (uint32_t)per + (uint32_t)s) * PLATE_SLAB;
        if (first >= M) break;  // (the same in every lane)
        const uint32_t count = min((uint32_t)PLATE_SLAB, M - first);
        __syncthreads();
        if (threadIdx.x < count) slab[threadIdx.x] = rows[first + threadIdx.x];
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < count; j++) {
                const PlateRow r = slab[j];
                double2 z = plate_seed(r, (double)t0);
#pragma unroll
                for (int k = 0; k < PLATE_K; k++) {
                    sumL[k] += (unsigned long long)__double_as_longlong(fma(r.AL, z.x, PLATE_ROUND));
                    sumR[k] += (unsigned long long)__double_as_longlong(fma(r.AR, z.x, PLATE_ROUND));
                    z = plate_turn(r, z);
                }
            }
            done += count;
        }
    }
    if (!live || !done) return;
    const unsigned long long bias = (unsigned long long)done * (unsigned long long)PLATE_ROUND_BITS;
#pragma unroll
    for (int k = 0; k < PLATE_K; k++) {
        const uint64_t t = t0 + (uint64_t)k;
        if (t < E) {
            const unsigned long long vL = sumL[k] - bias, vR = sumR[k] - bias;
            if (vL) atomicAdd(&acc[2 * t], vL);
            if (vR) atomicAdd(&acc[2 * t + 1], vR);
        }
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// E of the definition
inline uint64_t plate_last(const mc_ir_plate& p, uint64_t F) { return p.last ? std::min<uint64_t>(p.last, F) : F; }

inline double plate_kappa(const mc_ir_plate& p) {
#pragma clang fp contract(off)
    const double E = (double)p.young_gpa * 1e9, h = (double)p.thickness_mm * 1e-3, nu = (double)p.poisson;
    return std::sqrt(E * (h * h) / (12.0 * (double)p.density * (1.0 - nu * nu)));
}

// high_hz as used: 0 = min(20000, 0.45 rate)
inline double plate_high(const mc_ir_plate& p, uint32_t rate) { return p.high_hz != 0.f ? (double)p.high_hz : std::min(20000.0, 0.45 * (double)rate); }

// s_i of the definition
inline double plate_loss(float t60) { return t60 != 0.f ? 3.0 * std::log(10.0) / (double)t60 : 0.0; }

// The kept modes (m, n, f) in the table's order; stops one past `cap`.  The frequencies are made of multiplications, divisions
// and one addition in a fixed order with no contraction, so a restatement that keeps the order gets the same doubles and the
// same decisions at low and high.
inline void plate_enumerate(const mc_ir_plate& p, uint32_t rate, uint64_t cap, std::vector<PlateMode>& out) {
#pragma clang fp contract(off)
    const double Lx = (double)p.size_m[0], Ly = (double)p.size_m[1], lo = (double)p.low_hz, hi = plate_high(p, rate);
    const double c = M_PI * plate_kappa(p) / 2.0;
    out.clear();
    for (uint64_t m = 1;; m++) {
        const double qm = ((double)m / Lx) * ((double)m / Lx);
        if (!(c * (qm + (1.0 / Ly) * (1.0 / Ly)) <= hi)) break;
        // the first n that can reach low_hz, from a square root taken with room to spare; the walk below decides
        const double need = lo / c - qm;
        uint64_t n = 1;
        if (need > 0.0) {
            const double guess = std::floor(Ly * std::sqrt(need)) - 2.0;
            if (guess > 1.0) n = (uint64_t)guess;
        }
        for (;; n++) {
            const double qn = ((double)n / Ly) * ((double)n / Ly);
            const double f = c * (qm + qn);
            if (!(f <= hi)) break;
            if (f >= lo) {
                out.push_back(PlateMode{(double)m, (double)n, f, 0.0, 0.0, 0.0});
                if (out.size() > cap) return;
            }
        }
    }
}

// Every field of a plate, in the struct's order, then what follows from them and from the session's rate and F (a checked
// synthesis's; F = 0: no frames are involved and the work cap is not looked at), without touching an engine or HIP; the message
// names the field.  Null when it is good, and then *plan (when given) is the plan.
inline const char* plate_check(const mc_ir_plate* p, uint32_t rate, uint64_t F, PlatePlan* plan = nullptr) {
    static thread_local char msg[240];
    if (!p) return "null plate";
    if (p->struct_size != sizeof(mc_ir_plate)) return "mc_ir_plate struct_size mismatch";
    msg[0] = 0;
    const auto outside = [](const char* name, int j, float v, double lo, double hi) {
        if (std::isfinite(v) && (double)v >= lo && (double)v <= hi) return false;
        if (j < 0)
            std::snprintf(msg, sizeof(msg), "%s %g outside [%g, %g]", name, (double)v, lo, hi);
        else
            std::snprintf(msg, sizeof(msg), "%s[%d] %g outside [%g, %g]", name, j, (double)v, lo, hi);
        return true;
    };
    for (int a = 0; a < 2; a++)
        if (outside("size_m", a, p->size_m[a], 0.05, 10.0)) return msg;
    if (outside("thickness_mm", -1, p->thickness_mm, 0.05, 50.0)) return msg;
    if (outside("young_gpa", -1, p->young_gpa, 0.1, 2000.0)) return msg;
    if (outside("density", -1, p->density, 100.0, 30000.0)) return msg;
    if (outside("poisson", -1, p->poisson, 0.0, 0.499)) return msg;
    for (int a = 0; a < 2; a++)
        if (!(p->driver_m[a] > 0.f && p->driver_m[a] < p->size_m[a])) {
            std::snprintf(msg, sizeof(msg), "driver_m[%d] %g not strictly inside (0, %g)", a, (double)p->driver_m[a], (double)p->size_m[a]);
            return msg;
        }
    for (int c = 0; c < 2; c++)
        for (int a = 0; a < 2; a++)
            if (!(p->pickup_m[c][a] > 0.f && p->pickup_m[c][a] < p->size_m[a])) {
                std::snprintf(msg, sizeof(msg), "pickup_m[%d][%d] %g not strictly inside (0, %g)", c, a, (double)p->pickup_m[c][a], (double)p->size_m[a]);
                return msg;
            }
    if (outside("low_hz", -1, p->low_hz, 1.0, 100000.0)) return msg;
    if (p->high_hz != 0.f && !(std::isfinite(p->high_hz) && p->high_hz > p->low_hz)) {
        std::snprintf(msg, sizeof(msg), "high_hz %g must be 0 or finite and above low_hz %g", (double)p->high_hz, (double)p->low_hz);
        return msg;
    }
    for (int i = 0; i < 2; i++)
        if (p->t60_s[i] != 0.f && outside("t60_s", i, p->t60_s[i], 0.001, 1000.0)) {
            std::snprintf(msg, sizeof(msg), "t60_s[%d] %g must be 0 or in [0.001, 1000]", i, (double)p->t60_s[i]);
            return msg;
        }
    if (!(plate_loss(p->t60_s[1]) >= plate_loss(p->t60_s[0]))) {
        std::snprintf(msg, sizeof(msg), "t60_s[1] %g is longer than t60_s[0] %g: the decay may not grow with frequency (0 = no loss)", (double)p->t60_s[1],
                      (double)p->t60_s[0]);
        return msg;
    }
    if (outside("damp_hz", -1, p->damp_hz, 10.0, 1000000.0)) return msg;
    if (!(std::isfinite(p->gain) && p->gain > 0.f && p->gain <= 16.f)) {
        std::snprintf(msg, sizeof(msg), "gain %g outside (0, 16]", (double)p->gain);
        return msg;
    }
    if (p->reserved) {
        std::snprintf(msg, sizeof(msg), "reserved %u must be 0", p->reserved);
        return msg;
    }
    if (rate < 8000 || rate > 384000) {
        std::snprintf(msg, sizeof(msg), "rate %u outside [8000, 384000]: the plate needs the session's rate", rate);
        return msg;
    }
    const double hi = plate_high(*p, rate);
    if (!(hi < (double)rate / 2.0 && hi > (double)p->low_hz)) {
        std::snprintf(msg, sizeof(msg), "high_hz %g must lie above low_hz %g and below half the rate %u", hi, (double)p->low_hz, rate);
        return msg;
    }
    PlatePlan local;
    PlatePlan& pl = plan ? *plan : local;
    plate_enumerate(*p, rate, MC_PLATE_MAX_MODES, pl.modes);
    const uint64_t M = pl.modes.size();
    if (!M) {
        std::snprintf(msg, sizeof(msg), "low_hz %g to high_hz %g keep no mode (M = 0)", (double)p->low_hz, hi);
        return msg;
    }
    if (M > MC_PLATE_MAX_MODES) {
        std::snprintf(msg, sizeof(msg), "low_hz %g to high_hz %g keep more than %d modes (M): narrow them", (double)p->low_hz, hi, MC_PLATE_MAX_MODES);
        return msg;
    }
    if (!((double)p->gain * 4.0 * std::sqrt(2.0 * (double)M) < PLATE_MAX_SUM)) {
        std::snprintf(msg, sizeof(msg), "gain %g: %llu modes of at most gain 4 sqrt(2 / M) each may sum to 2^22 or more", (double)p->gain, (unsigned long long)M);
        return msg;
    }
    const uint64_t E = F ? plate_last(*p, F) : 0;
    if (E * M > (uint64_t)MC_PLATE_MAX_PAIRS) {
        std::snprintf(msg, sizeof(msg), "%llu frames of %llu modes are %.3g pairs, %.3g times the %.3g allowed: set last, or narrow low_hz to high_hz",
                      (unsigned long long)E, (unsigned long long)M, (double)E * (double)M, (double)E * (double)M / (double)MC_PLATE_MAX_PAIRS,
                      (double)MC_PLATE_MAX_PAIRS);
        return msg;
    }
    // the rest of the table: the loss, the amplitudes, and the rows as the kernel takes them
    {
#pragma clang fp contract(off)
        const double Lx = (double)p->size_m[0], Ly = (double)p->size_m[1];
        const double s0 = plate_loss(p->t60_s[0]), s1 = plate_loss(p->t60_s[1]), damp = (double)p->damp_hz;
        const double scale = (double)p->gain * 4.0 * std::sqrt(2.0 / (double)M);
        const auto phi = [&](double m, double n, const float* at) {
            return std::sin((m * M_PI * (double)at[0]) / Lx) * std::sin((n * M_PI * (double)at[1]) / Ly);
        };
        pl.rows.resize(M);
        pl.nonzero[0] = pl.nonzero[1] = 0;
        for (uint64_t j = 0; j < M; j++) {
            PlateMode& md = pl.modes[j];
            md.sigma = s0 + ((s1 - s0) * md.f) / damp;
            const double d = phi(md.m, md.n, p->driver_m);
            md.aL = (scale * d) * phi(md.m, md.n, p->pickup_m[0]);
            md.aR = (scale * d) * phi(md.m, md.n, p->pickup_m[1]);
            pl.nonzero[0] += md.aL != 0.0;
            pl.nonzero[1] += md.aR != 0.0;
            PlateRow& r = pl.rows[j];
            r.nu = md.f / (double)rate;
            r.dec = md.sigma / (double)rate;
            const double g = std::exp(-r.dec);
            r.rr = g * std::cos(2.0 * M_PI * r.nu);
            r.ri = g * std::sin(2.0 * M_PI * r.nu);
            r.AL = md.aL * ROOM_Q;
            r.AR = md.aR * ROOM_Q;
        }
        pl.M = M, pl.E = E, pl.F = F;
        pl.kappa = plate_kappa(*p);
        pl.density = Lx * Ly / (2.0 * pl.kappa);
        pl.lo = pl.hi = pl.modes[0].f;
        for (const PlateMode& md : pl.modes) pl.lo = std::min(pl.lo, md.f), pl.hi = std::max(pl.hi, md.f);
        const double sig_lo = s0 + ((s1 - s0) * (double)p->low_hz) / damp, sig_hi = s0 + ((s1 - s0) * pl.hi) / damp;
        pl.t60_lo = sig_lo > 0.0 ? 3.0 * std::log(10.0) / sig_lo : 0.0;
        pl.t60_hi = sig_hi > 0.0 ? 3.0 * std::log(10.0) / sig_hi : 0.0;
    }
    return nullptr;
}

// The syn.F frames with the plate's term into d_x (8-byte aligned), on `stream`, which is waited for.  The table and the
// accumulator live only inside this call.
inline hipError_t plate_generate(hipStream_t stream, const SynPlan& syn, const PlatePlan& plan, float2* d_x) {
    const uint64_t E = plan.E, M = plan.M;
    const size_t acc_bytes = sizeof(unsigned long long) * 2 * E, row_bytes = sizeof(PlateRow) * M;
    DevArray<char> d_all;
    hipError_t er = d_all.alloc(acc_bytes + row_bytes);  // (acc_bytes is a multiple of 16: the rows are aligned)
    if (er != hipSuccess) return er;
    unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(d_all.get());
    PlateRow* d_rows = reinterpret_cast<PlateRow*>(d_all + acc_bytes);
    er = hipMemsetAsync(d_acc, 0, acc_bytes, stream);
    if (er == hipSuccess) er = hipMemcpyAsync(d_rows, plan.rows.data(), row_bytes, hipMemcpyHostToDevice, stream);
    if (er == hipSuccess) {
        // enough workgroups to fill the device several times over, and beyond that more slabs per workgroup: fewer atomics
        const uint64_t tiles = (E + PLATE_TILE - 1) / PLATE_TILE, slabs = (M + PLATE_SLAB - 1) / PLATE_SLAB;
        const int per = (int)std::min<uint64_t>(std::max<uint64_t>(tiles * slabs / 2048, 1), PLATE_MAX_PER);
        hipLaunchKernelGGL(k_plate, dim3((unsigned)tiles, (unsigned)((slabs + per - 1) / per)), dim3(PLATE_THREADS), 0, stream, d_acc, d_rows, (uint32_t)M, E, per);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        const unsigned grid = (unsigned)((std::max<uint64_t>(syn.F / 2, 1) + SYN_THREADS - 1) / SYN_THREADS);
        hipLaunchKernelGGL(k_synth_room, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, reinterpret_cast<const long long*>(d_acc), E);
        er = hipGetLastError();
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (also after a failed launch: the copies may still be running)
    if (er == hipSuccess) er = waited;
    return er;
}
