// irdamp.hip.h — damping of an impulse response on load (mc_load_ir_damped): a decay time per frequency band.  No reference
// equivalent.
//
// Step 6a of the shaped load (include/mcconv.h has the definition): x = the n taps after the fade, P_k = x through crossover
// k's two identical low-pass sections from rest at tap 0, g_j[m] = band j's envelope, and
//     y[m] = g_X[m] x[m] + sum over k = 1 .. X of (g_(k-1)[m] - g_k[m]) P_k[m],
// which is sum_j g_j B_j over the bands B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X without a buffer per band.  ieq_finish
// calls damp_run on its double2 [n] buffer between k_eq_fill and the EQ bands.  tests/ir_damp_np.py states the same with
// sequential float64 loops.
//
// EQ's pass filters in place and in cascade; here the X crossovers run in parallel from the same input, so a lane carries all
// of them at once and x is read once, whatever X is.  Chunking, workgroup shape and LDS staging are chunkwalk.hip.h's chunk_walk
// (a lane per (chunk, channel)), as for ireq.hip.h.
// A crossover's state is four doubles, (s1, s2) of the first section and (s3, s4) of the second; over a run of taps it is
// affine in the state before it, s' = A^len s + e, with A the 4 x 4 matrix of the cascade's updates at x = 0.
//   local  k_damp_chunk<false> runs the X crossovers over every chunk from rest and keeps the X end states e_c;
//   carry  k_damp_carry, one workgroup per crossover, is ireq.hip.h's carry_scan over 4-vectors;
//   fix-up k_damp_chunk<true> runs every chunk again from its true states and writes y in place.  The envelopes are evaluated
//          per tap from the tap's own index, not as a running product: a tap's value does not depend on where its chunk starts.
// Two launches of the chunk kernel and one of the carry for any X.  The state scratch is double2 [2 X] per lane, allocated
// here and freed before damp_run returns.
//
// Determinism.  Chunks and runs depend on n alone; no atomics; nothing is combined out of order.
#pragma once
#include "ireq.hip.h"

struct DampMat {
    double m[4][4];
};
// a checked mc_ir_damp as the kernels take it
struct DampPlan {
    int X;
    IeqCoef c[MC_DAMP_MAX_XOVERS];          // one section of crossover k + 1
    uint64_t t60[MC_DAMP_MAX_XOVERS + 1];   // band j, 0 = none
    uint64_t origin;                        // clamped to n by damp_run
};
struct DampCarry {
    DampMat M[MC_DAMP_MAX_XOVERS], MK[MC_DAMP_MAX_XOVERS];
};
// (s1, s2) of the first section, (s3, s4) of the second
struct DampState {
    double s1, s2, s3, s4;
};

// one tap through the two sections; returns the second's output
__host__ __device__ inline double damp_step(const IeqCoef& c, DampState& s, double v) {
    const double y1 = c.b0 * v + s.s1;
    s.s1 = c.b1 * v - c.a1 * y1 + s.s2;
    s.s2 = c.b2 * v - c.a2 * y1;
    const double y2 = c.b0 * y1 + s.s3;
    s.s3 = c.b1 * y1 - c.a1 * y2 + s.s4;
    s.s4 = c.b2 * y1 - c.a2 * y2;
    return y2;
}

__host__ __device__ inline DampState damp_mul(const DampMat& M, const DampState& s) {
    DampState r;
    r.s1 = M.m[0][0] * s.s1 + M.m[0][1] * s.s2 + M.m[0][2] * s.s3 + M.m[0][3] * s.s4;
    r.s2 = M.m[1][0] * s.s1 + M.m[1][1] * s.s2 + M.m[1][2] * s.s3 + M.m[1][3] * s.s4;
    r.s3 = M.m[2][0] * s.s1 + M.m[2][1] * s.s2 + M.m[2][2] * s.s3 + M.m[2][3] * s.s4;
    r.s4 = M.m[3][0] * s.s1 + M.m[3][1] * s.s2 + M.m[3][2] * s.s3 + M.m[3][3] * s.s4;
    return r;
}

// band j's envelope at t taps past the origin: ish_tap's expression
__host__ __device__ inline double damp_env(uint64_t t60, uint64_t t) {
    return t60 ? exp2(-((double)t * ISH_DECAY_K) / (double)t60) : 1.0;
}

__device__ inline DampState damp_load(const double2* __restrict__ st, uint64_t at) {
    const double2 a = st[2 * at], b = st[2 * at + 1];
    return DampState{a.x, a.y, b.x, b.y};
}
__device__ inline void damp_store(double2* __restrict__ st, uint64_t at, const DampState& s) {
    st[2 * at] = make_double2(s.s1, s.s2);
    st[2 * at + 1] = make_double2(s.s3, s.s4);
}

// One pass over buf [n] (the file's head).  st: double2 [X][gridDim.x * IEQ_THREADS][2], crossover k's state of lane
// 2 * chunk + channel at (k * lanes + lane).  FIX = false: every crossover from rest, the end states to st, buf is only
// read.  FIX = true: every crossover from the state st holds, y written over x.  Taps at and past n read as zero and are
// not written.  pl.origin <= n.
template <bool FIX>
__global__ __launch_bounds__(IEQ_THREADS) void k_damp_chunk(double2* __restrict__ buf, uint64_t n, DampPlan pl, double2* __restrict__ st) {
    const uint64_t lanes = (uint64_t)gridDim.x * IEQ_THREADS, entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    DampState s[MC_DAMP_MAX_XOVERS];
#pragma unroll
    for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++) {
        s[k] = DampState{0.0, 0.0, 0.0, 0.0};
        if (FIX && k < pl.X) s[k] = damp_load(st, (uint64_t)k * lanes + entry);
    }
    chunk_walk<false, IEQ_TILE, double2>(
        FIX, [&](uint64_t g, double2& v) { v = g < n ? buf[g] : make_double2(0.0, 0.0); },
        [&](double& tap, uint64_t m) {
            const double v = tap;
            double P[MC_DAMP_MAX_XOVERS];
#pragma unroll
            for (int x = 0; x < MC_DAMP_MAX_XOVERS; x++)
                if (x < pl.X) P[x] = damp_step(pl.c[x], s[x], v);
            if (FIX) {
                const uint64_t tt = (m > pl.origin ? m : pl.origin) - pl.origin;
                // y = g_X x + (g_0 - g_1) P_1 + .. + (g_(X-1) - g_X) P_X, added in that order: the weights first, low to high
                double g = damp_env(pl.t60[0], tt), w[MC_DAMP_MAX_XOVERS];
#pragma unroll
                for (int x = 0; x < MC_DAMP_MAX_XOVERS; x++)
                    if (x < pl.X) {
                        const double gn = damp_env(pl.t60[x + 1], tt);
                        w[x] = g - gn;
                        g = gn;
                    }
                double y = g * v;
#pragma unroll
                for (int x = 0; x < MC_DAMP_MAX_XOVERS; x++)
                    if (x < pl.X) y += w[x] * P[x];
                tap = y;
            }
        },
        [&](uint64_t g, double2 v) {
            if (g < n) buf[g] = v;
        });
    if (!FIX) {
#pragma unroll
        for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++)
            if (k < pl.X) damp_store(st, (uint64_t)k * lanes + entry, s[k]);
    }
}

// Workgroup k (one per crossover): ireq.hip.h's carry_scan over its slice of st, entry 2 c + ch, c < nchunks, with 4-vectors.
// M = A^IEQ_CHUNK, MK = M^K.
__global__ __launch_bounds__(2 * IEQ_RUNS) void k_damp_carry(double2* __restrict__ st, uint64_t lanes, uint32_t nchunks, uint32_t K, DampCarry cm) {
    const DampMat &M = cm.M[blockIdx.x], &MK = cm.MK[blockIdx.x];
    double2* my = st + 2 * (uint64_t)blockIdx.x * lanes;
    carry_scan<DampState>(
        nchunks, K, [&](uint64_t i) { return damp_load(my, i); }, [&](uint64_t i, const DampState& s) { damp_store(my, i, s); },
        [&](bool runs, const DampState& s, const DampState& e) {
            const DampState r = damp_mul(runs ? MK : M, s);
            return DampState{r.s1 + e.s1, r.s2 + e.s2, r.s3 + e.s3, r.s4 + e.s4};
        });
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a damping that is on (n_xovers != 0), checked without touching an engine or HIP; the message
// (thread-local) names the field.  Null when it is good.
inline const char* damp_check(const mc_ir_damp* d, uint32_t ir_rate, uint32_t session_rate) {
    static thread_local char msg[200];
    if (d->struct_size != sizeof(mc_ir_damp)) return "mc_ir_damp struct_size mismatch";
    if (d->n_xovers > MC_DAMP_MAX_XOVERS) {
        std::snprintf(msg, sizeof(msg), "n_xovers %u above %d", d->n_xovers, MC_DAMP_MAX_XOVERS);
        return msg;
    }
    for (int k = 0; k < 2; k++) {
        const uint32_t r = k ? ir_rate : session_rate;
        if (r < 8000 || r > 384000) {
            std::snprintf(msg, sizeof(msg), "%s %u outside [8000, 384000] (damping needs the session's rate)", k ? "ir_rate" : "session_rate", r);
            return msg;
        }
    }
    const double top = IEQ_MAX_NYQ * (double)session_rate;
    for (uint32_t k = 0; k < d->n_xovers; k++) {
        const double f = (double)d->xover_hz[k];
        if (!(std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top)) {
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g outside [%g, %g]", k, f, IEQ_MIN_HZ, top);
            return msg;
        }
        if (k && !(d->xover_hz[k] > d->xover_hz[k - 1])) {
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g not above xover_hz[%u] %g: the crossovers must ascend strictly", k, f, k - 1,
                          (double)d->xover_hz[k - 1]);
            return msg;
        }
    }
    return nullptr;
}

// a checked damping that is on
inline DampPlan damp_plan(const mc_ir_damp& d, uint32_t session_rate) {
    DampPlan pl{};
    pl.X = (int)d.n_xovers;
    for (int k = 0; k < pl.X; k++) pl.c[k] = ieq_coef(mc_eq_band{MC_EQ_HIGHCUT, d.xover_hz[k], 0.f, 0.70710678f}, session_rate);
    for (int j = 0; j <= pl.X; j++) pl.t60[j] = d.decay_t60[j];
    pl.origin = d.origin;
    return pl;
}

// 20 log10 |g_X + sum_k (g_(k-1) - g_k) H_k(e^{jw})^2| at stored tap `tap`
inline double damp_response_db(const DampPlan& pl, uint32_t rate, uint64_t tap, double hz) {
    const double w = 2.0 * M_PI * hz / (double)rate, c1 = std::cos(w), s1 = std::sin(w), c2 = std::cos(2.0 * w), s2 = std::sin(2.0 * w);
    const uint64_t tt = (tap > pl.origin ? tap : pl.origin) - pl.origin;
    double g = damp_env(pl.t60[0], tt), re = 0.0, im = 0.0;
    for (int k = 0; k < pl.X; k++) {
        const IeqCoef& c = pl.c[k];
        const double nr = c.b0 + c.b1 * c1 + c.b2 * c2, ni = -(c.b1 * s1 + c.b2 * s2);
        const double dr = 1.0 + c.a1 * c1 + c.a2 * c2, di = -(c.a1 * s1 + c.a2 * s2), dd = dr * dr + di * di;
        const double hr = (nr * dr + ni * di) / dd, hi = (ni * dr - nr * di) / dd;  // one section
        const double gn = damp_env(pl.t60[k + 1], tt), wk = g - gn;
        re += wk * (hr * hr - hi * hi);
        im += wk * (2.0 * hr * hi);
        g = gn;
    }
    re += g;
    return 10.0 * std::log10(re * re + im * im);
}

// A of a crossover: column j = what damp_step makes of the unit state j at x = 0
inline DampMat damp_matrix(const IeqCoef& c) {
    DampMat A;
    for (int j = 0; j < 4; j++) {
        DampState s{j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, j == 3 ? 1.0 : 0.0};
        (void)damp_step(c, s, 0.0);
        A.m[0][j] = s.s1, A.m[1][j] = s.s2, A.m[2][j] = s.s3, A.m[3][j] = s.s4;
    }
    return A;
}
// The carry pass's matrices for the X crossovers c, runs of K chunks: ireq.hip.h's carry_powers (long double, rounded once; squared in
// double, the powers' own rounding was 3e-7 relative RMS of the result over 70 000 taps of a 10 Hz crossover at 384 kHz; 2e-9 so)
inline DampCarry damp_carry(const IeqCoef* c, int X, uint32_t K) {
    DampCarry cm{};
    for (int k = 0; k < X; k++) carry_powers<4>(damp_matrix(c[k]).m, K, cm.M[k].m, cm.MK[k].m);
    return cm;
}

// Step 6a over d_buf [n] in place, on the stream, after what the stream already holds.  Allocates the state scratch, waits for
// the kernels and frees it.
inline hipError_t damp_run(hipStream_t stream, double2* d_buf, uint64_t n, const DampPlan& plan) {
    DampPlan pl = plan;
    pl.origin = std::min<uint64_t>(pl.origin, n);
    const ChunkGeom cg = chunk_geom(n);
    const DampCarry cm = damp_carry(pl.c, pl.X, cg.K);
    DevArray<double2> d_st;
    hipError_t er = d_st.alloc(2 * (size_t)pl.X * cg.lanes);
    if (er != hipSuccess) return er;
    hipLaunchKernelGGL(k_damp_chunk<false>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, n, pl, d_st);
    er = hipGetLastError();
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_damp_carry, dim3(pl.X), dim3(2 * IEQ_RUNS), 0, stream, d_st, cg.lanes, cg.nchunks, cg.K, cm);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_damp_chunk<true>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, n, pl, d_st);
        er = hipGetLastError();
    }
    const hipError_t sy = hipStreamSynchronize(stream);
    return er != hipSuccess ? er : sy;
}
