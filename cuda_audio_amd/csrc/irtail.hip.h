// irtail.hip.h — the tail step of an impulse-response load (mc_load_ir_tail, mc_load_ir_sweep_tail): every frequency band of
// the frames is cut at its knee, or cross-faded there into decaying noise that continues the band's slope at the band's level.
// No reference equivalent.  Step 1a of the shaped load (include/mcconv.h has the definition, DESIGN.md 2.13 the reasons):
// shape_stage runs tail_run on the F frames the source left and hands irshape.hip.h the F' frames it makes.
// tests/ir_tail_np.py states the same with sequential float64 loops.
//
//   y[m] = fo_X x + sum_k (fo_(k-1) - fo_k) P_k(x) + [extend] q_X v + sum_k (q_(k-1) - q_k) P_k(v),   k = 1 .. X,
// irdamp.hip.h's rearrangement of sum_j fo_j B_j(x) + sum_j q_j B_j(v), used twice: X filters per signal and no band buffers.
// fo_j, fi_j are band j's power-complementary fades around its knee K_j, q_j = fi_j A_j g_j the level and decay of its noise,
// v the Gaussian noise of irsynth.hip.h's generator on Philox stream 3.
//
// The kernel is irdamp.hip.h's chunked recurrence with two signals: a lane owns one (chunk, channel) and carries 2 X crossover
// states, X for x and X for v; chunking, workgroup shape and the padded LDS rows are chunkwalk.hip.h's chunk_walk.  x comes in as
// float2 and is staged as double2; v is generated per frame in the lane (one Philox block, one Box-Muller pair in double, a second pair only
// for a right channel that is mixed from both) and never stored; y leaves as float2, rounded once.
//   local  k_tail_chunk<false> runs the crossovers over every chunk from rest and keeps the end states of both signals;
//   carry  k_damp_carry, unchanged, once per signal;
//   fix-up k_tail_chunk<true> runs every chunk again from its true states, evaluates the fades and q from the frame's own
//          index (a frame does not depend on where its chunk starts) and writes y.
// Frames before the first touched one are handed on as they came: with every fo = 1 the filters cancel exactly, and the copy
// also keeps the sign of a zero.  With X = 0 there is no state: the fix-up alone runs.
//
// Determinism.  Chunks, runs and grids depend on F' alone; no atomics; nothing is combined out of order.
#pragma once
#include "irdamp.hip.h"
#include "irsynth.hip.h"

constexpr int TAIL_BANDS = MC_DAMP_MAX_XOVERS + 1;
constexpr uint64_t TAIL_MAX_FRAMES = 1ull << 24;
constexpr int TAIL_BETA_POINTS = 8192;
constexpr uint32_t TAIL_STREAM = 3;   // W(m, 3): irsynth.hip.h uses streams 0 .. 2

// a checked mc_ir_tail as the kernels take it
struct TailPlan {
    int X;
    uint32_t key0, key1;
    uint32_t touched;                // bands with K_j < F'
    uint64_t F, Fp;                  // frames of the source, frames made
    uint64_t first;                  // first frame changed; Fp when no band is touched
    IeqCoef c[MC_DAMP_MAX_XOVERS];   // one section of crossover k + 1
    uint64_t lo[TAIL_BANDS], knee[TAIL_BANDS];  // K_j - W_j and K_j; both ~0 for a band that is left alone
    double t60[TAIL_BANDS];
    double A[TAIL_BANDS][2];
    double rho, rho_c;               // rho_c = sqrt(1 - rho^2)
};

// band j's fades at frame m
__device__ inline void tail_fades(const TailPlan& p, int j, uint64_t m, double& fo, double& fi) {
    if (m < p.lo[j]) {
        fo = 1.0, fi = 0.0;
    } else if (m >= p.knee[j]) {
        fo = 0.0, fi = 1.0;
    } else {
        const double theta = (M_PI / 2.0) * (double)(m - p.lo[j] + 1) / (double)(p.knee[j] - p.lo[j] + 1);
        fo = cos(theta), fi = sin(theta);
    }
}

// q_j of channel ch at frame m for a fade-in fi
__device__ inline double tail_q(const TailPlan& p, int j, int ch, uint64_t m, double fi) {
    if (!(fi > 0.0)) return 0.0;
    const double g = exp2(-((double)((int64_t)m - (int64_t)p.knee[j]) * ISH_DECAY_K) / p.t60[j]);
    return fi * g * p.A[j][ch];
}

__device__ inline double tail_normal(uint32_t a, uint32_t b) { return sqrt(-2.0 * log(syn_u(a))) * cos(2.0 * M_PI * syn_u(b)); }

// v of channel ch at frame m: gA for the left, rho gA + rho_c gB for the right
__device__ inline double tail_noise(const TailPlan& p, uint32_t m, int ch) {
    const SynWords w = syn_philox(m, 0u, TAIL_STREAM, 0u, p.key0, p.key1);
    double g = tail_normal(ch ? w.w2 : w.w0, ch ? w.w3 : w.w1);
    if (ch && p.rho != 0.0) g = p.rho * tail_normal(w.w0, w.w1) + p.rho_c * g;
    return g;
}

// One pass over the frames.  x [p.F] in (frames past F read as zero), y [p.Fp] out.  st: double2 [NOISE ? 2 X : X][gridDim.x *
// IEQ_THREADS][2], crossover k's state of lane 2 * chunk + channel at (k * lanes + lane) for x and at ((X + k) * lanes + lane)
// for v.  FIX = false: every crossover from rest, the end states to st, y untouched.  FIX = true: every crossover from the state
// st holds, y written.  NOISE: MC_TAIL_EXTEND.  Frames at and past Fp are not written.
template <bool FIX, bool NOISE>
__global__ __launch_bounds__(IEQ_THREADS) void k_tail_chunk(const float2* __restrict__ x, float2* __restrict__ y, TailPlan p, double2* __restrict__ st) {
    const int ch = threadIdx.x & 1;
    const uint64_t lanes = (uint64_t)gridDim.x * IEQ_THREADS, entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    DampState sx[MC_DAMP_MAX_XOVERS], sv[MC_DAMP_MAX_XOVERS];
#pragma unroll
    for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++) {
        sx[k] = sv[k] = DampState{0.0, 0.0, 0.0, 0.0};
        if (FIX && k < p.X) {
            sx[k] = damp_load(st, (uint64_t)k * lanes + entry);
            if (NOISE) sv[k] = damp_load(st, (uint64_t)(p.X + k) * lanes + entry);
        }
    }
    chunk_walk<false, 4, float2>(
        FIX, [&](uint64_t g, float2& v) { v = g < p.F && g < p.Fp ? x[g] : make_float2(0.f, 0.f); },
        [&](double& tap, uint64_t m) {
            const double vx = tap;
            const double vn = NOISE ? tail_noise(p, (uint32_t)m, ch) : 0.0;
            double Px[MC_DAMP_MAX_XOVERS], Pv[MC_DAMP_MAX_XOVERS];
#pragma unroll
            for (int i = 0; i < MC_DAMP_MAX_XOVERS; i++)
                if (i < p.X) {
                    Px[i] = damp_step(p.c[i], sx[i], vx);
                    if (NOISE) Pv[i] = damp_step(p.c[i], sv[i], vn);
                }
            if (FIX) {
                double out = vx;  // (before the first touched frame: the input's bits)
                if (m >= p.first) {
                    // fo_X x + (fo_0 - fo_1) P_1(x) + .. and then the same of q and v, added in that order
                    double fo, fi, wf[MC_DAMP_MAX_XOVERS], wq[MC_DAMP_MAX_XOVERS];
                    tail_fades(p, 0, m, fo, fi);
                    double q = NOISE ? tail_q(p, 0, ch, m, fi) : 0.0;
#pragma unroll
                    for (int i = 0; i < MC_DAMP_MAX_XOVERS; i++)
                        if (i < p.X) {
                            double fon, fin;
                            tail_fades(p, i + 1, m, fon, fin);
                            const double qn = NOISE ? tail_q(p, i + 1, ch, m, fin) : 0.0;
                            wf[i] = fo - fon, wq[i] = q - qn;
                            fo = fon, q = qn;
                        }
                    out = fo * vx;
#pragma unroll
                    for (int i = 0; i < MC_DAMP_MAX_XOVERS; i++)
                        if (i < p.X) out += wf[i] * Px[i];
                    if (NOISE) {
                        out += q * vn;
#pragma unroll
                        for (int i = 0; i < MC_DAMP_MAX_XOVERS; i++)
                            if (i < p.X) out += wq[i] * Pv[i];
                    }
                }
                tap = out;
            }
        },
        [&](uint64_t g, double2 v) {
            if (g < p.Fp) y[g] = make_float2((float)v.x, (float)v.y);
        });
    if (!FIX) {
#pragma unroll
        for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++)
            if (k < p.X) {
                damp_store(st, (uint64_t)k * lanes + entry, sx[k]);
                if (NOISE) damp_store(st, (uint64_t)(p.X + k) * lanes + entry, sv[k]);
            }
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a tail that is on, in the struct's order, checked without touching an engine or HIP; the message
// (thread-local) names the field.  session_rate bounds the crossovers from above when it is a rate at all (the rates
// themselves are the caller's next check).  Null when it is good.
inline const char* tail_check(const mc_ir_tail* t, uint32_t session_rate) {
    static thread_local char msg[200];
    if (t->struct_size != sizeof(mc_ir_tail)) return "mc_ir_tail struct_size mismatch";
    msg[0] = 0;
    if (t->mode > MC_TAIL_EXTEND) {
        std::snprintf(msg, sizeof(msg), "mode %u is not an MC_TAIL_* value", t->mode);
        return msg;
    }
    if (t->n_xovers > MC_DAMP_MAX_XOVERS) {
        std::snprintf(msg, sizeof(msg), "n_xovers %u above %d", t->n_xovers, MC_DAMP_MAX_XOVERS);
        return msg;
    }
    const bool rated = session_rate >= 8000 && session_rate <= 384000;
    const double top = rated ? IEQ_MAX_NYQ * (double)session_rate : std::numeric_limits<double>::infinity();
    for (uint32_t k = 0; k < t->n_xovers; k++) {
        const double f = (double)t->xover_hz[k];
        if (!(std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top))
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g outside [%g, %g]", k, f, IEQ_MIN_HZ, IEQ_MAX_NYQ * (double)session_rate);
        else if (k && !(t->xover_hz[k] > t->xover_hz[k - 1]))
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g not above xover_hz[%u] %g: the crossovers must ascend strictly", k, f, k - 1,
                          (double)t->xover_hz[k - 1]);
        if (msg[0]) return msg;
    }
    if (!(t->width >= 0.f && t->width <= 1.f)) {
        std::snprintf(msg, sizeof(msg), "width %g outside [0, 1]", (double)t->width);
        return msg;
    }
    if (t->length > TAIL_MAX_FRAMES) {
        std::snprintf(msg, sizeof(msg), "length %llu above %llu", (unsigned long long)t->length, (unsigned long long)TAIL_MAX_FRAMES);
        return msg;
    }
    if (t->mode == MC_TAIL_EXTEND) {
        for (uint32_t j = 0; j <= t->n_xovers; j++)
            if (!t->t60[j]) {
                std::snprintf(msg, sizeof(msg), "t60[%u] must be > 0 to extend", j);
                return msg;
            }
        for (uint32_t j = 0; j <= t->n_xovers; j++)
            for (int c = 0; c < 2; c++)
                if (!std::isfinite(t->level_db[j][c])) {
                    std::snprintf(msg, sizeof(msg), "level_db[%u][%d] %g must be finite", j, c, (double)t->level_db[j][c]);
                    return msg;
                }
    }
    return nullptr;
}

// F' of a checked tail over F source frames, refused when it leaves [1, 2^24]
inline const char* tail_check_frames(const mc_ir_tail* t, uint64_t F) {
    static thread_local char msg[160];
    const uint64_t Fp = t->length ? t->length : F;
    if (Fp >= 1 && Fp <= TAIL_MAX_FRAMES) return nullptr;
    std::snprintf(msg, sizeof(msg), "length 0 takes the IR's %llu frames at the session's rate, outside [1, %llu]", (unsigned long long)F,
                  (unsigned long long)TAIL_MAX_FRAMES);
    return msg;
}

// beta_j, j = 0 .. X: the share of white noise that band j of the split passes
inline void tail_beta(const IeqCoef* cs, int X, double beta[TAIL_BANDS]) {
    for (int j = 0; j < TAIL_BANDS; j++) beta[j] = j ? 0.0 : 1.0;
    if (!X) return;
    beta[0] = 0.0;
    for (int i = 0; i < TAIL_BETA_POINTS; i++) {
        const double w = M_PI * ((double)i + 0.5) / (double)TAIL_BETA_POINTS;
        const double c1 = std::cos(w), s1 = std::sin(w), c2 = std::cos(2.0 * w), s2 = std::sin(2.0 * w);
        double re[MC_DAMP_MAX_XOVERS], im[MC_DAMP_MAX_XOVERS];  // H_k^2
        for (int k = 0; k < X; k++) {
            const IeqCoef& c = cs[k];
            const double nr = c.b0 + c.b1 * c1 + c.b2 * c2, ni = -(c.b1 * s1 + c.b2 * s2);
            const double dr = 1.0 + c.a1 * c1 + c.a2 * c2, di = -(c.a1 * s1 + c.a2 * s2), dd = dr * dr + di * di;
            const double hr = (nr * dr + ni * di) / dd, hi = (ni * dr - nr * di) / dd;
            re[k] = hr * hr - hi * hi, im[k] = 2.0 * hr * hi;
        }
        for (int j = 0; j <= X; j++) {
            const double br = (j < X ? re[j] : 1.0) - (j ? re[j - 1] : 0.0), bi = (j < X ? im[j] : 0.0) - (j ? im[j - 1] : 0.0);
            beta[j] += br * br + bi * bi;
        }
    }
    for (int j = 0; j <= X; j++) beta[j] /= (double)TAIL_BETA_POINTS;
}

// a checked tail that is on, over F source frames in a session at session_rate
inline TailPlan tail_plan(const mc_ir_tail& t, uint32_t session_rate, uint64_t F) {
    TailPlan p{};
    p.X = (int)t.n_xovers;
    p.key0 = (uint32_t)(t.seed & 0xffffffffull);
    p.key1 = (uint32_t)(t.seed >> 32);
    p.F = F;
    p.Fp = t.length ? t.length : F;
    p.first = p.Fp;
    for (int k = 0; k < p.X; k++) p.c[k] = ieq_coef(mc_eq_band{MC_EQ_HIGHCUT, t.xover_hz[k], 0.f, 0.70710678f}, session_rate);
    double beta[TAIL_BANDS];
    tail_beta(p.c, p.X, beta);
    for (int j = 0; j < TAIL_BANDS; j++) {
        p.lo[j] = p.knee[j] = ~0ull;
        p.t60[j] = 1.0;
        if (j > p.X || t.knee[j] >= p.Fp) continue;
        p.touched++;
        p.knee[j] = t.knee[j];
        p.lo[j] = t.knee[j] - std::min<uint64_t>(t.fade, t.knee[j]);
        p.first = std::min(p.first, p.lo[j]);
        if (t.mode != MC_TAIL_EXTEND) continue;
        p.t60[j] = (double)t.t60[j];
        for (int c = 0; c < 2; c++) p.A[j][c] = std::sqrt(std::pow(10.0, (double)t.level_db[j][c] / 10.0) / beta[j]);
    }
    p.rho = 1.0 - (double)t.width;
    p.rho_c = std::sqrt(1.0 - p.rho * p.rho);
    return p;
}

// Step 1a: the p.Fp frames into d_y from the p.F frames d_x, on the stream, after what the stream already holds.  Allocates
// the state scratch, waits for the kernels and frees it.
inline hipError_t tail_run(hipStream_t stream, const float2* d_x, float2* d_y, const TailPlan& p, bool extend) {
    const ChunkGeom cg = chunk_geom(p.Fp);
    const uint64_t lanes = cg.lanes;
    const int signals = extend ? 2 : 1;
    DevArray<double2> d_st;
    hipError_t er = hipSuccess;
    if (p.X) {
        const DampCarry cm = damp_carry(p.c, p.X, cg.K);
        er = d_st.alloc(2 * (size_t)signals * p.X * lanes);
        if (er != hipSuccess) return er;
        if (extend)
            hipLaunchKernelGGL((k_tail_chunk<false, true>), dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_x, d_y, p, d_st);
        else
            hipLaunchKernelGGL((k_tail_chunk<false, false>), dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_x, d_y, p, d_st);
        er = hipGetLastError();
        for (int s = 0; s < signals && er == hipSuccess; s++) {
            hipLaunchKernelGGL(k_damp_carry, dim3(p.X), dim3(2 * IEQ_RUNS), 0, stream, d_st + 2 * (size_t)s * p.X * lanes, lanes, cg.nchunks, cg.K, cm);
            er = hipGetLastError();
        }
    }
    if (er == hipSuccess) {
        if (extend)
            hipLaunchKernelGGL((k_tail_chunk<true, true>), dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_x, d_y, p, d_st);
        else
            hipLaunchKernelGGL((k_tail_chunk<true, false>), dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_x, d_y, p, d_st);
        er = hipGetLastError();
    }
    const hipError_t sy = hipStreamSynchronize(stream);
    return er != hipSuccess ? er : sy;
}
