// ireq.hip.h — equalisation of an impulse response on load (mc_load_ir_eq): low cut, high cut, two shelves and peak bands,
// each one biquad with the Audio-EQ-Cookbook coefficients (include/mcconv.h writes them out).  No reference equivalent.
//
// The wet path is linear, so the bands filter the IR once instead of the signal for ever.  This is step 6b of the shaped load:
// irshape.hip.h selects the n taps (ish_shape), then ieq_finish
//   1. materialises the shaped taps before the gain as double2 [n] (k_eq_fill: ish_tap, the expression k_shape_apply uses);
//   1a. damps that buffer in place when the load is mc_load_ir_damped's (step 6a, damp_run of irdamp.hip.h);
//   2. runs every band over that buffer in place, in index order, as a chunked linear recurrence (below);
//   3. measures max |tap| and sum (L^2 + R^2) of the result (k_eq_store<false>), derives the gain, stores (float)(tap * gain)
//      and reduces the four sums mc_ir_info reports (k_eq_store<true>).
// tests/ir_eq_np.py states the same with one sequential float64 loop.
//
// The recurrence.  A band is the transposed direct form II
//     y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y
// whose state (s1, s2) after a run of taps is affine in the state before it: s' = A^len s + e, A = [[-a1, 1], [-a2, 0]], e =
// the state the run leaves when it starts at rest.  The n taps are cut into chunks of IEQ_CHUNK; a lane owns one (chunk,
// channel).
//   local  k_eq_chunk runs the band over every chunk from rest and keeps e_c, nothing else;
//   carry  k_eq_carry turns them into the states the chunks really start with, s_0 = 0, s_(c+1) = A^IEQ_CHUNK s_c + e_c: one
//          workgroup, 128 runs of chunks per channel, each scanned by its lane, the runs' ends by one lane, then each run again
//          from its true start;
//   fix-up k_eq_chunk runs the band over every chunk again, from s_c, and writes y.  (By linearity that is the local pass's
//          output plus the homogeneous response of s_c; running it this way costs the same reads, one write less, and what is
//          stored is the sequential recurrence's own arithmetic.)
// The fix-up of band k feeds what it writes to band k + 1 from rest in the same loop, so it is band k + 1's local pass as
// well: B bands take B + 1 launches of k_eq_chunk and B of k_eq_carry.
//
// Memory.  k_eq_chunk is one chunk_walk of chunkwalk.hip.h, whose head says how the taps reach the lanes (64 chunks x 2 channels
// per workgroup, IEQ_TILE taps of every chunk staged through padded LDS rows, the next tile's loads under the arithmetic).
//
// Determinism.  Chunks and runs depend on n alone; no atomics; every reduction ends in one partial per workgroup, combined
// on the host in index order (as irshape.hip.h does).  The same frames, shape and bands give the same bits.
#pragma once
#include "chunkwalk.hip.h"
#include "irshape.hip.h"

constexpr double IEQ_MIN_HZ = 10.0, IEQ_MAX_NYQ = 0.45, IEQ_MIN_Q = 0.1, IEQ_MAX_Q = 32.0, IEQ_MIN_DB = -36.0, IEQ_MAX_DB = 24.0;

// one band, a0 = 1
struct IeqCoef {
    double b0, b1, b2, a1, a2;
};
struct IeqStage {
    IeqCoef c;
    int on;
};
struct IeqMat {
    double m00, m01, m10, m11;
};
// the bands that are on, in order
struct IeqCascade {
    int bands;
    IeqCoef c[MC_EQ_MAX_BANDS];
};

__host__ __device__ inline double2 ieq_mul(const IeqMat& M, double2 s) { return make_double2(M.m00 * s.x + M.m01 * s.y, M.m10 * s.x + M.m11 * s.y); }

// buf[m] = tap m of the shaped IR before the gain
__global__ __launch_bounds__(ISH_THREADS) void k_eq_fill(const float2* __restrict__ x, IshPlan pl, double2* __restrict__ buf) {
    const uint64_t m = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x;
    if (m >= pl.n) return;
    double L, R;
    ish_tap(x, pl, m, L, R);
    buf[m] = make_double2(L, R);
}

// One pass over buf [n] (the file's head).  cur.on: every chunk runs through `cur` from the state st holds for it and is
// written back.  nxt.on: what the chunk now holds runs through `nxt` from rest; the state that leaves replaces the lane's
// entry of st (read at the start, written at the end, by the same lane).  st: double2 [gridDim.x * IEQ_THREADS], entry
// 2 * chunk + channel.  Taps at and past n read as zero and are not written.
__global__ __launch_bounds__(IEQ_THREADS) void k_eq_chunk(double2* __restrict__ buf, uint64_t n, IeqStage cur, IeqStage nxt, double2* __restrict__ st) {
    const uint64_t entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    double s1 = 0.0, s2 = 0.0, u1 = 0.0, u2 = 0.0;
    if (cur.on) {
        const double2 s = st[entry];
        s1 = s.x;
        s2 = s.y;
    }
    chunk_walk<false, IEQ_TILE, double2>(
        cur.on, [&](uint64_t g, double2& v) { v = g < n ? buf[g] : make_double2(0.0, 0.0); },
        [&](double& tap, uint64_t) {
            double v = tap;
            if (cur.on) {
                const double y = cur.c.b0 * v + s1;
                s1 = cur.c.b1 * v - cur.c.a1 * y + s2;
                s2 = cur.c.b2 * v - cur.c.a2 * y;
                tap = v = y;
            }
            if (nxt.on) {
                const double y = nxt.c.b0 * v + u1;
                u1 = nxt.c.b1 * v - nxt.c.a1 * y + u2;
                u2 = nxt.c.b2 * v - nxt.c.a2 * y;
            }
        },
        [&](uint64_t g, double2 v) {
            if (g < n) buf[g] = v;
        });
    if (nxt.on) st[entry] = make_double2(u1, u2);
}

// The carry pass over one channel pair's chunk states, c < nchunks: in, the state chunk c leaves when it starts at rest; out,
// the state it starts with.  One workgroup of 2 IEQ_RUNS lanes; lane (run, ch) owns chunks [run K, (run + 1) K): it scans its
// run, lanes 0 and 1 scan the runs' ends, and it scans its run again from its true start and writes.  load(i) / store(i, s):
// entry i = 2 c + ch; step(runs, s, e) = A s + e with A = the matrix of a chunk, or with `runs` that of a run of K chunks.
template <class S, class Load, class Store, class Step>
__device__ __forceinline__ void carry_scan(uint32_t nchunks, uint32_t K, Load&& load, Store&& store, Step&& step) {
    __shared__ S ends[2 * IEQ_RUNS];
    const int t = threadIdx.x, ch = t & 1;
    const uint64_t r0 = (uint64_t)(t >> 1) * K, c0 = r0 < nchunks ? r0 : nchunks, c1 = c0 + K < nchunks ? c0 + K : nchunks;
    S s{};
    for (uint64_t c = c0; c < c1; c++) s = step(false, s, load(2 * c + ch));
    ends[t] = s;
    __syncthreads();
    if (t < 2) {  // (a run that is short or empty is the last or lies behind the last: what follows it is not used)
        S r{};
        for (int g = 0; g < IEQ_RUNS; g++) {
            const S e = ends[2 * g + t];
            ends[2 * g + t] = r;
            r = step(true, r, e);
        }
    }
    __syncthreads();
    s = ends[t];
    for (uint64_t c = c0; c < c1; c++) {
        const S e = load(2 * c + ch);
        store(2 * c + ch, s);
        s = step(false, s, e);
    }
}

// carry_scan over st[2 c + ch].  M = A^IEQ_CHUNK, MK = M^K.
__global__ __launch_bounds__(2 * IEQ_RUNS) void k_eq_carry(double2* __restrict__ st, uint32_t nchunks, uint32_t K, IeqMat M, IeqMat MK) {
    carry_scan<double2>(
        nchunks, K, [&](uint64_t i) { return st[i]; }, [&](uint64_t i, double2 s) { st[i] = s; },
        [&](bool runs, double2 s, double2 e) {
            const double2 r = ieq_mul(runs ? MK : M, s);
            return make_double2(r.x + e.x, r.y + e.y);
        });
}

// k_shape_apply's two forms over the equalised taps.  WRITE = false: part[2 b] = max |tap|, part[2 b + 1] = sum (L^2 + R^2) of
// workgroup b.  WRITE = true: y[m] = (float)(tap * gain), part[4 b ..] = the workgroup's share of the four mc_ir_info sums.
template <bool WRITE>
__global__ __launch_bounds__(ISH_THREADS) void k_eq_store(const double2* __restrict__ buf, uint64_t n, double gain, float2* __restrict__ y,
                                                          double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t m = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x;
    const double2 v = m < n ? buf[m] : make_double2(0.0, 0.0);
    const auto add = [](double p, double q) { return p + q; };
    if (WRITE) {
        const float2 out = make_float2((float)(v.x * gain), (float)(v.y * gain));
        if (m < n) y[m] = out;
        const double sg = (threadIdx.x & 1) ? -1.0 : 1.0;  // (the workgroup's first m is even)
        const double s[4] = {(double)out.x, (double)out.y, sg * (double)out.x, sg * (double)out.y};
        for (int k = 0; k < 4; k++) {
            const double r = ish_block_reduce(s[k], red, add);
            if (threadIdx.x == 0) part[4 * (uint64_t)blockIdx.x + k] = r;
        }
    } else {
        const double pk = ish_block_reduce(fmax(fabs(v.x), fabs(v.y)), red, [](double p, double q) { return fmax(p, q); });
        const double sq = ish_block_reduce(v.x * v.x + v.y * v.y, red, add);
        if (threadIdx.x == 0) {
            part[2 * (uint64_t)blockIdx.x] = pk;
            part[2 * (uint64_t)blockIdx.x + 1] = sq;
        }
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// irdamp.hip.h: step 6a over the buffer ieq_finish has filled
inline hipError_t damp_run(hipStream_t stream, double2* d_buf, uint64_t n, const DampPlan& plan);

// The band's coefficients (include/mcconv.h), in double from the float fields.
inline IeqCoef ieq_coef(const mc_eq_band& b, uint32_t rate) {
    const double w0 = 2.0 * M_PI * (double)b.freq_hz / (double)rate, c = std::cos(w0), al = std::sin(w0) / (2.0 * (double)b.q);
    const double A = std::pow(10.0, (double)b.gain_db / 40.0), r = 2.0 * std::sqrt(A) * al;
    double b0, b1, b2, a0, a1, a2;
    switch (b.kind) {
        case MC_EQ_LOWCUT:
            b0 = (1.0 + c) / 2.0, b1 = -(1.0 + c), b2 = (1.0 + c) / 2.0;
            a0 = 1.0 + al, a1 = -2.0 * c, a2 = 1.0 - al;
            break;
        case MC_EQ_HIGHCUT:
            b0 = (1.0 - c) / 2.0, b1 = 1.0 - c, b2 = (1.0 - c) / 2.0;
            a0 = 1.0 + al, a1 = -2.0 * c, a2 = 1.0 - al;
            break;
        case MC_EQ_LOWSHELF:
            b0 = A * ((A + 1.0) - (A - 1.0) * c + r), b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * c), b2 = A * ((A + 1.0) - (A - 1.0) * c - r);
            a0 = (A + 1.0) + (A - 1.0) * c + r, a1 = -2.0 * ((A - 1.0) + (A + 1.0) * c), a2 = (A + 1.0) + (A - 1.0) * c - r;
            break;
        case MC_EQ_HIGHSHELF:
            b0 = A * ((A + 1.0) + (A - 1.0) * c + r), b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * c), b2 = A * ((A + 1.0) + (A - 1.0) * c - r);
            a0 = (A + 1.0) - (A - 1.0) * c + r, a1 = 2.0 * ((A - 1.0) - (A + 1.0) * c), a2 = (A + 1.0) - (A - 1.0) * c - r;
            break;
        default:  // MC_EQ_PEAK
            b0 = 1.0 + al * A, b1 = -2.0 * c, b2 = 1.0 - al * A;
            a0 = 1.0 + al / A, a1 = -2.0 * c, a2 = 1.0 - al / A;
            break;
    }
    return IeqCoef{b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
}

// Every field of an EQ, checked without touching an engine or HIP; the message (thread-local) names the field.  Null when it
// is good; *on = the bands that are on.  The rates are looked at only with a band on.
inline const char* ieq_check(const mc_ir_eq* eq, uint32_t ir_rate, uint32_t session_rate, int* on) {
    static thread_local char msg[160];
    *on = 0;
    if (!eq) return "null eq";
    if (eq->struct_size != sizeof(mc_ir_eq)) return "mc_ir_eq struct_size mismatch";
    for (int k = 0; k < MC_EQ_MAX_BANDS; k++) {
        if (eq->band[k].kind > MC_EQ_PEAK) {
            std::snprintf(msg, sizeof(msg), "band %d: kind %u is not an MC_EQ_* value", k, eq->band[k].kind);
            return msg;
        }
        *on += eq->band[k].kind != MC_EQ_OFF;
    }
    if (!*on) return nullptr;
    for (int k = 0; k < 2; k++) {
        const uint32_t r = k ? ir_rate : session_rate;
        if (r < 8000 || r > 384000) {
            std::snprintf(msg, sizeof(msg), "%s %u outside [8000, 384000] (a band that is on needs the session's rate)", k ? "ir_rate" : "session_rate", r);
            return msg;
        }
    }
    for (int k = 0; k < MC_EQ_MAX_BANDS; k++) {
        const mc_eq_band& b = eq->band[k];
        if (b.kind == MC_EQ_OFF) continue;
        const double f = (double)b.freq_hz, q = (double)b.q, g = (double)b.gain_db, top = IEQ_MAX_NYQ * (double)session_rate;
        const bool cut = b.kind == MC_EQ_LOWCUT || b.kind == MC_EQ_HIGHCUT;
        if (!(std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top))
            std::snprintf(msg, sizeof(msg), "band %d: freq_hz %g outside [%g, %g]", k, f, IEQ_MIN_HZ, top);
        else if (!(std::isfinite(q) && q >= IEQ_MIN_Q && q <= IEQ_MAX_Q))
            std::snprintf(msg, sizeof(msg), "band %d: q %g outside [%g, %g]", k, q, IEQ_MIN_Q, IEQ_MAX_Q);
        else if (!cut && !(std::isfinite(g) && g >= IEQ_MIN_DB && g <= IEQ_MAX_DB))
            std::snprintf(msg, sizeof(msg), "band %d: gain_db %g outside [%g, %g]", k, g, IEQ_MIN_DB, IEQ_MAX_DB);
        else
            continue;
        return msg;
    }
    return nullptr;
}

// the bands of a checked eq that are on
inline IeqCascade ieq_cascade(const mc_ir_eq& eq, uint32_t session_rate) {
    IeqCascade cs;
    cs.bands = 0;
    for (int k = 0; k < MC_EQ_MAX_BANDS; k++)
        if (eq.band[k].kind != MC_EQ_OFF) cs.c[cs.bands++] = ieq_coef(eq.band[k], session_rate);
    return cs;
}

// 20 log10 |H| of the cascade at hz
inline double ieq_response_db(const IeqCascade& cs, uint32_t rate, double hz) {
    const double w = 2.0 * M_PI * hz / (double)rate, c1 = std::cos(w), s1 = std::sin(w), c2 = std::cos(2.0 * w), s2 = std::sin(2.0 * w);
    double db = 0.0;
    for (int k = 0; k < cs.bands; k++) {
        const IeqCoef& c = cs.c[k];
        const double nr = c.b0 + c.b1 * c1 + c.b2 * c2, ni = -(c.b1 * s1 + c.b2 * s2);
        const double dr = 1.0 + c.a1 * c1 + c.a2 * c2, di = -(c.a1 * s1 + c.a2 * s2);
        db += 10.0 * std::log10((nr * nr + ni * ni) / (dr * dr + di * di));
    }
    return db;
}

// The chunk passes over n taps: workgroups of a chunk kernel, their lanes (= entries of a state array), chunks, and chunks per
// run of the carry pass.
struct ChunkGeom {
    unsigned grid;
    uint64_t lanes;
    uint32_t nchunks, K;
};
inline ChunkGeom chunk_geom(uint64_t n) {
    const unsigned grid = (unsigned)((n + IEQ_SPAN - 1) / IEQ_SPAN);
    const uint32_t nchunks = (uint32_t)((n + IEQ_CHUNK - 1) / IEQ_CHUNK);
    return ChunkGeom{grid, (uint64_t)grid * IEQ_THREADS, nchunks, (nchunks + IEQ_RUNS - 1) / IEQ_RUNS};
}

// The carry pass's matrices of a D x D recurrence matrix A (2: a band; 4: a crossover of irdamp.hip.h): M = A^IEQ_CHUNK and
// MK = M^K, by repeated squaring in long double, each rounded to double once, MK raised from the unrounded M.  A 10 Hz band at
// 384 kHz has its poles 2.6e-6 .. 1.2e-4 inside the circle and A^256 entries near 250 that cancel against each other: squared
// in double, the powers' own rounding (a 10 Hz high cut: 6e-12 of M, 3e-8 of MK at K = 16) was what the chunked form differed from
// the sequential recurrence by, 1e-4 relative RMS over the last eighth of 523 264 taps (DESIGN 2.8 has the figures before and after).
template <int D>
struct CarryMatL {
    long double m[D][D];
};
template <int D>
inline CarryMatL<D> carry_matmul(const CarryMatL<D>& a, const CarryMatL<D>& b) {
    CarryMatL<D> r;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) {
            long double v = 0.0L;
            for (int k = 0; k < D; k++) v += a.m[i][k] * b.m[k][j];
            r.m[i][j] = v;
        }
    return r;
}
template <int D>
inline CarryMatL<D> carry_matpow(CarryMatL<D> a, uint64_t p) {
    CarryMatL<D> r{};
    for (int i = 0; i < D; i++) r.m[i][i] = 1.0L;
    for (; p; p >>= 1, a = carry_matmul(a, a))
        if (p & 1) r = carry_matmul(r, a);
    return r;
}
template <int D>
inline void carry_powers(const double (&A)[D][D], uint32_t K, double (&M)[D][D], double (&MK)[D][D]) {
    CarryMatL<D> a;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) a.m[i][j] = (long double)A[i][j];
    const CarryMatL<D> m = carry_matpow(a, IEQ_CHUNK), mk = carry_matpow(m, K);
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) M[i][j] = (double)m.m[i][j], MK[i][j] = (double)mk.m[i][j];
}

// k_eq_carry's two matrices for one band (or one section of a decay band), runs of K chunks
struct IeqCarry {
    IeqMat M, MK;
};
inline IeqCarry ieq_carry(const IeqCoef& c, uint32_t K) {
    const double A[2][2] = {{-c.a1, 1.0}, {-c.a2, 0.0}};
    double M[2][2], MK[2][2];
    carry_powers<2>(A, K, M, MK);
    return IeqCarry{IeqMat{M[0][0], M[0][1], M[1][0], M[1][1]}, IeqMat{MK[0][0], MK[0][1], MK[1][0], MK[1][1]}};
}

// The rest of a load with EQ once ish_shape has resolved the plan (the file's head).  Same contract as ish_shape's own tail:
// *d_out = the n stored taps (the caller's), sums and info as there, info[7] = the bands applied.  Synchronises the stream.
// damp: the taps are damped before the bands see them (null: not).
inline hipError_t ieq_finish(hipStream_t stream, const float2* d_x, const IshPlan& pl, const mc_ir_shape& sh, const IeqCascade& eq,
                             float2** d_out, uint64_t* n_out, double sums[4], double info[8], const DampPlan* damp) {
    const uint64_t n = pl.n;
    const unsigned grid = (unsigned)((n + ISH_THREADS - 1) / ISH_THREADS);       // k_eq_fill, k_eq_store
    const ChunkGeom cg = chunk_geom(n);                                          // k_eq_chunk, k_eq_carry
    DevArray<double2> d_buf, d_st;
    DevArray<float2> d_y;
    DevArray<double> d_part;
    std::vector<double> part(4 * (size_t)grid);
    hipError_t er = d_buf.alloc(n);
    if (er == hipSuccess) er = d_st.alloc((size_t)cg.lanes);
    if (er == hipSuccess) er = d_y.alloc(n);
    if (er == hipSuccess) er = d_part.alloc(part.size());
    if (er == hipSuccess) er = d_st.zero(stream);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_eq_fill, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x, pl, d_buf);
        er = hipGetLastError();
    }
    if (er == hipSuccess && damp) er = damp_run(stream, d_buf, n, *damp);
    for (int k = 0; k <= eq.bands && er == hipSuccess; k++) {
        IeqStage cur{}, nxt{};
        if (k > 0) {
            cur.c = eq.c[k - 1], cur.on = 1;
            const IeqCarry cm = ieq_carry(cur.c, cg.K);
            hipLaunchKernelGGL(k_eq_carry, dim3(1), dim3(2 * IEQ_RUNS), 0, stream, d_st, cg.nchunks, cg.K, cm.M, cm.MK);
            er = hipGetLastError();
        }
        if (k < eq.bands) nxt.c = eq.c[k], nxt.on = 1;
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_eq_chunk, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, n, cur, nxt, d_st);
            er = hipGetLastError();
        }
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_eq_store<false>, dim3(grid), dim3(ISH_THREADS), 0, stream, d_buf, n, 1.0, (float2*)nullptr, d_part);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * 2 * grid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    if (er == hipSuccess) {
        double peak = 0.0, sq = 0.0, gain = 1.0;
        for (unsigned b = 0; b < grid; b++) {
            peak = std::max(peak, part[2 * (size_t)b]);
            sq += part[2 * (size_t)b + 1];
        }
        const double energy = std::sqrt(sq / 2.0);
        const double measure = sh.normalize == MC_NORM_PEAK ? peak : (sh.normalize == MC_NORM_ENERGY ? energy : 0.0);
        if (measure > 0.0) gain = (double)sh.target / measure;
        hipLaunchKernelGGL(k_eq_store<true>, dim3(grid), dim3(ISH_THREADS), 0, stream, d_buf, n, gain, d_y, d_part);
        er = hipGetLastError();
        const double inf[8] = {(double)pl.F, (double)pl.onset, (double)pl.first, (double)n, gain, peak, energy, (double)eq.bands};
        std::copy(inf, inf + 8, info);
    }
    if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * 4 * grid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    if (er != hipSuccess) return er;
    for (int k = 0; k < 4; k++) sums[k] = 0.0;
    for (unsigned b = 0; b < grid; b++)
        for (int k = 0; k < 4; k++) sums[k] += part[4 * (size_t)b + k];
    *d_out = d_y.release();  // (as ish_shape hands its taps out)
    *n_out = n;
    return hipSuccess;
}
