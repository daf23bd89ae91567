// irfloor.hip.h — the noise floor of a loaded impulse response, measured on the device (mc_ir_floor): Lundeby's search for the
// level of the noise, the knee where the decay meets it and the late decay rate, broadband and in the bands of irdamp.hip.h's
// crossover split.  No reference equivalent.  include/mcconv.h and DESIGN.md 2.13 hold the definition; tests/ir_floor_np.py
// states it in float64.  mc_ir_tail_from_floor, host arithmetic, turns a measurement into the tail step's struct (irtail.hip.h).
//
// The stored taps x [n] are only read.  With N = end ? min(end, n) : n and the origin o of irdecay.hip.h's Measure:
//   split   with X crossovers: k_dec_fill, then irdamp.hip.h's local pass and carry, unchanged (k_damp_chunk<false>,
//           k_damp_carry), leave every chunk's true starting states; they serve all X + 1 bands;
//   per row group (broadband, then band 0 .. X):
//     fill    k_dec_fill: buf[m] = (double) x[m];
//     band    k_flr_band, the fix-up pass of k_damp_chunk with the band's own combination in place of the envelopes: buf = B_j,
//             formed as damping forms it with band j's gain 1 and the others 0 (B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X);
//     sum     buf[m] = EDC[m], the backward sum (Measure::edc);
//     search  the host walks the three channel sets' rows through the search in step.  All it ever needs of EDC are values at
//             interval edges and at single taps: k_flr_gather fetches, per set, EDC at start + i step, i < count, in one launch per
//             means() and one per noise().  The interval means are differences of neighbouring edges; the regressions over at most
//             n1 / w points run on the host, as dec_row's do.
//
// Determinism.  Chunks, grids and the carries' order depend on N alone; no atomics; the gather has one writer per slot; the
// host works in index order.  The same query on the same taps gives the same bits.
//
// Scratch (double2 [N], the chunk states, the gathered edges) is allocated by the call and freed before it returns.
#pragma once
#include <algorithm>
#include <limits>
#include <vector>

#include "irdamp.hip.h"
#include "irdecay.hip.h"

constexpr int FLR_SETS = DEC_SETS;
constexpr uint64_t FLR_LEFT_ALONE = ~0ull;  // mc_ir_tail.knee of a band the tail step does not touch

// what k_flr_gather fetches for set s (0 = L, 1 = R, 2 = L + R): EDC at start[s] + i step[s], i < count[s]; out[at[s] + i]
struct FlrGather {
    uint64_t start[FLR_SETS], step[FLR_SETS], count[FLR_SETS], at[FLR_SETS];
};

// k_damp_chunk<true> with band j's combination: st holds every chunk's starting states (k_damp_carry's output), buf [n] = x in,
// B_j out.  The weights are damping's with g_j = 1 and every other gain 0, added in damping's order, so the band is exactly
// P_1, P_(j+1) - P_j or x - P_X.  Taps at and past n read as zero and are not written.
__global__ __launch_bounds__(IEQ_THREADS) void k_flr_band(double2* __restrict__ buf, uint64_t n, DampPlan pl, int band, const double2* __restrict__ st) {
    const uint64_t lanes = (uint64_t)gridDim.x * IEQ_THREADS, entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    DampState s[MC_DAMP_MAX_XOVERS];
#pragma unroll
    for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++) {
        s[k] = DampState{0.0, 0.0, 0.0, 0.0};
        if (k < pl.X) s[k] = damp_load(st, (uint64_t)k * lanes + entry);
    }
    // g_j = [j == band]; w_k = g_(k-1) - g_k for crossover k = 1 .. X (index k - 1)
    double w[MC_DAMP_MAX_XOVERS];
#pragma unroll
    for (int k = 0; k < MC_DAMP_MAX_XOVERS; k++) w[k] = (band == k ? 1.0 : 0.0) - (band == k + 1 ? 1.0 : 0.0);
    const double gX = band == pl.X ? 1.0 : 0.0;
    chunk_walk<false, IEQ_TILE, double2>(
        true, [&](uint64_t g, double2& v) { v = g < n ? buf[g] : make_double2(0.0, 0.0); },
        [&](double& tap, uint64_t) {
            const double v = tap;
            double y = gX * v;
#pragma unroll
            for (int x = 0; x < MC_DAMP_MAX_XOVERS; x++)
                if (x < pl.X) y += w[x] * damp_step(pl.c[x], s[x], v);
            tap = y;
        },
        [&](uint64_t g, double2 v) {
            if (g < n) buf[g] = v;
        });
}

// out[ga.at[s] + i] = EDC of set s at ga.start[s] + i ga.step[s], i < ga.count[s]; a tap at or past n: 0 (EDC[N] = 0).
// gridDim.x * ISH_THREADS >= the sum of the counts.
__global__ __launch_bounds__(ISH_THREADS) void k_flr_gather(const double2* __restrict__ buf, uint64_t n, FlrGather ga, double* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x;
    const int s = j < ga.at[1] ? 0 : (j < ga.at[2] ? 1 : 2);
    const uint64_t i = j - ga.at[s];
    if (i >= ga.count[s]) return;
    const uint64_t m = ga.start[s] + i * ga.step[s];
    out[j] = m < n ? dec_edc(buf[m], s) : 0.0;
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a query, in field order, checked without touching an engine or HIP; the message (thread-local) names the
// field.  Null when it is good.
inline const char* flr_check(const mc_floor_query* q) {
    static thread_local char msg[200];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_floor_query)) return "mc_floor_query struct_size mismatch";
    msg[0] = 0;
    const double top = IEQ_MAX_NYQ * (double)q->rate, tf = (double)q->tail_fraction;
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    if (q->n_xovers > MC_FLOOR_MAX_XOVERS)
        std::snprintf(msg, sizeof(msg), "n_xovers %u above %d", q->n_xovers, MC_FLOOR_MAX_XOVERS);
    if (msg[0]) return msg;
    for (uint32_t k = 0; k < q->n_xovers; k++) {
        const double f = (double)q->xover_hz[k];
        if (!(std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top))
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g outside [%g, %g]", k, f, IEQ_MIN_HZ, top);
        else if (k && !(q->xover_hz[k] > q->xover_hz[k - 1]))
            std::snprintf(msg, sizeof(msg), "xover_hz[%u] %g not above xover_hz[%u] %g: the crossovers must ascend strictly", k, f, k - 1,
                          (double)q->xover_hz[k - 1]);
        if (msg[0]) return msg;
    }
    if (!dec_onset_ok(q->onset_db, msg, sizeof(msg)))
        return msg;
    else if (!(tf > 0.0 && tf <= 0.5))
        std::snprintf(msg, sizeof(msg), "tail_fraction %g outside (0, 0.5]", tf);
    else if (!(q->margin_db >= 1.f && q->margin_db <= 30.f))
        std::snprintf(msg, sizeof(msg), "margin_db %g outside [1, 30]", (double)q->margin_db);
    else if (!(q->span_db >= 5.f && q->span_db <= 60.f))
        std::snprintf(msg, sizeof(msg), "span_db %g outside [5, 60]", (double)q->span_db);
    else if (q->per_decade < 1 || q->per_decade > 20)
        std::snprintf(msg, sizeof(msg), "per_decade %u outside [1, 20]", q->per_decade);
    else if (q->rounds < 1 || q->rounds > 16)
        std::snprintf(msg, sizeof(msg), "rounds %u outside [1, 16]", q->rounds);
    else if (q->reserved)
        std::snprintf(msg, sizeof(msg), "reserved %u must be 0", q->reserved);
    return msg[0] ? msg : nullptr;
}

inline uint32_t flr_groups(const mc_floor_query& q) { return 1 + (q.n_xovers ? q.n_xovers + 1 : 0); }

// One row's walk through the search (include/mcconv.h).  The caller feeds it what the device gathered: a value for noise(),
// the edges for means().
struct FlrRow {
    uint64_t o = 0, N = 0, n1 = 0, cap = 0, tail = 0;
    double margin = 0.0, span = 0.0;
    int status = 0;                  // 0 while the search runs
    double E = 0.0, Nz = 0.0, V = 0.0, a = 0.0, tc = 0.0, tc_prev = 0.0, pmax = 0.0;
    uint64_t w = 0;
    std::vector<double> P, D;

    void end(int st) { status = st; }
    // Nz = EDC[at] / (N - at); false (status 3) when it is 0
    bool noise(double edc, uint64_t at) {
        Nz = edc / (double)(N - at);
        V = 10.0 * std::log10(Nz);
        if (!(Nz > 0.0)) end(3);
        return status == 0;
    }
    // edges[i] = EDC[o + i w], i <= I
    void means(const double* edges, uint64_t width) {
        w = width;
        const uint64_t I = n1 / w;
        P.resize(I), D.resize(I);
        pmax = 0.0;
        for (uint64_t i = 0; i < I; i++) {
            P[i] = (edges[i] - edges[i + 1]) / (double)w;
            D[i] = 10.0 * std::log10(P[i]);
            pmax = std::max(pmax, P[i]);
        }
    }
    // fit over run(V), narrowed to the levels within span_db of the threshold when `narrow`; false (status 2) when there is none
    bool fit(bool narrow) {
        const uint64_t I = P.size();
        uint64_t ip = 0;
        for (uint64_t i = 1; i < I; i++)
            if (P[i] > P[ip]) ip = i;
        uint64_t iF = I;
        for (uint64_t i = ip; i < I; i++)
            if (D[i] < V + margin) {
                iF = i;
                break;
            }
        const double top = V + margin + span;
        if (narrow) {
            uint64_t low = 0;
            for (uint64_t i = ip; i < iF; i++) low += D[i] <= top;
            if (low < 2) narrow = false;
        }
        double n = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0, t0 = 0.0;
        for (uint64_t i = ip; i < iF; i++) {
            if (narrow && !(D[i] <= top)) continue;
            const double ti = (double)o + (double)i * (double)w + ((double)w - 1.0) / 2.0;
            if (n == 0.0) t0 = ti;
            const double x = ti - t0;
            n += 1.0, sx += x, sy += D[i], sxx += x * x, sxy += x * D[i];
        }
        if (n < 2.0) return end(2), false;
        const double slope = (n * sxy - sx * sy) / (n * sxx - sx * sx);
        if (!(std::isfinite(slope) && slope < 0.0)) return end(2), false;
        const double c = (sy - slope * sx) / n;
        a = slope;
        tc_prev = tc;
        tc = t0 + (V - c) / slope;
        return true;
    }
    uint64_t interval(uint32_t per_decade) const {
        const double v = std::floor(-10.0 / (a * (double)per_decade) + 0.5);
        return (uint64_t)std::min(std::max(v, 1.0), (double)cap);
    }
    uint64_t next_noise_tap() const {
        const double v = std::ceil(tc + margin / -a);
        return (uint64_t)std::min(std::max(v, (double)o), (double)(N - tail));
    }
    void write(double* row, uint32_t rate) const {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int k = 0; k < 8; k++) row[k] = nan;
        row[0] = E;
        row[7] = (double)status;
        if (status == 3) row[2] = (double)N;
        if (status) return;
        row[1] = Nz;
        row[2] = tc;
        row[3] = -60.0 / (a * (double)rate);
        row[4] = 10.0 * std::log10(pmax / Nz);
        row[5] = (double)w;
        row[6] = std::fabs(tc - tc_prev);
    }
};

// The three channel sets' rows of one row group, walked through the search in step.  gather(ga) fetches what ga names (EDC of
// the group at the taps it lists) into part [ga.at[s] + i] and fills ga.at; false when it fails, and so does the search.
// rows: [3 * 8].
template <class Gather>
inline bool flr_search(uint64_t o, uint64_t N, const mc_floor_query& q, Gather&& gather, const std::vector<double>& part, double* rows) {
    FlrRow row[FLR_SETS];
    for (FlrRow& r : row) {
        r.o = o, r.N = N, r.n1 = N - o, r.cap = r.n1 / 16;
        r.tail = std::max<uint64_t>(1, (uint64_t)std::floor((double)q.tail_fraction * (double)r.n1));
        r.margin = (double)q.margin_db, r.span = (double)q.span_db;
    }
    const auto alive = [&](int s) { return row[s].status == 0; };
    // E = EDC[o] and the first noise level, EDC[N - tail]
    FlrGather ga{};
    for (int s = 0; s < FLR_SETS; s++) ga.start[s] = o, ga.step[s] = N - row[s].tail - o, ga.count[s] = 2;
    if (!gather(ga)) return false;
    for (int s = 0; s < FLR_SETS; s++) {
        FlrRow& r = row[s];
        r.E = part[ga.at[s]];
        if (r.cap < 1 || !(r.E > 0.0))
            r.end(1);
        else
            r.noise(part[ga.at[s] + 1], N - r.tail);
    }
    // the first fit over intervals of w0 taps, then the interval the search keeps
    for (int pass = 0; pass < 2; pass++) {
        ga = FlrGather{};
        for (int s = 0; s < FLR_SETS; s++) {
            if (!alive(s)) continue;
            FlrRow& r = row[s];
            const uint64_t w0 = q.window ? q.window : (uint64_t)std::floor(0.03 * (double)q.rate + 0.5);
            r.w = pass ? r.interval(q.per_decade) : std::min<uint64_t>(w0, r.cap);
            ga.start[s] = o, ga.step[s] = r.w, ga.count[s] = r.n1 / r.w + 1;
        }
        if (!gather(ga)) return false;
        for (int s = 0; s < FLR_SETS; s++) {
            if (!alive(s)) continue;
            row[s].means(part.data() + ga.at[s], row[s].w);
            if (!pass) row[s].fit(false);
        }
    }
    for (uint32_t k = 0; k < q.rounds; k++) {
        ga = FlrGather{};
        uint64_t at[FLR_SETS] = {0, 0, 0};
        for (int s = 0; s < FLR_SETS; s++) {
            if (!alive(s)) continue;
            at[s] = row[s].next_noise_tap();
            ga.start[s] = at[s], ga.step[s] = 1, ga.count[s] = 1;
        }
        if (!gather(ga)) return false;
        for (int s = 0; s < FLR_SETS; s++)
            if (alive(s) && row[s].noise(part[ga.at[s]], at[s])) row[s].fit(true);
    }
    for (int s = 0; s < FLR_SETS; s++) row[s].write(rows + 8 * s, q.rate);
    return true;
}

// The whole measurement of the n stored taps d_x for a checked query.  rows, info as mc_ir_floor describes them.  Synchronises
// the stream; leaves nothing allocated.
inline hipError_t flr_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_floor_query& q, double* rows, uint64_t info[2]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const int X = (int)q.n_xovers;
    const unsigned grid = (unsigned)((N + ISH_THREADS - 1) / ISH_THREADS);                    // k_dec_fill
    const ChunkGeom& cg = m.cg;                                                               // the chunk passes
    std::vector<double> part;
    m.open(q.onset_db, N, 2 * (size_t)X * cg.lanes, cg.lanes, 16, 0);
    const uint64_t o = m.o;

    // the split's starting states, once for every band
    DampPlan pl{};
    pl.X = X;
    for (int k = 0; k < X; k++) pl.c[k] = ieq_coef(mc_eq_band{MC_EQ_HIGHCUT, q.xover_hz[k], 0.f, 0.70710678f}, q.rate);
    if (m.er == hipSuccess && X) {
        const DampCarry cm = damp_carry(pl.c, X, cg.K);
        hipLaunchKernelGGL(k_dec_fill, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x, N, m.d_buf);
        m.launched();
        if (m.er == hipSuccess) {
            hipLaunchKernelGGL(k_damp_chunk<false>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, m.d_buf, N, pl, m.d_st);
            m.launched();
        }
        if (m.er == hipSuccess) {
            hipLaunchKernelGGL(k_damp_carry, dim3(X), dim3(2 * IEQ_RUNS), 0, stream, m.d_st, cg.lanes, cg.nchunks, cg.K, cm);
            m.launched();
        }
    }

    // Fetches what `ga` names into `part` (the scratch grows to fit)
    const auto gather = [&](FlrGather& ga) {
        uint64_t total = 0;
        for (int s = 0; s < FLR_SETS; s++) ga.at[s] = total, total += ga.count[s];
        if (m.er != hipSuccess) return false;
        if (!total) return true;
        m.grow_part((size_t)total);
        if (m.er != hipSuccess) return false;
        part.resize((size_t)total);
        hipLaunchKernelGGL(k_flr_gather, dim3((unsigned)((total + ISH_THREADS - 1) / ISH_THREADS)), dim3(ISH_THREADS), 0, stream, m.d_buf, N, ga, m.d_part);
        m.launched();
        m.fetch(part.data(), m.d_part, sizeof(double) * (size_t)total);
        return m.er == hipSuccess;
    };

    // the band split is the damping's, not Measure::group's band-pass: its own fill and k_flr_band
    const uint32_t groups = flr_groups(q);
    for (uint32_t g = 0; g < groups && m.er == hipSuccess; g++) {
        hipLaunchKernelGGL(k_dec_fill, dim3(grid), dim3(ISH_THREADS), 0, stream, d_x, N, m.d_buf);
        m.launched();
        if (m.er == hipSuccess && g > 0) {
            hipLaunchKernelGGL(k_flr_band, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, m.d_buf, N, pl, (int)g - 1, m.d_st);
            m.launched();
        }
        m.edc();
        if (m.er != hipSuccess) break;

        if (!flr_search(o, N, q, gather, part, rows + 8 * (size_t)g * FLR_SETS)) break;
    }
    m.info(info);
    return m.er;
}

// mc_ir_tail_from_floor for a checked query: fills n_xovers, xover_hz, knee, t60 and level_db of *t
inline void flr_to_tail(const mc_floor_query& q, const double* rows, const uint64_t info[2], uint64_t first, mc_ir_tail* t) {
    const uint32_t X = q.n_xovers;
    const double rate = (double)q.rate;
    t->n_xovers = X;
    for (uint32_t k = 0; k < X; k++) t->xover_hz[k] = q.xover_hz[k];
    for (uint32_t j = 0; j <= X; j++) {
        const uint32_t g = X ? j + 1 : 0;
        const double* lr = rows + 8 * ((size_t)g * FLR_SETS + 2);
        t->knee[j] = FLR_LEFT_ALONE, t->t60[j] = 1, t->level_db[j][0] = t->level_db[j][1] = 0.f;
        if (lr[7] != 0.0 || !std::isfinite(lr[2]) || !(std::floor(lr[2]) < (double)info[1]) || lr[2] < 0.0) continue;
        const double k = std::floor(lr[2]);
        t->knee[j] = first + (uint64_t)k;
        t->t60[j] = (uint64_t)std::max(1.0, std::floor(lr[3] * rate + 0.5));
        for (int c = 0; c < 2; c++) {
            const double* r = rows + 8 * ((size_t)g * FLR_SETS + c);
            const bool own = r[7] == 0.0;
            const double* u = own ? r : lr;  // (the channel has no line of its own: half of what the pair has)
            const double level = 10.0 * std::log10(u[1]) + (-60.0 / (u[3] * rate)) * (k - u[2]) - (own ? 0.0 : 10.0 * std::log10(2.0));
            t->level_db[j][c] = (float)level;
        }
    }
}
