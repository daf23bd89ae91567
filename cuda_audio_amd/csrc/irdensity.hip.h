// irdensity.hip.h — the echo density of a loaded impulse response, measured on the device (mc_ir_density): Abel and Huang's
// normalised echo density in a sliding raised-cosine window, and the mixing time it gives, for L, R and L + R.  No reference
// equivalent.  include/mcconv.h and DESIGN.md 2.15 hold the definition; tests/ir_density_np.py states it in float64.
// mc_ir_tail_move_knee, host arithmetic, moves a tail band's knee to such a mixing time (den_move_knee).
//
// The stored taps x [n] are only read.  With N = end ? min(end, n) : n and the origin o of irdecay.hip.h's Measure, centre i sits at
// t_i = o + i hop, i < I = floor((N - 1 - o) / hop) + 1, and its window holds the taps t_i + k, k = -H .. H, that lie in [0, N).
//   table   the host fills tab[k + H] = {h_k, g_k}: the window's weight and the decay compensation exp2(k 3 log2(10) / decay_t60)
//           (1 with decay_t60 = 0).  Both depend on k alone, so no centre ever evaluates a cosine or an exp2;
//   window  k_den_window: a workgroup of DEN_WAVES wavefronts owns a run of C consecutive centres, one wavefront per centre at
//           a time (wave w takes the run's centres w, w + DEN_WAVES, ...).
//             staged  (STAGED = true) the run's taps [t_first - H, t_last + H], cut to [0, N), are copied to LDS once, (C - 1) hop
//                     + 2 H + 1 float2 at most.  C = den_run(H, hop) is the largest count up to DEN_RUN whose span fits
//                     DEN_LDS_TAPS; the launch asks for exactly the bytes the span needs, so narrow windows leave the LDS to
//                     more workgroups.  Lane l reads LDS entry base + l + 64 j: consecutive 8-byte entries, no bank is asked twice.
//             global  (STAGED = false) a window wider than DEN_LDS_TAPS, or windows that do not overlap (hop > 2 H, where
//                     staging would copy the gaps between them), are read from global memory by the same code, C = DEN_WAVES.
//           Pass one: lane l adds h, h vL^2, h vR^2 over k = -H + l + 64 j in ascending j (v = (double) x g); the wavefront tree
//           below adds the 64 partials; sigma_L, sigma_R, sigma_LR follow.  Pass two: the same walk adds h where |v| > sigma, four
//           sums (L and R against their own sigma, L and R against sigma_LR); the tree again; lane 0 writes the centre's four
//           doubles: eta_L, eta_R, eta_LR and the silent flags (bit s set: sigma_s = 0).
//   rows    the host walks the profile in index order (den_rows).
//
// Reduction order.  A lane's partial is one chain over its own taps, k ascending; tap k of the window belongs to lane
// (k + H) mod 64 whatever the centre, and a tap outside [0, N) adds nothing.  The partials are added by a butterfly, v +=
// shfl_xor(v, 32), 16, .. 1: addition commutes, so every lane holds the same bits and sigma needs no broadcast.  The order
// depends on H alone.  No atomics, one writer per output.
//
// Determinism.  The grid and the runs depend on (N, o, hop, H) alone; the same query on the same taps gives the same bits.
//
// Scratch (the table, double [4 I]) is allocated by the call and freed before it returns.
#pragma once
#include <algorithm>
#include <limits>
#include <vector>

#include "irdecay.hip.h"

constexpr int DEN_THREADS = 256, DEN_WAVES = DEN_THREADS / 64;
constexpr uint32_t DEN_LDS_TAPS = 6144;   // float2 entries a workgroup may stage: 48 KiB, three workgroups on a CU's 160 KiB
constexpr uint32_t DEN_RUN = 16;          // centres of a staged run, at most (four per wavefront)
constexpr uint32_t DEN_MIN_HALF = 4, DEN_MAX_HALF = 16384, DEN_MAX_HOP = 1u << 20;
constexpr uint64_t DEN_MAX_CENTRES = 1ull << 22, DEN_MAX_WORK = 1ull << 34;
constexpr double DEN_MAX_OCTAVES = 256.0;                  // |log2 g| at the window's edge, at most
constexpr double DEN_GAUSS_SHARE = 0.31731050786291415;    // erfc(1 / sqrt 2)
constexpr int DEN_OUT = 4;                                 // doubles per centre: eta L, R, L + R, silent flags

// what the kernel needs of a resolved query
struct DenPlan {
    uint64_t N, o, I;
    uint32_t H, hop, C;   // C: centres per workgroup
};

// the wavefront's sum in every lane (the file's head)
__device__ inline double den_wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// out[DEN_OUT i ..] of every centre i < pl.I.  gridDim.x = ceil(I / C).  STAGED: dynamic LDS of float2 [span of a run], see
// den_lds_bytes.
template <bool STAGED>
__global__ __launch_bounds__(DEN_THREADS) void k_den_window(const float2* __restrict__ x, DenPlan pl, const double2* __restrict__ tab,
                                                            double* __restrict__ out) {
    extern __shared__ float2 den_taps[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t H = (int64_t)pl.H, N = (int64_t)pl.N;
    const uint64_t i0 = (uint64_t)blockIdx.x * pl.C, i1 = i0 + pl.C < pl.I ? i0 + pl.C : pl.I;
    // the run's taps: [lo, hi]
    const int64_t below = (int64_t)(pl.o + i0 * pl.hop) - H, above = (int64_t)(pl.o + (i1 - 1) * pl.hop) + H;
    const int64_t lo = below > 0 ? below : 0;
    if (STAGED) {
        const int64_t hi = above < N - 1 ? above : N - 1;
        for (int64_t m = lo + threadIdx.x; m <= hi; m += DEN_THREADS) den_taps[m - lo] = x[m];
        __syncthreads();
    }
    const auto tap = [&](int64_t tau) { return STAGED ? den_taps[tau - lo] : x[tau]; };
    const int width = 2 * (int)pl.H + 1;
    for (uint64_t i = i0 + wave; i < i1; i += DEN_WAVES) {
        const int64_t first = (int64_t)(pl.o + i * pl.hop) - H;  // the tap of k = -H
        double ws = 0.0, sL = 0.0, sR = 0.0;
        for (int kk = lane; kk < width; kk += 64) {
            const int64_t tau = first + kk;
            if (tau < 0 || tau >= N) continue;
            const double2 hg = tab[kk];
            const float2 v = tap(tau);
            const double vL = (double)v.x * hg.y, vR = (double)v.y * hg.y;
            ws += hg.x;
            sL += hg.x * (vL * vL);
            sR += hg.x * (vR * vR);
        }
        ws = den_wave_sum(ws), sL = den_wave_sum(sL), sR = den_wave_sum(sR);
        const double gL = sqrt(sL / ws), gR = sqrt(sR / ws), gLR = sqrt((sL + sR) / (2.0 * ws));
        double aL = 0.0, aR = 0.0, bL = 0.0, bR = 0.0;
        for (int kk = lane; kk < width; kk += 64) {
            const int64_t tau = first + kk;
            if (tau < 0 || tau >= N) continue;
            const double2 hg = tab[kk];
            const float2 v = tap(tau);
            const double vL = fabs((double)v.x * hg.y), vR = fabs((double)v.y * hg.y);
            if (vL > gL) aL += hg.x;
            if (vR > gR) aR += hg.x;
            if (vL > gLR) bL += hg.x;
            if (vR > gLR) bR += hg.x;
        }
        aL = den_wave_sum(aL), aR = den_wave_sum(aR), bL = den_wave_sum(bL), bR = den_wave_sum(bR);
        if (lane == 0) {
            const double full = ws * DEN_GAUSS_SHARE;
            double* mine = out + (uint64_t)DEN_OUT * i;
            mine[0] = aL / full;
            mine[1] = aR / full;
            mine[2] = ((bL + bR) / 2.0) / full;
            mine[3] = (double)((gL == 0.0 ? 1 : 0) | (gR == 0.0 ? 2 : 0) | (gLR == 0.0 ? 4 : 0));
        }
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
inline uint32_t den_half(const mc_density_query& q) { return q.half ? q.half : (uint32_t)std::floor(0.01 * (double)q.rate + 0.5); }
inline uint32_t den_hop(const mc_density_query& q) { return q.hop ? q.hop : std::max<uint32_t>(1, den_half(q) / 4); }
// windows that overlap and fit the budget are staged
inline bool den_staged(uint32_t H, uint32_t hop) { return 2 * H + 1 <= DEN_LDS_TAPS && hop <= 2 * H; }
// centres per workgroup
inline uint32_t den_run(uint32_t H, uint32_t hop) {
    return den_staged(H, hop) ? 1 + std::min<uint32_t>(DEN_RUN - 1, (DEN_LDS_TAPS - (2 * H + 1)) / hop) : (uint32_t)DEN_WAVES;
}
inline size_t den_lds_bytes(uint32_t H, uint32_t hop) {
    return den_staged(H, hop) ? sizeof(float2) * ((size_t)(den_run(H, hop) - 1) * hop + 2 * (size_t)H + 1) : 0;
}

// Every field of a query, in field order, checked without touching an engine or HIP; the message (thread-local) names the
// field.  Null when it is good.
inline const char* den_check(const mc_density_query* q) {
    static thread_local char msg[200];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_density_query)) return "mc_density_query struct_size mismatch";
    msg[0] = 0;
    const double th = (double)q->threshold;
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    if (q->half && (q->half < DEN_MIN_HALF || q->half > DEN_MAX_HALF))
        std::snprintf(msg, sizeof(msg), "half %u is neither 0 nor in [%u, %u]", q->half, DEN_MIN_HALF, DEN_MAX_HALF);
    else if (q->hop > DEN_MAX_HOP)
        std::snprintf(msg, sizeof(msg), "hop %u above %u", q->hop, DEN_MAX_HOP);
    else if (!dec_onset_ok(q->onset_db, msg, sizeof(msg)))
        return msg;
    else if (!(std::isfinite(th) && th > 0.0 && th <= 2.0))
        std::snprintf(msg, sizeof(msg), "threshold %g outside (0, 2]", th);
    else if (q->decay_t60 && (double)den_half(*q) * ISH_DECAY_K / (double)q->decay_t60 > DEN_MAX_OCTAVES)
        std::snprintf(msg, sizeof(msg), "decay_t60 %llu undoes more than %g octaves across half a window of %u taps",
                      (unsigned long long)q->decay_t60, DEN_MAX_OCTAVES, den_half(*q));
    else if (q->reserved[0] || q->reserved[1])
        std::snprintf(msg, sizeof(msg), "reserved {%u, %u} must be 0", q->reserved[0], q->reserved[1]);
    return msg[0] ? msg : nullptr;
}

// The work bounds for n stored taps, with the origin taken as 0; null when they hold
inline const char* den_check_work(const mc_density_query& q, uint64_t n) {
    static thread_local char msg[200];
    const uint64_t N = dec_span(q.end, n), hop = den_hop(q), width = 2 * (uint64_t)den_half(q) + 1;
    const uint64_t imax = (N - 1) / hop + 1;
    if (imax > DEN_MAX_CENTRES)
        std::snprintf(msg, sizeof(msg), "hop %llu puts %llu windows on %llu taps, above %llu", (unsigned long long)hop, (unsigned long long)imax,
                      (unsigned long long)N, (unsigned long long)DEN_MAX_CENTRES);
    else if (imax * width > DEN_MAX_WORK)
        std::snprintf(msg, sizeof(msg), "hop %llu puts %llu windows of %llu taps on %llu taps: above %llu weighted taps", (unsigned long long)hop,
                      (unsigned long long)imax, (unsigned long long)width, (unsigned long long)N, (unsigned long long)DEN_MAX_WORK);
    else
        return nullptr;
    return msg;
}

// tab[k + H] = {h_k, g_k}, k = -H .. H
inline std::vector<double2> den_table(uint32_t H, uint64_t decay_t60) {
    std::vector<double2> tab(2 * (size_t)H + 1);
    for (int64_t k = -(int64_t)H; k <= (int64_t)H; k++) {
        const double h = (1.0 + std::cos(M_PI * (double)k / ((double)H + 1.0))) / 2.0;
        const double g = decay_t60 ? std::exp2((double)k * ISH_DECAY_K / (double)decay_t60) : 1.0;
        tab[(size_t)(k + (int64_t)H)] = make_double2(h, g);
    }
    return tab;
}

// The eight numbers of set s from the I centres' outputs (out: DEN_OUT doubles per centre), in index order
inline void den_rows(const double* out, uint64_t I, int s, uint64_t o, uint32_t hop, uint32_t rate, double threshold, double* row) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t mix = I, top = 0, silent = 0;
    for (uint64_t i = 0; i < I; i++) {
        const double eta = out[DEN_OUT * i + s];
        if (mix == I && eta >= threshold) mix = i;
        if (eta > out[DEN_OUT * top + s]) top = i;
        silent += ((uint32_t)out[DEN_OUT * i + 3] >> s) & 1u;
    }
    double after = 0.0;
    for (uint64_t i = mix; i < I; i++) after += out[DEN_OUT * i + s];
    const bool found = mix < I;
    row[0] = found ? (double)(o + mix * hop) : nan;
    row[1] = found ? (double)(mix * hop) / (double)rate : nan;
    row[2] = out[s];
    row[3] = out[DEN_OUT * top + s];
    row[4] = (double)(o + top * hop);
    row[5] = found ? after / (double)(I - mix) : nan;
    row[6] = (double)silent;
    row[7] = found ? 0.0 : 1.0;
}

// The whole measurement of the n stored taps d_x for a checked query whose work bounds hold.  rows, profile, info as
// mc_ir_density describes them.  Synchronises the stream; leaves nothing allocated.
inline hipError_t den_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_density_query& q, double* rows, double* profile,
                              uint64_t info[3]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const uint32_t H = den_half(q), hop = den_hop(q);
    const uint64_t imax = (N - 1) / hop + 1;
    const std::vector<double2> tab = den_table(H, q.decay_t60);
    // no row groups: the table rides in the states' place, the centres' outputs in the folded sums'
    m.open(q.onset_db, 0, tab.size(), 0, 0, DEN_OUT * (size_t)imax, tab.data());
    double2* const d_tab = m.d_st;
    double* const d_out = m.d_fin;
    const uint64_t o = m.o;

    DenPlan pl{};
    pl.N = N, pl.o = o, pl.I = (N - 1 - o) / hop + 1, pl.H = H, pl.hop = hop, pl.C = den_run(H, hop);
    std::vector<double> out(DEN_OUT * (size_t)pl.I);
    if (m.er == hipSuccess) {
        const unsigned grid = (unsigned)((pl.I + pl.C - 1) / pl.C);
        if (den_staged(H, hop))
            hipLaunchKernelGGL(k_den_window<true>, dim3(grid), dim3(DEN_THREADS), den_lds_bytes(H, hop), stream, d_x, pl, d_tab, d_out);
        else
            hipLaunchKernelGGL(k_den_window<false>, dim3(grid), dim3(DEN_THREADS), 0, stream, d_x, pl, d_tab, d_out);
        m.launched();
    }
    m.fetch(out.data(), d_out, sizeof(double) * out.size());
    if (m.er != hipSuccess) {
        (void)hipStreamSynchronize(stream);  // (the table's upload reads `tab`: wait for it on every path)
        return m.er;
    }
    for (int s = 0; s < DEC_SETS; s++) den_rows(out.data(), pl.I, s, o, hop, q.rate, (double)q.threshold, rows + 8 * s);
    if (profile)
        for (uint64_t i = 0; i < pl.I; i++)
            for (int s = 0; s < DEC_SETS; s++) profile[3 * i + s] = out[DEN_OUT * i + s];
    m.info(info), info[2] = pl.I;
    return hipSuccess;
}

// mc_ir_tail_move_knee for checked arguments: the band's knee goes to `frame`, its two levels slide along its own line
inline void den_move_knee(mc_ir_tail* t, uint32_t band, uint64_t frame) {
    const double slide = 60.0 * ((double)t->knee[band] - (double)frame) / (double)t->t60[band];
    for (int c = 0; c < 2; c++) t->level_db[band][c] = (float)((double)t->level_db[band][c] + slide);
    t->knee[band] = frame;
}
