// iriacc.hip.h — the interaural cross-correlation of a loaded impulse response, measured on the device (mc_ir_iacc; ISO 3382-1
// Annex A): IACF over lags of +/- max_lag taps and IACC = max |IACF|, over the early, the late and the whole IR, broadband and in
// up to MC_DECAY_MAX_BANDS band-passed row groups.  No reference equivalent.  include/mcconv.h and DESIGN.md 2.16 hold the
// definition; tests/ir_iacc_np.py states it in float64.
//
// The stored taps are only read.  N, the origin o and a row group's doubles y (double2 [N]: L in x, R in y) are irdecay.hip.h's
// (its Measure: open, group).  Per group the three windows [a, b) = [o, k), [k, N), [o, N) are measured as three ranges of their
// own by one launch (blockIdx.y = window): the whole IR costs as much again as its two parts, and every window's sums are
// folded in an order that depends on its own length alone.
//
// k_iacc_runs is the hot path, (b - a) (2T + 1) double fma per window.  A workgroup owns run r of its window, the IACC_RUN taps
// from a + r IACC_RUN.  It stages y_L of the run (sl) and y_R of the run with T taps before and after it (sr: entry i is tap
// m0 - T + i); every entry whose tap lies outside [a, b) is zero and is never read from memory, so a pair with either tap
// outside the window adds nothing.  Thread t owns the IACC_R = 9 consecutive lags tau = -T + 9 t + c and keeps the nine y_R
// entries that the current tap meets in registers (a window that moves one entry per tap; the loop is unrolled by 9 so that the
// move is a renaming, as k_sweep_corr's).  Per tap a thread reads y_L[m] (one address for the whole workgroup: a broadcast) and
// one new y_R entry, and does 9 fma.  A lane's entries lie 9 doubles apart: 18 t dwords modulo the 64 banks visits the 32 even
// banks once in each 32-lane group of ds_read_b64, so no skew is needed.  256 threads x 9 = 2304 >= 2 MC_IACC_MAX_LAG + 1 lags;
// threads whose first lag is past T idle.  Lags past T inside the last busy thread meet zeros and are not written.  The energies
// ride along: a thread squares the entries it stages that belong to the run and the workgroup adds them in ish_block_reduce's
// fixed order.  A workgroup writes 2T + 3 partials (the lags, E_L, E_R); k_iacc_fold adds the runs' partials in run order, one
// thread per (window, slot).  No atomics; runs, grids and orders depend on a, b and T alone: the same query on the same taps
// gives the same bits.
//
// Scratch (double2 [N], the chunk states, the partials) is allocated by the call and freed before it returns.
#pragma once
#include "irdecay.hip.h"

constexpr int IACC_THREADS = 256;
constexpr int IACC_R = 9;                                          // consecutive lags per thread
constexpr int IACC_RUN = IACC_THREADS * IACC_R;                    // taps per workgroup (2304)
constexpr int IACC_SPAN = IACC_RUN + 2 * MC_IACC_MAX_LAG + 2 * IACC_R;  // y_R entries: the run, T each side, the last thread's spare
                                                                   // lags (< 9) and the sliding window's look-ahead (9)
constexpr int IACC_WINDOWS = 3;
constexpr uint64_t IACC_MAX_WORK = 1ull << 40;   // (1 + n_bands) N (2T + 1)
constexpr uint64_t IACC_MAX_PART = 1ull << 23;   // doubles of partial sums (64 MiB)
static_assert(IACC_RUN >= 2 * MC_IACC_MAX_LAG + 1, "every lag needs a thread");
static_assert(sizeof(double) * (IACC_RUN + IACC_SPAN) <= 64 * 1024, "sl + sr must fit the static LDS limit");

struct IaccPlan {
    uint64_t a[IACC_WINDOWS], b[IACC_WINDOWS];  // the windows' taps [a, b), inside [0, N)
    uint32_t T;                                 // lags -T .. T
    uint32_t maxruns;                           // gridDim.x of k_iacc_runs: the runs of the longest window
};

__host__ __device__ inline uint32_t iacc_runs(uint64_t a, uint64_t b) { return b > a ? (uint32_t)((b - a + IACC_RUN - 1) / IACC_RUN) : 0u; }

// part[((w maxruns + r) (2T + 3)) + s]: s < 2T + 1 the sum of y_L[m] y_R[m + s - T] over the taps m of run r of window w with both
// taps in the window, in ascending m; s = 2T + 1, 2T + 2 the run's sum of y_L^2 and of y_R^2.  grid (maxruns, 3).
__global__ __launch_bounds__(IACC_THREADS) void k_iacc_runs(const double2* __restrict__ y, IaccPlan pl, double* __restrict__ part) {
    __shared__ double sl[IACC_RUN];
    __shared__ double sr[IACC_SPAN];
    __shared__ double red[IACC_THREADS / 64];
    const int t = threadIdx.x, w = blockIdx.y;
    const uint64_t a = pl.a[w], b = pl.b[w];
    const int T = (int)pl.T, lags = 2 * T + 1;
    if (blockIdx.x >= iacc_runs(a, b)) return;  // (the same in every thread of the workgroup)
    const uint64_t m0 = a + (uint64_t)blockIdx.x * IACC_RUN;
    double eL = 0.0, eR = 0.0;
    for (int i = t; i < IACC_RUN; i += IACC_THREADS) {
        const uint64_t m = m0 + (uint64_t)i;
        const double v = m < b ? y[m].x : 0.0;
        sl[i] = v;
        eL += v * v;
    }
    const int used = IACC_RUN + 2 * T + 2 * IACC_R;  // entries the loop below can read, <= IACC_SPAN
    for (int i = t; i < used; i += IACC_THREADS) {
        const int64_t m = (int64_t)m0 - T + i;
        const double v = m >= (int64_t)a && m < (int64_t)b ? y[m].y : 0.0;
        sr[i] = v;
        if (i >= T && i < T + IACC_RUN) eR += v * v;
    }
    __syncthreads();
    double* mine = part + ((uint64_t)w * pl.maxruns + blockIdx.x) * (uint64_t)(lags + 2);
    if (IACC_R * t < lags) {
        double acc[IACC_R], win[IACC_R];  // win[(c + j) % 9] = sr[j + 9 t + c]
        const double* mr = sr + IACC_R * t;
#pragma unroll
        for (int c = 0; c < IACC_R; c++) acc[c] = 0.0, win[c] = mr[c];
        for (int j = 0; j < IACC_RUN; j += IACC_R) {
#pragma unroll
            for (int jj = 0; jj < IACC_R; jj++) {
                const double yl = sl[j + jj];
#pragma unroll
                for (int c = 0; c < IACC_R; c++) acc[c] = fma(yl, win[(c + jj) % IACC_R], acc[c]);
                win[jj] = mr[j + jj + IACC_R];  // entry 9 t + j + jj + 9 <= 2T + IACC_RUN - 1 + 9 < used
            }
        }
#pragma unroll
        for (int c = 0; c < IACC_R; c++)
            if (IACC_R * t + c < lags) mine[IACC_R * t + c] = acc[c];
    }
    const auto add = [](double p, double q) { return p + q; };
    eL = ish_block_reduce(eL, red, add);
    eR = ish_block_reduce(eR, red, add);
    if (t == 0) mine[lags] = eL, mine[lags + 1] = eR;
}

// fin[w (2T + 3) + s] = the sum over window w's runs r, ascending, of part[((w maxruns + r) (2T + 3)) + s]; 0 for an empty window.
// grid (ceil((2T + 3) / IACC_THREADS), 3).
__global__ __launch_bounds__(IACC_THREADS) void k_iacc_fold(const double* __restrict__ part, IaccPlan pl, double* __restrict__ fin) {
    const uint32_t slots = 2 * pl.T + 3, s = blockIdx.x * IACC_THREADS + threadIdx.x, w = blockIdx.y;
    if (s >= slots) return;
    const uint32_t runs = iacc_runs(pl.a[w], pl.b[w]);
    const double* p = part + (uint64_t)w * pl.maxruns * slots + s;
    double sum = 0.0;
    for (uint32_t r = 0; r < runs; r++) sum += p[(uint64_t)r * slots];
    fin[(uint64_t)w * slots + s] = sum;
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a query, in field order, checked without touching an engine or HIP; the message (thread-local) names the
// field.  Null when it is good.
inline const char* iacc_check(const mc_iacc_query* q) {
    static thread_local char msg[160];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_iacc_query)) return "mc_iacc_query struct_size mismatch";
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    if (q->n_bands > MC_DECAY_MAX_BANDS) {
        std::snprintf(msg, sizeof(msg), "n_bands %u above %d", q->n_bands, MC_DECAY_MAX_BANDS);
        return msg;
    }
    if (q->max_lag > MC_IACC_MAX_LAG) {
        std::snprintf(msg, sizeof(msg), "max_lag %u above %d", q->max_lag, MC_IACC_MAX_LAG);
        return msg;
    }
    if (!dec_bands_ok(q->centre_hz, q->n_bands, q->q, q->rate, msg, sizeof(msg)) || !dec_onset_ok(q->onset_db, msg, sizeof(msg))) return msg;
    if (!q->reserved[0] && !q->reserved[1]) return nullptr;
    std::snprintf(msg, sizeof(msg), "reserved {%u, %u} must be 0", q->reserved[0], q->reserved[1]);
    return msg;
}

// doubles of partial sums for N taps analysed: three windows of at most ceil(N / IACC_RUN) runs of 2T + 3 slots
inline uint64_t iacc_part(uint64_t N, uint32_t T) { return (uint64_t)IACC_WINDOWS * iacc_runs(0, N) * (2 * (uint64_t)T + 3); }

// The work bounds for n stored taps; null when they hold
inline const char* iacc_check_work(const mc_iacc_query& q, uint64_t n) {
    static thread_local char msg[200];
    const uint64_t N = dec_span(q.end, n), lags = 2 * (uint64_t)q.max_lag + 1, groups = 1 + (uint64_t)q.n_bands;
    if (N > IACC_MAX_WORK / (groups * lags))
        std::snprintf(msg, sizeof(msg), "max_lag %u puts %llu lags on %llu taps in %llu row groups: above %llu lag products", q.max_lag,
                      (unsigned long long)lags, (unsigned long long)N, (unsigned long long)groups, (unsigned long long)IACC_MAX_WORK);
    else if (iacc_part(N, q.max_lag) > IACC_MAX_PART)
        std::snprintf(msg, sizeof(msg), "max_lag %u needs %llu partial sums on %llu taps, above %llu", q.max_lag,
                      (unsigned long long)iacc_part(N, q.max_lag), (unsigned long long)N, (unsigned long long)IACC_MAX_PART);
    else
        return nullptr;
    return msg;
}

// The eight numbers of a row and its 2T + 1 curve entries (curve may be null) from a window's folded sums fin[2T + 3]
inline void iacc_row(const double* fin, uint32_t T, bool empty, double* row, double* curve) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t lags = 2 * T + 1;
    const double EL = fin[lags], ER = fin[lags + 1];
    row[0] = EL, row[1] = ER;
    for (int k = 2; k < 7; k++) row[k] = nan;
    if (curve)
        for (uint32_t s = 0; s < lags; s++) curve[s] = nan;
    row[7] = 1.0;
    if (empty || !(EL * ER > 0.0)) return;  // (an empty window, a silent channel, or taps that are not numbers)
    const double den = std::sqrt(EL * ER);
    uint32_t at = 0;
    for (uint32_t s = 0; s < lags; s++) {
        const double v = fin[s] / den;
        if (curve) curve[s] = v;
        if (std::fabs(v) > std::fabs(fin[at] / den)) at = s;
    }
    row[2] = std::fabs(fin[at] / den);
    row[3] = (double)((int64_t)at - (int64_t)T);
    row[4] = fin[at] / den;
    row[5] = fin[T] / den;
    row[6] = 10.0 * std::log10(EL / ER);
    row[7] = 0.0;
}

// The whole measurement of the n stored taps d_x for a checked query whose work bounds hold.  rows, curve, info as mc_ir_iacc
// describes them.  Synchronises the stream; leaves nothing allocated.
inline hipError_t iacc_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_iacc_query& q, double* rows, double* curve,
                               uint64_t info[3]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const uint32_t T = q.max_lag, lags = 2 * T + 1, slots = lags + 2;
    std::vector<double> fin((size_t)IACC_WINDOWS * slots);
    m.open(q.onset_db, N, m.cg.lanes, 0, (size_t)iacc_part(N, T), fin.size());
    const uint64_t o = m.o;
    const uint64_t k = std::min<uint64_t>(o + (q.split ? std::min<uint64_t>(q.split, N) : (uint64_t)std::floor(0.08 * (double)q.rate + 0.5)), N);
    IaccPlan pl{};
    pl.a[0] = o, pl.b[0] = k, pl.a[1] = k, pl.b[1] = N, pl.a[2] = o, pl.b[2] = N;
    pl.T = T;
    for (int w = 0; w < IACC_WINDOWS; w++) pl.maxruns = std::max(pl.maxruns, iacc_runs(pl.a[w], pl.b[w]));

    for (uint32_t g = 0; g <= q.n_bands && m.er == hipSuccess; g++) {
        m.group(g ? &q.centre_hz[g - 1] : nullptr, q.q, q.rate);
        if (m.er == hipSuccess && pl.maxruns) {
            hipLaunchKernelGGL(k_iacc_runs, dim3(pl.maxruns, IACC_WINDOWS), dim3(IACC_THREADS), 0, stream, m.d_buf, pl, m.d_part);
            m.launched();
        }
        if (m.er == hipSuccess) {
            hipLaunchKernelGGL(k_iacc_fold, dim3((slots + IACC_THREADS - 1) / IACC_THREADS, IACC_WINDOWS), dim3(IACC_THREADS), 0, stream, m.d_part, pl, m.d_fin);
            m.launched();
        }
        m.fetch(fin.data(), m.d_fin, sizeof(double) * fin.size());
        if (m.er != hipSuccess) break;
        for (int w = 0; w < IACC_WINDOWS; w++) {
            const size_t r = (size_t)g * IACC_WINDOWS + w;
            iacc_row(fin.data() + (size_t)w * slots, T, pl.a[w] >= pl.b[w], rows + 8 * r, curve ? curve + (size_t)lags * r : nullptr);
        }
    }
    m.info(info), info[2] = k;
    return m.er;
}

// mc_ir_tail_width_from_iacc's arithmetic for a finite rho
inline float iacc_width(double rho) { return (float)std::min(std::max(1.0 - rho, 0.0), 1.0); }
