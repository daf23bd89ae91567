// irresponse.hip.h — the frequency response of a loaded impulse response, measured on the device (mc_ir_response): the complex
// response H and the exact group delay at up to MC_RSP_MAX_FREQ frequencies of one's own choosing, over up to MC_RSP_MAX_WIN
// windows of the taps with raised-cosine edges (the slices of a waterfall).  No reference equivalent.  include/mcconv.h and
// DESIGN.md 2.18 hold the definition; tests/ir_response_np.py states it in float64.
//
// The stored taps are only read.  N and the origin o are irdecay.hip.h's (its Measure: open).  There are no row groups and no
// double2 [N] here: a window w is the taps [a, b) (rsp_window), and per window one launch of k_rsp_runs and one of k_rsp_fold reduce
// them into 8 n_freq + 4 sums: per frequency Re and Im of H_L, H_R, D_L, D_R, then E_L, E_R, A_L, A_R.  The windows go one after
// another over the same scratch, as the row groups of the other measurements do.
//
// k_rsp_runs is the hot path, L n_freq (one complex rotation + 8 double fma).  A workgroup owns run r, the RSP_RUN taps from
// a + r RSP_RUN, and a slice of RSP_FT frequencies, one per thread: grid (runs, ceil(n_freq / RSP_FT)).
//   stage    the run's taps go into LDS once, as two double2 per tap: v = (u x_L, u x_R), u the window's weight (the float -> double
//            conversion is exact, u x is rounded once), and d = (m - o) v (m - o is exact, the product is rounded once): 32 bytes
//            per tap, 32 KiB per workgroup, so that four or five workgroups share a CU's 160 KiB;
//   walk     thread t walks the run's taps in order for its frequency F with a rotator z = (c, s) = e^{j theta}; every lane reads the
//            same LDS address per tap, which the LDS serves as one broadcast: no bank conflicts, two 16-byte reads per tap and wave.
//            H += v conj z, D += d conj z: 8 fma;
//   seed     every RSP_STRETCH taps the rotator starts again from theta = 2 pi frac(F k / rate), k = m - o, by irsti.hip.h's exact
//            reduction: x = F k is exact in double for a float F and k < 2^29, n = floor(x / rate), r = fma(-n, rate, x) is exact,
//            sincospi(2 (r / rate)) is the seed;
//   step     z <- z w, w = e^{j 2 pi F / rate}, computed on the host in long double and rounded once (each part within half a unit
//            of the last place: the angle reaches pi here, where a double's 2 pi F / rate alone would be several units off).
// F and w travel in a device buffer (Measure::open's st0, two double2 per frequency): 1024 of them do not fit the kernel's arguments.
// The rotator's error is irsti.hip.h's: with u = 2^-53, after k steps |z_k - e^{j theta_k}| <= (2 + 3.3 k) u, k < RSP_STRETCH, so
// |delta H| <= (n_w + 3.3 RSP_STRETCH + 16) u A over a window of n_w taps with A = sum |u x| (n_w u for the order of the additions, the
// 16 for the roundings of u, v, d, the seed's argument and the restatement's own), and the same for D with A_D = sum (m - o) |u x|.
// A workgroup writes 8 partials per frequency; the workgroups of the first slice reduce the run's E and A as well (ish_block_reduce).
// k_rsp_fold adds the runs' partials in run order, one thread per slot.
//
// Determinism.  No atomics.  Runs are counted from the window's first tap a, seeds from o: run length, grid and every order of
// addition depend on o, a, b and the frequency's own value alone.  The same query on the same taps gives the same bits; a
// frequency's numbers do not depend on its place in hz or on the other frequencies (its walk is thread-local and its fold is its
// own), and a window's numbers do not depend on the other windows.
//
// Scratch (the table, the partials of the largest window, the folded sums) is allocated by the call and freed before it returns.
#pragma once
#include "irdecay.hip.h"

constexpr int RSP_FT = ISH_THREADS;   // frequencies per workgroup, one per thread (ish_block_reduce's workgroup)
constexpr int RSP_RUN = 1024;         // taps per workgroup: 32 bytes of LDS each
constexpr int RSP_STRETCH = 64;       // taps between two seeds of the rotator
constexpr int RSP_SUMS = 8, RSP_TAIL = 4;  // per frequency: Re, Im of H_L, H_R, D_L, D_R; per run: E_L, E_R, A_L, A_R
static_assert(RSP_RUN % RSP_STRETCH == 0 && RSP_RUN % RSP_FT == 0, "a run is whole stretches and whole staging rounds");

struct RspPlan {
    uint64_t o, a, L;          // the origin; the window's first tap and its length
    uint32_t rise, fall;       // clamped: rise <= L, fall <= L - rise
    uint32_t n_freq, runs;     // runs = gridDim.x of k_rsp_runs
    double rate;
};

inline uint32_t rsp_runs(uint64_t L) { return (uint32_t)((L + RSP_RUN - 1) / RSP_RUN); }
__host__ __device__ inline uint32_t rsp_slots(uint32_t n_freq) { return RSP_SUMS * n_freq + RSP_TAIL; }

// the weight of tap k of a window of L taps (step 2 of the definition; irshape.hip.h's fade at both ends)
__device__ inline double rsp_weight(uint64_t k, const RspPlan& pl) {
    if (k < pl.rise) return 0.5 * (1.0 - cos(M_PI * ((double)k + 1.0) / ((double)pl.rise + 1.0)));
    const uint64_t f0 = pl.L - pl.fall;
    if (k >= f0) return 0.5 * (1.0 + cos(M_PI * ((double)(k - f0) + 1.0) / ((double)pl.fall + 1.0)));
    return 1.0;
}

// part[r slots + j n_freq + f], j < 8: run r's sums at frequency f (tab[2 f].x = F in Hz, tab[2 f + 1] = w) of v c, -v s over
// {v_L, v_R, d_L, d_R} with (c, s) = e^{j theta}, theta = 2 pi F (m - o) / rate; part[r slots + 8 n_freq ..] = the run's E_L, E_R,
// A_L, A_R.  grid (runs, ceil(n_freq / RSP_FT)); slots = rsp_slots(n_freq).
__global__ __launch_bounds__(RSP_FT) void k_rsp_runs(const float2* __restrict__ x, const double2* __restrict__ tab, RspPlan pl,
                                                     double* __restrict__ part) {
    __shared__ double2 sv[RSP_RUN], sd[RSP_RUN];
    __shared__ double red[ISH_WAVES];
    const int t = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * RSP_RUN;  // (counted from a; < L, since runs = ceil(L / RSP_RUN))
    const uint64_t left = pl.L - k0;
    const int cnt = left < (uint64_t)RSP_RUN ? (int)left : RSP_RUN;
    double* mine = part + (uint64_t)blockIdx.x * rsp_slots(pl.n_freq);

    double e[RSP_TAIL] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < cnt; i += RSP_FT) {
        const uint64_t k = k0 + (uint64_t)i;
        const float2 tap = x[pl.a + k];  // (a + k < a + L = b <= N)
        const double u = rsp_weight(k, pl), d = (double)(pl.a - pl.o + k);
        const double2 v = make_double2(u * (double)tap.x, u * (double)tap.y);
        sv[i] = v, sd[i] = make_double2(d * v.x, d * v.y);
        e[0] += v.x * v.x, e[1] += v.y * v.y, e[2] += fabs(v.x), e[3] += fabs(v.y);
    }
    if (blockIdx.y == 0) {  // (the same for the whole workgroup)
        for (int j = 0; j < RSP_TAIL; j++) {
            const double r = ish_block_reduce(e[j], red, [](double p, double q) { return p + q; });
            if (t == 0) mine[RSP_SUMS * pl.n_freq + j] = r;
        }
    }
    __syncthreads();

    const uint32_t f = blockIdx.y * RSP_FT + (uint32_t)t;
    if (f >= pl.n_freq) return;
    const double F = tab[2 * f].x, wc = tab[2 * f + 1].x, ws = tab[2 * f + 1].y;
    double hlr = 0.0, hli = 0.0, hrr = 0.0, hri = 0.0, dlr = 0.0, dli = 0.0, drr = 0.0, dri = 0.0;
    for (int i0 = 0; i0 < cnt; i0 += RSP_STRETCH) {
        const double xk = F * (double)(pl.a - pl.o + k0 + (uint64_t)i0), r = fma(-floor(xk / pl.rate), pl.rate, xk);
        double c, s;
        sincospi(2.0 * (r / pl.rate), &s, &c);
        const int i1 = min(cnt, i0 + RSP_STRETCH);
#pragma unroll 8
        for (int i = i0; i < i1; i++) {
            const double2 v = sv[i], d = sd[i];
            hlr = fma(v.x, c, hlr), hli = fma(-v.x, s, hli);
            hrr = fma(v.y, c, hrr), hri = fma(-v.y, s, hri);
            dlr = fma(d.x, c, dlr), dli = fma(-d.x, s, dli);
            drr = fma(d.y, c, drr), dri = fma(-d.y, s, dri);
            const double cn = c * wc - s * ws;
            s = s * wc + c * ws, c = cn;
        }
    }
    const uint32_t nf = pl.n_freq;
    mine[f] = hlr, mine[nf + f] = hli, mine[2 * nf + f] = hrr, mine[3 * nf + f] = hri;
    mine[4 * nf + f] = dlr, mine[5 * nf + f] = dli, mine[6 * nf + f] = drr, mine[7 * nf + f] = dri;
}

// fin[s] = the sum over the runs r, ascending, of part[r slots + s].  grid (ceil(slots / RSP_FT)).
__global__ __launch_bounds__(RSP_FT) void k_rsp_fold(const double* __restrict__ part, RspPlan pl, double* __restrict__ fin) {
    const uint32_t slots = rsp_slots(pl.n_freq), s = blockIdx.x * RSP_FT + threadIdx.x;
    if (s >= slots) return;
    double sum = 0.0;
    for (uint32_t r = 0; r < pl.runs; r++) sum += part[(uint64_t)r * slots + s];
    fin[s] = sum;
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a query in struct order, then every hz[f], checked without touching an engine or HIP; the message
// (thread-local) names the field.  Null when all is good.  (A null hz is the caller's to name: the pointers come after.)
inline const char* rsp_check(const mc_response_query* q, const float* hz) {
    static thread_local char msg[160];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_response_query)) return "mc_response_query struct_size mismatch";
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    if (q->n_freq < 1 || q->n_freq > MC_RSP_MAX_FREQ) {
        std::snprintf(msg, sizeof(msg), "n_freq %u outside [1, %d]", q->n_freq, MC_RSP_MAX_FREQ);
        return msg;
    }
    if (q->n_win < 1 || q->n_win > MC_RSP_MAX_WIN) {
        std::snprintf(msg, sizeof(msg), "n_win %u outside [1, %d]", q->n_win, MC_RSP_MAX_WIN);
        return msg;
    }
    if (q->flags) {
        std::snprintf(msg, sizeof(msg), "unknown bit in flags 0x%x", q->flags);
        return msg;
    }
    if (!dec_onset_ok(q->onset_db, msg, sizeof(msg))) return msg;
    if (q->reserved[0] || q->reserved[1]) {
        std::snprintf(msg, sizeof(msg), "reserved {%u, %u} must be 0", q->reserved[0], q->reserved[1]);
        return msg;
    }
    if (!hz) return nullptr;
    const double top = 0.5 * (double)q->rate;
    for (uint32_t f = 0; f < q->n_freq; f++)
        if (const double v = (double)hz[f]; !(v >= 0.0 && v <= top)) {  // (NaN compares false)
            std::snprintf(msg, sizeof(msg), "hz[%u] %g outside [0, %g]", f, v, top);
            return msg;
        }
    return nullptr;
}

// step 2 of the definition: window w of the taps [o, N) as a plan (a, L, rise, fall)
inline void rsp_window(const mc_response_window& w, uint64_t o, uint64_t N, RspPlan* pl) {
    const uint64_t a = w.first < N - o ? o + w.first : N;  // min(o + first, N) without the sum's overflow (o <= N)
    const uint64_t b = w.count && w.count < N - a ? a + w.count : N;
    pl->a = a, pl->L = b - a;
    pl->rise = (uint32_t)std::min<uint64_t>(w.rise, pl->L);
    pl->fall = (uint32_t)std::min<uint64_t>(w.fall, pl->L - pl->rise);
}

// Steps 3 to 5 for one window from its folded sums fin [rsp_slots(n_freq)] (all zero for an empty window): the two channels'
// rows (4 numbers each) and resp entries (3 n_freq each)
inline void rsp_rows(const double* fin, uint32_t nf, bool empty, double* rows, double* resp) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < 2; c++) {
        const double E = fin[RSP_SUMS * nf + c], A = fin[RSP_SUMS * nf + 2 + c];
        const bool bad = empty || A == 0.0 || !std::isfinite(A);
        double* row = rows + 4 * c;
        row[0] = E, row[1] = A, row[2] = bad ? 1.0 : 0.0, row[3] = 0.0;
        for (uint32_t f = 0; f < nf; f++) {
            double* out = resp + ((size_t)c * nf + f) * 3;
            if (bad) {
                out[0] = 0.0, out[1] = 0.0, out[2] = nan;
                continue;
            }
            const double hr = fin[(2 * c) * nf + f], hi = fin[(2 * c + 1) * nf + f];
            const double dr = fin[(4 + 2 * c) * nf + f], di = fin[(5 + 2 * c) * nf + f];
            const double p = hr * hr + hi * hi;
            out[0] = hr, out[1] = hi, out[2] = p != 0.0 && std::isfinite(p) ? (dr * hr + di * hi) / p : nan;
        }
    }
}

// The whole measurement of the n stored taps d_x for a checked query.  resp, rows, spans, info as mc_ir_response describes them;
// win null: the whole span.  Synchronises the stream; leaves nothing allocated.
inline hipError_t rsp_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_response_query& q, const float* hz,
                              const mc_response_window* win, double* resp, double* rows, uint64_t* spans, uint64_t info[2]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const uint32_t nf = q.n_freq, slots = rsp_slots(nf);
    std::vector<double2> tab((size_t)2 * nf);
    for (uint32_t f = 0; f < nf; f++) {
        const long double w = 2.0L * 3.14159265358979323846264338327950288L * (long double)hz[f] / (long double)q.rate;
        tab[2 * f] = make_double2((double)hz[f], 0.0);
        tab[2 * f + 1] = make_double2((double)cosl(w), (double)sinl(w));
    }
    std::vector<double> fin(slots);
    m.open(q.onset_db, 0, tab.size(), 0, 0, slots, tab.data());
    const uint64_t o = m.o;
    const mc_response_window whole{0, 0, 0, 0};
    std::vector<RspPlan> plans(q.n_win);
    uint32_t most = 0;
    for (uint32_t w = 0; w < q.n_win; w++) {
        RspPlan& pl = plans[w];
        pl.o = o, pl.n_freq = nf, pl.rate = (double)q.rate;
        rsp_window(win ? win[w] : whole, o, N, &pl);
        pl.runs = rsp_runs(pl.L);
        most = std::max(most, pl.runs);
    }
    m.grow_part((size_t)most * slots);  // (the origin's walks are done with d_part: the stream ran dry in open)

    for (uint32_t w = 0; w < q.n_win && m.er == hipSuccess; w++) {
        const RspPlan& pl = plans[w];
        if (pl.runs) {
            hipLaunchKernelGGL(k_rsp_runs, dim3(pl.runs, (nf + RSP_FT - 1) / RSP_FT), dim3(RSP_FT), 0, stream, d_x, m.d_st, pl, m.d_part);
            m.launched();
            if (m.er == hipSuccess) {
                hipLaunchKernelGGL(k_rsp_fold, dim3((slots + RSP_FT - 1) / RSP_FT), dim3(RSP_FT), 0, stream, m.d_part, pl, m.d_fin);
                m.launched();
            }
            m.fetch(fin.data(), m.d_fin, sizeof(double) * slots);
            if (m.er != hipSuccess) break;
        } else
            std::fill(fin.begin(), fin.end(), 0.0);
        rsp_rows(fin.data(), nf, pl.L == 0, rows + (size_t)w * 8, resp + (size_t)w * 2 * nf * 3);
        spans[2 * w] = pl.a, spans[2 * w + 1] = pl.a + pl.L;
    }
    if (m.er == hipSuccess) m.er = hipStreamSynchronize(stream);  // (the table's copy, when every window was empty and onset_db is 0)
    m.info(info);
    return m.er;
}

// mc_response_grid's arithmetic: hz[i] = (float)(lo 2^(i / per_octave)) while that double is <= hi.  The count, or -1 when it
// exceeds cap.
inline int rsp_grid(double lo, double hi, uint32_t per_octave, float* hz, uint32_t cap) {
    uint32_t i = 0;
    for (;; i++) {
        const double v = lo * std::exp2((double)i / (double)per_octave);
        if (!(v <= hi)) break;
        if (i >= cap) return -1;
        hz[i] = (float)v;
    }
    return (int)i;
}

// mc_response_smooth's arithmetic: out[f] = the mean of power[g], ascending g, over hz[g] in [hz[f] 2^(-octaves / 2), hz[f] 2^(octaves / 2)]
inline void rsp_smooth(const float* hz, const double* power, uint32_t n, double octaves, double* out) {
    const double down = std::exp2(-0.5 * octaves), up = std::exp2(0.5 * octaves);
    uint32_t g0 = 0, g1 = 0;  // hz ascends: both edges only move up
    for (uint32_t f = 0; f < n; f++) {
        const double c = (double)hz[f], lo = c * down, hi = c * up;
        if (octaves == 0.0) {
            out[f] = power[f];
            continue;
        }
        while (g0 < n && (double)hz[g0] < lo) g0++;
        if (g1 < g0) g1 = g0;
        while (g1 < n && (double)hz[g1] <= hi) g1++;
        double sum = 0.0;
        for (uint32_t g = g0; g < g1; g++) sum += power[g];
        out[f] = sum / (double)(g1 - g0);
    }
}
