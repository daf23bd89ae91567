// irsti.hip.h — the speech transmission index of a loaded impulse response, measured on the device (mc_ir_sti; the indirect
// method of IEC 60268-16 by Schroeder's relation): the modulation transfer function of the squared response at up to
// MC_STI_MAX_MOD modulation frequencies, broadband and in up to MC_STI_MAX_BANDS band-passed row groups, and the index the
// band weights fold it into.  No reference equivalent.  include/mcconv.h and DESIGN.md 2.17 hold the definition;
// tests/ir_sti_np.py states it in float64.
//
// The stored taps are only read.  N, the origin o and a row group's doubles y (double2 [N]: L in x, R in y) are irdecay.hip.h's
// (its Measure: open, group).  Per group one launch of k_sti_runs reduces the taps [o, N) into 4 n_mod + 2 sums: C_L, S_L, C_R, S_R
// per modulation frequency, then E_L and E_R.  The third channel set (L + R) is the sum of the other two's folded sums, added on
// the host: it is not walked.
//
// k_sti_runs is the hot path, (N - o) 4 n_mod double fma plus the trigonometry.  A workgroup owns run r, the STI_RUN taps from
// o + r STI_RUN; thread t owns the STI_STRETCH = 16 consecutive taps from k0 = r STI_RUN + 16 t (counted from o) and keeps their
// squares in registers.  Per modulation frequency F it walks its stretch with a rotator z = (c, s) = e^{j theta}:
//   seed     theta = 2 pi frac(F k0 / rate).  x = F k0 is exact in double for k0 < 2^29 (F is a float: 24 bits), n = floor(x / rate),
//            r = fma(-n, rate, x) is exact too (a multiple of F's last bit below 2 rate: 47 bits at most), so r / rate is the
//            reduced phase in cycles with one rounding, and sincospi(2 r / rate) is the seed, a unit off in the last place at
//            most.  (Past 2^29 taps, three hours at 48 kHz, x carries one rounding more: 2^-53 of the cycles run so far.);
//   step     z <- z w, w = e^{j 2 pi F / rate} in double from the host: a complex multiply.
// The rotator's error: with u = 2^-53, the seed is within 2u of the unit circle's point, w within u of its own, and a complex
// multiply in double adds at most sqrt(5) u |z w| (Brent, Percival and Zimmermann 2007), so after k steps
//   |z_k - e^{j theta_k}| <= (2 + (1 + sqrt 5) k) u < (2 + 3.3 k) u,
// about k 2^-53 times a small constant.  A stretch takes k <= 15 steps: 52 u = 5.8e-15, and since every tap's square is
// non-negative that is also the bound on |delta C| / E and |delta S| / E, 8.2e-15 on m: four orders under the 1e-10 the
// broadband figures are held to, which the sums' own n 2^-53 fills.  A stretch could be a hundred times as long before the
// rotator mattered; 16 is chosen for the registers (32 squares) and so that 2^20 taps make 256 workgroups.
// The loop over the frequencies is the outer one and its four sums are reduced at once (ish_block_reduce, wave64 xor
// butterflies then the four waves in order), so nothing is indexed by f in registers and nothing spills.  A workgroup writes
// 4 n_mod + 2 partials; k_sti_fold adds the runs' partials in run order, one thread per slot.  No atomics; the run length, the
// grid and every order of addition depend on o, N and n_mod alone: the same query on the same taps gives the same bits.
//
// Scratch (double2 [N], the chunk states, the partials) is allocated by the call and freed before it returns.
#pragma once
#include "irdecay.hip.h"

constexpr int STI_THREADS = ISH_THREADS;             // (ish_block_reduce's workgroup)
constexpr int STI_STRETCH = 16;                      // consecutive taps per thread: the rotator is reseeded at each one's start
constexpr int STI_RUN = STI_THREADS * STI_STRETCH;   // taps per workgroup (4096)
constexpr int STI_SETS = 3;
constexpr double STI_MIN_MOD_HZ = 0.1, STI_MAX_MOD_HZ = 50.0, STI_MIN_SNR_DB = -60.0, STI_MAX_SNR_DB = 120.0;

struct StiPlan {
    uint64_t o, N;                  // the taps [o, N)
    uint32_t n_mod, runs;           // runs = gridDim.x of k_sti_runs
    double rate;
    double F[MC_STI_MAX_MOD];       // the modulation frequencies in Hz
    double wc[MC_STI_MAX_MOD], ws[MC_STI_MAX_MOD];  // cos and sin of 2 pi F / rate
};

__host__ __device__ inline uint32_t sti_runs(uint64_t o, uint64_t N) { return N > o ? (uint32_t)((N - o + STI_RUN - 1) / STI_RUN) : 0u; }
inline uint32_t sti_slots(uint32_t n_mod) { return 4 * n_mod + 2; }

// part[r (4 n_mod + 2) + 4 f + {0, 1, 2, 3}] = run r's sums of y_L^2 cos, y_L^2 sin, y_R^2 cos, y_R^2 sin of theta = 2 pi F_f (m - o) / rate
// over its taps m < N; the last two slots its sums of y_L^2 and y_R^2.  grid (runs).
__global__ __launch_bounds__(STI_THREADS) void k_sti_runs(const double2* __restrict__ y, StiPlan pl, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const int t = threadIdx.x;
    const uint64_t k0 = (uint64_t)blockIdx.x * STI_RUN + (uint64_t)t * STI_STRETCH, m0 = pl.o + k0;
    double eL[STI_STRETCH], eR[STI_STRETCH], EL = 0.0, ER = 0.0;
#pragma unroll
    for (int j = 0; j < STI_STRETCH; j++) {
        const uint64_t m = m0 + (uint64_t)j;
        const double2 v = m < pl.N ? y[m] : double2{0.0, 0.0};  // (a tap past N is never read and adds nothing)
        eL[j] = v.x * v.x, eR[j] = v.y * v.y;
        EL += eL[j], ER += eR[j];
    }
    const auto add = [](double p, double q) { return p + q; };
    double* mine = part + (uint64_t)blockIdx.x * (4 * pl.n_mod + 2);
    for (uint32_t f = 0; f < pl.n_mod; f++) {
        const double wc = pl.wc[f], ws = pl.ws[f];
        const double x = pl.F[f] * (double)k0, r = fma(-floor(x / pl.rate), pl.rate, x);
        double c, s;
        sincospi(2.0 * (r / pl.rate), &s, &c);
        double cl = 0.0, sl = 0.0, cr = 0.0, sr = 0.0;
#pragma unroll
        for (int j = 0; j < STI_STRETCH; j++) {
            cl = fma(eL[j], c, cl), sl = fma(eL[j], s, sl);
            cr = fma(eR[j], c, cr), sr = fma(eR[j], s, sr);
            const double cn = c * wc - s * ws;
            s = s * wc + c * ws, c = cn;
        }
        cl = ish_block_reduce(cl, red, add);
        sl = ish_block_reduce(sl, red, add);
        cr = ish_block_reduce(cr, red, add);
        sr = ish_block_reduce(sr, red, add);
        if (t == 0) mine[4 * f] = cl, mine[4 * f + 1] = sl, mine[4 * f + 2] = cr, mine[4 * f + 3] = sr;
    }
    EL = ish_block_reduce(EL, red, add);
    ER = ish_block_reduce(ER, red, add);
    if (t == 0) mine[4 * pl.n_mod] = EL, mine[4 * pl.n_mod + 1] = ER;
}

// fin[s] = the sum over the runs r, ascending, of part[r (4 n_mod + 2) + s].  grid (1): 4 n_mod + 2 <= 66 slots.
__global__ __launch_bounds__(STI_THREADS) void k_sti_fold(const double* __restrict__ part, StiPlan pl, double* __restrict__ fin) {
    const uint32_t slots = 4 * pl.n_mod + 2, s = threadIdx.x;
    if (s >= slots) return;
    double sum = 0.0;
    for (uint32_t r = 0; r < pl.runs; r++) sum += part[(uint64_t)r * slots + s];
    fin[s] = sum;
}
static_assert(4 * MC_STI_MAX_MOD + 2 <= STI_THREADS, "k_sti_fold is one workgroup");

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a query, in struct order, checked without touching an engine or HIP; the message (thread-local) names the
// field.  Null when it is good.
inline const char* sti_check(const mc_sti_query* q) {
    static thread_local char msg[160];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_sti_query)) return "mc_sti_query struct_size mismatch";
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    const auto bad = [&](const char* field, uint32_t i, double v, const char* rule) {
        std::snprintf(msg, sizeof(msg), "%s[%u] %g %s", field, i, v, rule);
        return msg;
    };
    if (q->n_bands > MC_STI_MAX_BANDS) {
        std::snprintf(msg, sizeof(msg), "n_bands %u above %d", q->n_bands, MC_STI_MAX_BANDS);
        return msg;
    }
    if (q->n_mod < 1 || q->n_mod > MC_STI_MAX_MOD) {
        std::snprintf(msg, sizeof(msg), "n_mod %u outside [1, %d]", q->n_mod, MC_STI_MAX_MOD);
        return msg;
    }
    if (q->flags & ~MC_STI_SNR) {
        std::snprintf(msg, sizeof(msg), "unknown bit in flags 0x%x", q->flags);
        return msg;
    }
    // (the centres alone here, with a Q that passes; q has its turn in struct order below)
    if (!dec_bands_ok(q->centre_hz, q->n_bands, 1.f, q->rate, msg, sizeof(msg))) return msg;
    for (uint32_t b = 0; b < q->n_bands; b++)
        if (const double v = q->alpha[b]; !(std::isfinite(v) && v >= 0.0)) return bad("alpha", b, v, "is not a finite weight >= 0");
    for (uint32_t b = 0; b + 1 < q->n_bands; b++)
        if (const double v = q->beta[b]; !(std::isfinite(v) && v >= 0.0)) return bad("beta", b, v, "is not a finite weight >= 0");
    if (q->flags & MC_STI_SNR)
        for (uint32_t b = 0; b < q->n_bands; b++)
            if (const double v = (double)q->snr_db[b]; !(v >= STI_MIN_SNR_DB && v <= STI_MAX_SNR_DB)) return bad("snr_db", b, v, "outside [-60, 120]");
    for (uint32_t f = 0; f < q->n_mod; f++)
        if (const double v = (double)q->mod_hz[f]; !(v >= STI_MIN_MOD_HZ && v <= STI_MAX_MOD_HZ)) return bad("mod_hz", f, v, "outside [0.1, 50]");
    if (!dec_bands_ok(nullptr, 0, q->q, q->rate, msg, sizeof(msg)) || !dec_onset_ok(q->onset_db, msg, sizeof(msg))) return msg;
    if (!q->reserved[0] && !q->reserved[1]) return nullptr;
    std::snprintf(msg, sizeof(msg), "reserved {%u, %u} must be 0", q->reserved[0], q->reserved[1]);
    return msg;
}

// step 4 of the definition for an m that is a number
inline double sti_ti(double m) {
    if (m >= 1.0) return 1.0;
    if (m <= 0.0) return 0.0;
    return std::min(std::max((10.0 * std::log10(m / (1.0 - m)) + 15.0) / 30.0, 0.0), 1.0);
}

// Steps 3 and 4 for row group g from its folded sums fin[4 n_mod + 2]: the three sets' rows (4 numbers each) and mtf entries
// (n_mod each).
inline void sti_group(const double* fin, const mc_sti_query& q, uint32_t g, double* rows, double* mtf) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t F = q.n_mod;
    const double gain = g && (q.flags & MC_STI_SNR) ? 1.0 / (1.0 + std::pow(10.0, -(double)q.snr_db[g - 1] / 10.0)) : 1.0;
    for (int s = 0; s < STI_SETS; s++) {
        const double E = s < 2 ? fin[4 * F + s] : fin[4 * F] + fin[4 * F + 1];
        const bool ok = std::isfinite(E) && E != 0.0;
        double sum = 0.0;
        for (uint32_t f = 0; f < F; f++) {
            const double* p = fin + 4 * f;
            const double Cs = s < 2 ? p[2 * s] : p[0] + p[2], Ss = s < 2 ? p[2 * s + 1] : p[1] + p[3];
            double m = nan;
            if (ok) {
                m = std::hypot(Cs, Ss) / E;
                if (g && (q.flags & MC_STI_SNR)) m *= gain;
                sum += sti_ti(m);
            }
            mtf[(size_t)s * F + f] = m;
        }
        double* row = rows + 4 * s;
        row[0] = E, row[1] = ok ? sum / (double)F : nan, row[2] = ok ? 0.0 : 1.0, row[3] = 0.0;
    }
}

// Step 5 from the rows of all groups
inline void sti_index(const mc_sti_query& q, const double* rows, double sti[3]) {
    for (int s = 0; s < STI_SETS; s++) {
        const auto mti = [&](uint32_t b) { return rows[((size_t)(b + 1) * STI_SETS + s) * 4 + 1]; };  // (NaN with status 1)
        double v = q.n_bands ? 0.0 : std::numeric_limits<double>::quiet_NaN();
        for (uint32_t b = 0; b < q.n_bands; b++) v += q.alpha[b] * mti(b);
        for (uint32_t b = 0; b + 1 < q.n_bands; b++) v -= q.beta[b] * std::sqrt(mti(b) * mti(b + 1));
        sti[s] = v;
    }
}

// The whole measurement of the n stored taps d_x for a checked query.  rows, mtf, sti, info as mc_ir_sti describes them.
// Synchronises the stream; leaves nothing allocated.
inline hipError_t sti_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_sti_query& q, double* rows, double* mtf, double sti[3],
                              uint64_t info[2]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const uint32_t slots = sti_slots(q.n_mod);
    std::vector<double> fin(slots);
    m.open(q.onset_db, N, m.cg.lanes, 0, (size_t)sti_runs(0, N) * slots, fin.size());
    const uint64_t o = m.o;
    StiPlan pl{};
    pl.o = o, pl.N = N, pl.n_mod = q.n_mod, pl.runs = sti_runs(o, N), pl.rate = (double)q.rate;
    for (uint32_t f = 0; f < q.n_mod; f++) {
        pl.F[f] = (double)q.mod_hz[f];
        const double w = 2.0 * M_PI * pl.F[f] / pl.rate;
        pl.wc[f] = std::cos(w), pl.ws[f] = std::sin(w);
    }

    for (uint32_t g = 0; g <= q.n_bands && m.er == hipSuccess; g++) {
        m.group(g ? &q.centre_hz[g - 1] : nullptr, q.q, q.rate);
        if (m.er == hipSuccess && pl.runs) {
            hipLaunchKernelGGL(k_sti_runs, dim3(pl.runs), dim3(STI_THREADS), 0, stream, m.d_buf, pl, m.d_part);
            m.launched();
        }
        if (m.er == hipSuccess) {
            hipLaunchKernelGGL(k_sti_fold, dim3(1), dim3(STI_THREADS), 0, stream, m.d_part, pl, m.d_fin);
            m.launched();
        }
        m.fetch(fin.data(), m.d_fin, sizeof(double) * fin.size());
        if (m.er != hipSuccess) break;
        sti_group(fin.data(), q, g, rows + (size_t)g * STI_SETS * 4, mtf + (size_t)g * STI_SETS * q.n_mod);
    }
    if (m.er == hipSuccess) sti_index(q, rows, sti);
    m.info(info);
    return m.er;
}
