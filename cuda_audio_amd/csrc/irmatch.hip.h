// irmatch.hip.h — the match step of an impulse-response load (mc_load_ir_match, mc_load_ir_sweep_match): the F frames get the
// tonal balance of a second impulse response (or of a flat or tilted line) by a match EQ.  The two fractional-octave-smoothed
// power spectra are compared on a logarithmic grid, the difference is bounded and applied as a smooth minimum-phase or
// linear-phase correction.  No reference equivalent.  Step 1d of the shaped load (include/mcconv.h has the definition,
// DESIGN.md 2.21 the reasons): shape_stage runs match_run on the F frames that the source and the tail, phase and filter steps
// left and hands irshape.hip.h the Fo frames it makes.  tests/ir_match_np.py states the same with numpy's FFT, one channel at
// a time.  It is the third user of fft64.hip.h.
//
// Per channel c, in double, Nfft = max(16, smallest power of two >= 2 max(F, G)):
//   A = FFT(a_c padded), T = FFT(t_c padded); Pa = |A|^2, Pt = |T|^2 for k = 0 .. Nfft / 2;
//   grid f_j = lo 2^(j / per_octave) <= hi, J points; window of j: the bins k_lo .. k_hi within f_j 2^(-+octaves / 2), from
//   the host's table; Sa[j], St[j] = the mean of Pa, Pt over the window (flat: St[j] = 10^(tilt log2(f_j / 1000) / 10));
//   linked: both channels' levels added; floor: S = max(S, max S 10^(-floor_db / 10));
//   raw = 10 log10(St / Sa), m = mean raw, d = clamp(amount (raw - m), -cut_db, boost_db)            (host, on the J points)
//   per bin: u = per_octave log2(k rate / Nfft / lo) clipped to [0, J - 1], dB by linear interpolation of d, L = dB ln 10 / 20;
//   minimum: c = Re IFFT(L), folded as the phase step folds; C = exp(FFT(c)); Fo = F;
//   linear:  C = exp(L) e^(-2 pi i k D / Nfft); Fo = F + D;
//   Y = A C; y = Re IFFT(Y); the first Fo of y, rounded to float once.
//
// Both channels ride one complex transform (fft64.hip.h), as in irphase.hip.h and irfilter.hip.h: z_a = a_L + i a_R -> Z_a,
// z_t = t_L + i t_R -> Z_t.  k_mt_power: one lane owns the pair of bins (k, Nfft - k), splits both packed spectra into the
// channels' own and writes (Pa_L, Pa_R)[k] and (Pt_L, Pt_R)[k] as double2, k = 0 .. Nfft / 2, each signal in a stretch of its
// own whose length is a multiple of 256 elements, so that a row of 256 bins is 4 KiB on a 4 KiB boundary in both.
//
// k_mt_smooth is the step's own loop.  One workgroup per (grid point, signal): lane l takes the bins 256 r + l of the rows r that
// the window [k_lo, k_hi] touches, in ascending r, four rows' loads in flight ahead of their adds; the 256 partial sums are
// joined by a fixed tree in LDS.  The order of the additions is a function of (k_lo, k_hi) alone: the same window gives the same
// bits whatever else is asked.  The windows overlap heavily (up to 0.6 Nfft / 2 bins each at two octaves), so most loads are
// served from cache.  No prefix sums: a spectrum here spans 120 dB and more, and the difference of two large prefixes loses
// a quiet window entirely; every window is added up from its own bins.
//
// k_mt_gain: one lane per bin k <= Nfft / 2 interpolates the curve and writes L[k] and L[Nfft - k], (L_L, L_R) as one complex
// number when the channels have curves of their own, (L, 0) when they are linked.  The cepstral path is the phase step's:
// IFFT, k_ph_fold, FFT, then k_ph_exp for two curves (it separates the two cepstra's spectra as k_ph_power separates Z) and
// k_mt_exp for one.  k_mt_linear makes the linear-phase correction from L.  k_mt_apply: Y = A C in place, by pairs of bins for
// two curves (as k_fl_mul_pair) and bin by bin for one (as k_fl_mul_mono).  k_fl_pack and k_fl_unpack (irfilter.hip.h) are
// used as they are: they carry the energies that go in, that are stored and that are left behind past Fo, one partial per
// workgroup, added on the host in index order.  No atomics; grids that depend on F, G, J and Nfft alone.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "irfilter.hip.h"
#include "irphase.hip.h"
#include "irspectral.hip.h"

constexpr int MT_MAX_LOG2 = F64_MAX_LOG2;  // Nfft <= 2^22
constexpr int MT_THREADS = ISH_THREADS;
constexpr uint32_t MT_MAX_POINTS = 1024;
constexpr uint32_t MT_MAX_DELAY = 1u << 20;
constexpr int MT_ROWS = 4;  // rows of 256 bins whose loads k_mt_smooth issues before it adds them

// a checked mc_ir_match that is on, over F frames and a target of G frames, both at the session's rate
struct MatchStep {
    uint64_t F = 0, G = 0, Fo = 0, Nfft = 0, D = 0;
    uint32_t mode = 0, phase = 0, link = 1, J = 0, per_octave = 0;
    double rate = 0, lo = 0, hi = 0, octaves = 0, amount = 0, boost_db = 0, cut_db = 0, floor_db = 0, tilt_db = 0;
    Fft64Plan fft{};
    std::vector<double> hz;     // f_j
    std::vector<uint32_t> win;  // k_lo, k_hi of point j at [2 j], [2 j + 1]
    uint64_t window_bins = 0;   // the sum of the windows' widths
    SecondIr second;            // where the target's frames come from
};

// what match_run hands back beside the taps: mc_ir_match_info's twelve numbers and mc_ir_match_curve's arrays
struct MatchFacts {
    double info[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> curve;  // hz[J], then (before L, before R)[J], then (gain L, gain R)[J]
};

// (Pa_L, Pa_R)[k] and, with Zt, (Pt_L, Pt_R)[k] at P[k] and P[stride + k], for the pair of bins (k, N - k), k <= N / 2
__global__ __launch_bounds__(MT_THREADS) void k_mt_power(const double2* __restrict__ Za, const double2* __restrict__ Zt, uint64_t N, uint64_t stride,
                                                         double2* __restrict__ P) {
    const uint64_t k = (uint64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (k > N / 2) return;
    const uint64_t km = (N - k) & (N - 1);
    double2 l, r;
    fl_split(Za[k], Za[km], l, r);
    P[k] = make_double2(l.x * l.x + l.y * l.y, r.x * r.x + r.y * r.y);
    if (Zt) {
        fl_split(Zt[k], Zt[km], l, r);
        P[stride + k] = make_double2(l.x * l.x + l.y * l.y, r.x * r.x + r.y * r.y);
    }
}

// S[s J + j] = the sums of both channels' powers of signal s = blockIdx.y over the window win[j] = (k_lo, k_hi) of point
// j = blockIdx.x, 1 <= k_lo <= k_hi <= half (anything else sums to zero, and k_hi is clipped to half).  Lane l adds the bins
// 256 r + l inside the window in ascending r; then a fixed tree over the 256 lanes.
__global__ __launch_bounds__(MT_THREADS) void k_mt_smooth(const double2* __restrict__ P, uint64_t stride, const uint2* __restrict__ win, uint32_t J,
                                                          uint64_t half, double2* __restrict__ S) {
    __shared__ double2 red[MT_THREADS];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    const double2* __restrict__ p = P + (uint64_t)blockIdx.y * stride;
    const uint2 w = win[j];
    const uint64_t k_lo = w.x, k_hi = w.y < half ? w.y : half;
    double2 acc = make_double2(0.0, 0.0);
    if (k_lo >= 1 && k_lo <= k_hi) {
        for (uint64_t row = k_lo & ~(uint64_t)(MT_THREADS - 1); row <= k_hi; row += MT_ROWS * MT_THREADS) {
            double2 v[MT_ROWS];
#pragma unroll
            for (int r = 0; r < MT_ROWS; r++) {
                const uint64_t k = row + (uint64_t)r * MT_THREADS + t;
                v[r] = k >= k_lo && k <= k_hi ? p[k] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int r = 0; r < MT_ROWS; r++) acc.x += v[r].x, acc.y += v[r].y;
        }
    }
    red[t] = acc;
    __syncthreads();
    for (uint32_t s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double2 a = red[t], b = red[t + s];
            red[t] = make_double2(a.x + b.x, a.y + b.y);
        }
        __syncthreads();
    }
    if (t == 0) S[(uint64_t)blockIdx.y * J + j] = red[0];
}

// Lg[k] and Lg[N - k] = (L_L, L_R)[k] (two curves) or (L, 0)[k] (one), k <= N / 2: the curve d (dB per channel at the J grid
// points lo 2^(j / per_octave)) interpolated at k rate / N Hz, flat outside the grid, times ln 10 / 20
__global__ __launch_bounds__(MT_THREADS) void k_mt_gain(const double2* __restrict__ d, uint32_t J, double per_octave, double rate, double lo, int two,
                                                        uint64_t N, double2* __restrict__ Lg) {
    const uint64_t k = (uint64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (k > N / 2) return;
    double u = 0.0;
    if (k) u = per_octave * log2((double)k * rate / (double)N / lo);
    u = fmin(fmax(u, 0.0), (double)(J - 1));
    uint32_t i = (uint32_t)floor(u);
    if (i > J - 2) i = J - 2;
    const double2 a = d[i], b = d[i + 1];
    const double f = u - (double)i, ln10_20 = 0.11512925464970228420;  // ln 10 / 20
    const double2 v = make_double2((a.x + f * (b.x - a.x)) * ln10_20, two ? (a.y + f * (b.y - a.y)) * ln10_20 : 0.0);
    Lg[k] = v;
    Lg[(N - k) & (N - 1)] = v;
}

// one curve, minimum phase: C[k] = exp(Z[k]), Z = FFT of the folded cepstrum
__global__ __launch_bounds__(MT_THREADS) void k_mt_exp(const double2* __restrict__ Z, uint64_t N, double2* __restrict__ Cs) {
    const uint64_t k = (uint64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (k < N) Cs[k] = ph_cexp(Z[k]);
}

// linear phase: C[k] = exp(L[k]) e^(-2 pi i k D / N), the angle reduced as (k D mod N) first; two curves: C_L + i C_R
__global__ __launch_bounds__(MT_THREADS) void k_mt_linear(const double2* __restrict__ Lg, uint64_t N, uint64_t D, int two, double2* __restrict__ Cs) {
    const uint64_t k = (uint64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (k >= N) return;
    const double2 l = Lg[k];
    double sn, cs;
    sincospi(-2.0 * (double)((k * D) & (N - 1)) / (double)N, &sn, &cs);
    const double gl = exp(l.x), gr = two ? exp(l.y) : 0.0;
    // C_L = gl (cs + i sn); C_R = gr (cs + i sn); C_L + i C_R
    Cs[k] = make_double2(gl * cs - gr * sn, gl * sn + gr * cs);
}

// Y = A C in place.  two: lane k <= N / 2 owns the pair (k, N - k) of both packed spectra (as k_fl_mul_pair); else lane k < N
// multiplies bin by bin (as k_fl_mul_mono)
__global__ __launch_bounds__(MT_THREADS) void k_mt_apply(double2* __restrict__ Za, const double2* __restrict__ Cs, uint64_t N, int two) {
    const uint64_t k = (uint64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (!two) {
        if (k < N) Za[k] = fl_mul(Za[k], Cs[k]);
        return;
    }
    if (k > N / 2) return;
    const uint64_t km = (N - k) & (N - 1);
    double2 al, ar, cl, cr;
    fl_split(Za[k], Za[km], al, ar);
    fl_split(Cs[k], Cs[km], cl, cr);
    fl_store_pair(Za, k, km, fl_mul(al, cl), fl_mul(ar, cr));
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a match step that is on, in the struct's order, checked without touching an engine or HIP; the message
// (thread-local) names the field.  Null when it is good.
inline const char* match_check(const mc_ir_match* m) {
    static thread_local char msg[200];
    if (m->struct_size != sizeof(mc_ir_match)) return "mc_ir_match struct_size mismatch";
    if (m->mode > MC_MATCH_FLAT) {
        std::snprintf(msg, sizeof(msg), "mode %u is not an MC_MATCH_OFF / TARGET / FLAT value", m->mode);
        return msg;
    }
    if (m->phase > MC_MATCH_LINEAR) {
        std::snprintf(msg, sizeof(msg), "phase %u is not an MC_MATCH_MINIMUM / LINEAR value", m->phase);
        return msg;
    }
    if (m->link > 1) {
        std::snprintf(msg, sizeof(msg), "link %u is not 0 or 1", m->link);
        return msg;
    }
    if (m->rate && (m->rate < RS_MIN_RATE || m->rate > RS_MAX_RATE)) {
        std::snprintf(msg, sizeof(msg), "the target's rate %u outside [%u, %u] (0 = the session's)", m->rate, RS_MIN_RATE, RS_MAX_RATE);
        return msg;
    }
    if (m->per_octave < 1 || m->per_octave > 96) {
        std::snprintf(msg, sizeof(msg), "per_octave %u outside [1, 96]", m->per_octave);
        return msg;
    }
    if (!(m->lo_hz >= 1.0 && m->lo_hz <= 192000.0)) {
        std::snprintf(msg, sizeof(msg), "lo_hz %g outside [1, 192000]", m->lo_hz);
        return msg;
    }
    if (!(m->hi_hz == 0.0 || (m->hi_hz > m->lo_hz && m->hi_hz <= 192000.0))) {
        std::snprintf(msg, sizeof(msg), "hi_hz %g is neither 0 (the default) nor within (lo_hz, 192000]", m->hi_hz);
        return msg;
    }
    if (!(m->octaves >= 1.0 / 24.0 && m->octaves <= 2.0)) {
        std::snprintf(msg, sizeof(msg), "octaves %g outside [1/24, 2]", m->octaves);
        return msg;
    }
    if (!(m->amount >= 0.f && m->amount <= 1.f)) {
        std::snprintf(msg, sizeof(msg), "amount %g outside [0, 1]", (double)m->amount);
        return msg;
    }
    if (!(m->boost_db >= 0.f && m->boost_db <= 60.f)) {
        std::snprintf(msg, sizeof(msg), "boost_db %g outside [0, 60]", (double)m->boost_db);
        return msg;
    }
    if (!(m->cut_db >= 0.f && m->cut_db <= 60.f)) {
        std::snprintf(msg, sizeof(msg), "cut_db %g outside [0, 60]", (double)m->cut_db);
        return msg;
    }
    if (!(m->floor_db >= 40.f && m->floor_db <= 300.f)) {
        std::snprintf(msg, sizeof(msg), "floor_db %g outside [40, 300]", (double)m->floor_db);
        return msg;
    }
    if (!(m->tilt_db >= -12.f && m->tilt_db <= 12.f)) {
        std::snprintf(msg, sizeof(msg), "tilt_db %g outside [-12, 12]", (double)m->tilt_db);
        return msg;
    }
    if (m->delay > MT_MAX_DELAY) {
        std::snprintf(msg, sizeof(msg), "delay %u above %u frames", m->delay, MT_MAX_DELAY);
        return msg;
    }
    if (m->reserved[0] || m->reserved[1]) {
        std::snprintf(msg, sizeof(msg), "the match's reserved words are %u and %u, not 0", m->reserved[0], m->reserved[1]);
        return msg;
    }
    return nullptr;
}

// hi_hz as the step uses it: its own, or min(20000, rate / 2)
inline double match_hi(const mc_ir_match* m, uint32_t session_rate) { return m->hi_hz != 0.0 ? m->hi_hz : std::min(20000.0, 0.5 * (double)session_rate); }

// the grid's points: f_j = lo 2^(j / per_octave) while that double is <= hi (mc_response_grid's rule, kept in double); at most
// MT_MAX_POINTS + 1 are counted
inline uint32_t match_grid(double lo, double hi, uint32_t per_octave, std::vector<double>* hz) {
    uint32_t j = 0;
    for (; j <= MT_MAX_POINTS; j++) {
        const double v = lo * std::exp2((double)j / (double)per_octave);
        if (!(v <= hi)) break;
        if (hz) hz->push_back(v);
    }
    return j;
}

// log2 of the transform: max(16, smallest power of two >= 2 max(F, G)); above MT_MAX_LOG2 when that is too long
inline int match_log2(uint64_t F, uint64_t G) { return spec_ceil_log2(2 * std::max(F, G), F64_MIN_LOG2); }

// The limits of a checked match step in a load whose F frames at the session's rate are known, in the documented order: the
// session's rate, hi_hz, the grid, the target's frames (target_frames at m's rate become *G at the session's), Nfft, delay.
inline const char* match_check_load(const mc_ir_match* m, uint32_t session_rate, uint64_t F, uint64_t target_frames, uint64_t* G) {
    static thread_local char msg[240];
    *G = 0;
    if (!F) return nullptr;  // (the load's own "empty IR")
    if (!session_rate) return "the match step's grid is in Hz and needs the session's rate: session_rate is 0";
    if (session_rate < RS_MIN_RATE || session_rate > RS_MAX_RATE) {
        std::snprintf(msg, sizeof(msg), "session_rate %u outside [%u, %u] (the match step needs it)", session_rate, RS_MIN_RATE, RS_MAX_RATE);
        return msg;
    }
    const double hi = match_hi(m, session_rate);
    if (hi > 0.5 * (double)session_rate) {
        std::snprintf(msg, sizeof(msg), "hi_hz %g above half the session's rate %u", hi, session_rate);
        return msg;
    }
    const uint32_t J = match_grid(m->lo_hz, hi, m->per_octave, nullptr);
    if (J < 2 || J > MT_MAX_POINTS) {
        std::snprintf(msg, sizeof(msg), "lo_hz %g, hi_hz %g and per_octave %u give a grid of %s%u points, outside [2, %u]", m->lo_hz, hi, m->per_octave,
                      J > MT_MAX_POINTS ? "more than " : "", std::min(J, MT_MAX_POINTS), MT_MAX_POINTS);
        return msg;
    }
    if (m->mode == MC_MATCH_TARGET) {
        if (!target_frames) return "empty target: target_frames is 0";
        if (target_frames > (1ull << 40)) {
            std::snprintf(msg, sizeof(msg), "target of %llu frames (target_frames)", (unsigned long long)target_frames);
            return msg;
        }
        *G = second_frames_at(m->rate, session_rate, target_frames);
    }
    const int lg = match_log2(F, *G);
    if (lg > MT_MAX_LOG2) {
        std::snprintf(msg, sizeof(msg), "%llu frames and %llu target frames at the session's rate need a transform of more than 2^%d points",
                      (unsigned long long)F, (unsigned long long)*G, MT_MAX_LOG2);
        return msg;
    }
    if (m->phase == MC_MATCH_LINEAR && F + m->delay > (1ull << lg)) {
        std::snprintf(msg, sizeof(msg), "delay %u with %llu frames is beyond the transform's %llu points", m->delay, (unsigned long long)F, 1ull << lg);
        return msg;
    }
    return nullptr;
}

// a checked match step that is on, over F frames and G target frames within the limits (the source of the target's frames is
// the caller's to fill in)
inline MatchStep match_step(const mc_ir_match& m, uint32_t session_rate, uint64_t F, uint64_t G) {
    MatchStep s;
    const int lg = match_log2(std::max<uint64_t>(F, 1), G);
    s.F = F, s.G = G, s.Nfft = 1ull << lg;
    s.mode = m.mode, s.phase = m.phase, s.link = m.link, s.per_octave = m.per_octave;
    s.D = m.phase == MC_MATCH_LINEAR ? m.delay : 0;
    s.Fo = F + s.D;
    s.rate = (double)session_rate, s.lo = m.lo_hz, s.hi = match_hi(&m, session_rate), s.octaves = m.octaves;
    s.amount = (double)m.amount, s.boost_db = (double)m.boost_db, s.cut_db = (double)m.cut_db, s.floor_db = (double)m.floor_db, s.tilt_db = (double)m.tilt_db;
    s.fft = fft64_plan(lg);
    s.J = match_grid(s.lo, s.hi, s.per_octave, &s.hz);
    const double down = std::exp2(-0.5 * s.octaves), up = std::exp2(0.5 * s.octaves), N = (double)s.Nfft, half = (double)(s.Nfft / 2);
    const auto clip = [half](double k) { return (uint32_t)std::min(std::max(k, 1.0), half); };
    for (uint32_t j = 0; j < s.J; j++) {
        const double klo = std::ceil(s.hz[j] * down * N / s.rate), khi = std::floor(s.hz[j] * up * N / s.rate);
        uint32_t a = clip(klo), b = clip(khi);
        if (a > b) a = b = clip(std::nearbyint(s.hz[j] * N / s.rate));
        s.win.push_back(a), s.win.push_back(b);
        s.window_bins += b - a + 1;
    }
    return s;
}

// the length of one signal's stretch of powers: Nfft / 2 + 1 bins, rounded up to whole rows of 256
inline uint64_t match_stride(const MatchStep& s) { return spec_groups(s.Nfft / 2 + 1) * MT_THREADS; }

// what match_run allocates on the device while it runs: the target's G frames, two buffers of Nfft double2 and a third when
// the transform has two passes, the two stretches of powers (which hold the correction's spectrum afterwards), the partials,
// the window table, the sums and the curve (the resampler's own temporaries for a target at another rate are not counted)
inline uint64_t match_device_bytes(const MatchStep& s) {
    return 8 * s.G + spec_work_bytes(s.fft, s.Nfft) + 2 * 16 * match_stride(s) + 8 * s.J + 2 * 16 * s.J + 16 * s.J;
}

// The curve on the J points, host arithmetic in double.  S = the four sums per point as k_mt_smooth left them: (L, R) of the
// source at [2 j], [2 j + 1], of the target at [2 J + 2 j], ..; Ea, Et = the channels' energies before the transform, which
// decide whether a signal is all zeros.  before[2 j + c] = raw - m and gain[2 j + c] = d of channel c; mean[c] = m;
// *clamped = the points of the curves (one when linked, two otherwise) whose amount (raw - m) lies outside the range.
inline void match_curve(const MatchStep& s, const double* S, const double Ea[2], const double Et[2], double* before, double* gain, double mean[2],
                        uint64_t* clamped) {
    const uint32_t J = s.J;
    const bool flat = s.mode == MC_MATCH_FLAT;
    const double rel = std::pow(10.0, -s.floor_db / 10.0);
    std::vector<double> sa(J), st(J);
    *clamped = 0;
    for (int c = 0; c < (s.link ? 1 : 2); c++) {
        const bool src_zero = s.link ? Ea[0] + Ea[1] == 0.0 : Ea[c] == 0.0;
        const bool tgt_zero = !flat && (s.link ? Et[0] + Et[1] == 0.0 : Et[c] == 0.0);
        double ma = 0.0, mt = 0.0;
        for (uint32_t j = 0; j < J; j++) {
            const double n = (double)(s.win[2 * j + 1] - s.win[2 * j] + 1);
            sa[j] = s.link ? S[2 * j] / n + S[2 * j + 1] / n : S[2 * j + c] / n;
            if (flat) {
                const double one = std::pow(10.0, s.tilt_db * std::log2(s.hz[j] / 1000.0) / 10.0);
                st[j] = s.link ? one + one : one;
            } else {
                st[j] = s.link ? S[2 * J + 2 * j] / n + S[2 * J + 2 * j + 1] / n : S[2 * J + 2 * j + c] / n;
            }
            ma = std::max(ma, sa[j]), mt = std::max(mt, st[j]);
        }
        double m = 0.0;
        uint64_t hit = 0;
        std::vector<double> raw(J, 0.0);
        if (!src_zero && !tgt_zero && ma > 0.0 && mt > 0.0) {
            for (uint32_t j = 0; j < J; j++) {
                raw[j] = 10.0 * std::log10(std::max(st[j], mt * rel) / std::max(sa[j], ma * rel));
                m += raw[j];
            }
            m /= (double)J;
        }
        for (uint32_t j = 0; j < J; j++) {
            const double b = raw[j] - m, want = s.amount * b, d = std::min(std::max(want, -s.cut_db), s.boost_db);
            hit += want < -s.cut_db || want > s.boost_db;
            before[2 * j + c] = b, gain[2 * j + c] = d;
            if (s.link) before[2 * j + 1] = b, gain[2 * j + 1] = d;
        }
        mean[c] = m;
        if (s.link) mean[1] = m;
        *clamped += hit;
    }
}

// Step 1d: the s.Fo frames d_y from the s.F frames d_x and the target's host frames, on the stream, after what the stream
// already holds.  Allocates the work buffers (SpectralWork and its own), waits for the kernels and frees them.
inline hipError_t match_run(hipStream_t stream, const float2* d_x, float2* d_y, const MatchStep& s, MatchFacts* facts) {
    const uint64_t F = s.F, G = s.G, Fo = s.Fo, N = s.Nfft, gF = spec_groups(F), gG = spec_groups(G), gN = spec_groups(N);
    const uint64_t gH = spec_groups(N / 2 + 1), stride = match_stride(s);
    const uint32_t J = s.J;
    const bool target = s.mode == MC_MATCH_TARGET;
    const int two = s.link ? 0 : 1;
    DevArray<float2> d_t;
    DevArray<double2> d_P, d_S, d_d;
    DevArray<uint2> d_win;
    std::vector<double> S(8 * (size_t)J, 0.0);
    SpectralWork wk;
    hipError_t er = target ? d_t.alloc(G) : hipSuccess;
    if (er == hipSuccess) er = wk.alloc(s.fft, N);
    if (er == hipSuccess) er = d_P.alloc(2 * stride);
    if (er == hipSuccess) er = d_win.alloc(J);
    if (er == hipSuccess) er = d_S.alloc(2 * (size_t)J);
    if (er == hipSuccess) er = d_d.alloc(J);
    if (er == hipSuccess) er = hipMemcpy(d_win, s.win.data(), sizeof(uint2) * J, hipMemcpyHostToDevice);
    if (er == hipSuccess && target) er = second_upload(stream, s.second, d_t, G);
    double2 *const d_a = wk.d_a, *const d_b = wk.d_b, *const d_w = wk.d_w;
    double* const d_part = wk.d_part;
    const std::vector<double>& part = wk.part;
    const auto fetch = [&](uint64_t count) { return wk.fetch(stream, count); };
    // A channel whose frames are all zero is recognised from its energy before the transform: the packed transform leaves
    // rounding noise of the other channel in its spectrum (irfilter.hip.h has the same device).
    double Ea[2] = {0.0, 0.0}, Et[2] = {0.0, 0.0}, Eout = 0.0, Erest = 0.0, mean[2] = {0.0, 0.0};
    uint64_t clamped = 0;
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_fl_pack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, d_x, F, N, (uint32_t)MC_FILTER_STEREO, d_a, d_part);
        er = fetch(2 * gF);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gF; b++) Ea[0] += part[2 * b], Ea[1] += part[2 * b + 1];
        if (target) {
            hipLaunchKernelGGL(k_fl_pack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, (const float2*)d_t, G, N, (uint32_t)MC_FILTER_STEREO, d_b, d_part);
            er = fetch(2 * gG);
            if (er == hipSuccess)
                for (uint64_t b = 0; b < gG; b++) Et[0] += part[2 * b], Et[1] += part[2 * b + 1];
        }
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_a, d_a, d_w, false);
    if (er == hipSuccess && target) er = fft64_run(stream, s.fft, d_b, d_b, d_w, false);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_mt_power, dim3((unsigned)gH), dim3(MT_THREADS), 0, stream, (const double2*)d_a, target ? (const double2*)d_b : nullptr, N, stride,
                           d_P);
        hipLaunchKernelGGL(k_mt_smooth, dim3(J, target ? 2 : 1), dim3(MT_THREADS), 0, stream, (const double2*)d_P, stride, (const uint2*)d_win, J, N / 2, d_S);
        er = hipGetLastError();
        // the 4 J sums in one round trip
        if (er == hipSuccess) er = hipMemcpyAsync(S.data(), d_S, sizeof(double2) * (target ? 2 : 1) * J, hipMemcpyDeviceToHost, stream);
        if (er == hipSuccess) er = hipStreamSynchronize(stream);
    }
    facts->curve.assign(5 * (size_t)J, 0.0);
    double* const before = facts->curve.data() + J;
    double* const gain = before + 2 * (size_t)J;
    if (er == hipSuccess) {
        std::copy(s.hz.begin(), s.hz.end(), facts->curve.begin());
        match_curve(s, S.data(), Ea, Et, before, gain, mean, &clamped);
        er = hipMemcpy(d_d, gain, sizeof(double2) * J, hipMemcpyHostToDevice);
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_mt_gain, dim3((unsigned)gH), dim3(MT_THREADS), 0, stream, (const double2*)d_d, J, (double)s.per_octave, s.rate, s.lo, two, N, d_b);
        er = hipGetLastError();
    }
    // the correction's spectrum into d_P, whose 2 stride >= Nfft elements the powers no longer need
    if (er == hipSuccess && s.phase == MC_MATCH_MINIMUM) {
        er = fft64_run(stream, s.fft, d_b, d_b, d_w, true);
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_ph_fold, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, d_b, N);
            er = hipGetLastError();
        }
        if (er == hipSuccess) er = fft64_run(stream, s.fft, d_b, d_b, d_w, false);
        if (er == hipSuccess) {
            if (two)
                hipLaunchKernelGGL(k_ph_exp, dim3((unsigned)gN), dim3(PH_THREADS), 0, stream, (const double2*)d_b, N, d_P);
            else
                hipLaunchKernelGGL(k_mt_exp, dim3((unsigned)gN), dim3(MT_THREADS), 0, stream, (const double2*)d_b, N, d_P);
            er = hipGetLastError();
        }
    } else if (er == hipSuccess) {
        hipLaunchKernelGGL(k_mt_linear, dim3((unsigned)gN), dim3(MT_THREADS), 0, stream, (const double2*)d_b, N, s.D, two, d_P);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_mt_apply, dim3((unsigned)(two ? gH : gN)), dim3(MT_THREADS), 0, stream, d_a, (const double2*)d_P, N, two);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_a, d_a, d_w, true);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_fl_unpack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, (const double2*)d_a, Fo, N, (int)(Ea[0] > 0.0), (int)(Ea[1] > 0.0), d_y,
                           d_part);
        er = fetch(2 * gN);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gN; b++) Eout += part[2 * b], Erest += part[2 * b + 1];
        const double inf[12] = {(double)F, (double)G, (double)Fo, (double)N, (double)J, Ea[0] + Ea[1], Et[0] + Et[1], Eout, Erest, mean[0], mean[1], (double)clamped};
        std::copy(inf, inf + 12, facts->info);
    } else {
        (void)hipStreamSynchronize(stream);
    }
    return er;
}
