// irdecay.hip.h — the decay of a loaded impulse response, measured on the device (mc_ir_decay): energy decay curve, EDT,
// T20, T30, C50, C80, D50 and centre time, broadband and in up to MC_DECAY_MAX_BANDS band-passed rows.  No reference
// equivalent.  include/mcconv.h and DESIGN.md 2.9 hold the definition; tests/ir_decay_np.py states it in float64.
//
// The stored taps x [n] (float2, what the engine convolves with) are only read.  With N = end ? min(end, n) : n:
//   origin  o = the onset of irshape.hip.h (k_shape_peak, k_shape_onset over taps [0, N)) or 0;
//   per row group (broadband, then one per band):
//     fill    buf[m] = (double) x[m], m < N (k_dec_fill);
//     filter  a band's two identical sections run over buf in place through ireq.hip.h's chunked recurrence, unchanged:
//             k_eq_chunk (nxt = section), k_eq_carry, k_eq_chunk (cur = nxt = section: the first section's fix-up is the
//             second's local pass), k_eq_carry, k_eq_chunk (cur = section);
//     sum     buf[m] = EDC[m] = sum over k in [max(m, o), N) of (yL[k]^2, yR[k]^2), the backward running sum (below);
//     read    k_dec_pick gathers EDC at o, N - 1, k50, k80 and the curve's points; k_dec_members reduces, for the three
//             channel sets and the three fit ranges, how many taps lie in the range and the first of them, and sum EDC[m]
//             over m in (o, N) (= sum (m - o) e[m] by parts: the centre time without a second pass over e);
//             k_dec_fit reduces sum x, sum y, sum x^2, sum x y over each range with x counted from the range's first tap.
//   The host turns those into the eight numbers of a row and the curve (dec_row).
//
// The backward sum.  The taps are cut into chunks of IEQ_CHUNK, a function of N alone; a lane owns one (chunk, channel) and
// walks it from its last tap to its first, one addition per tap in a fixed order.
//   totals  k_dec_sum<false> keeps the sum of every chunk;
//   carry   k_dec_carry replaces total c by the sum of the totals behind it, tot[c] = tot'[c + 1] + total[c + 1], one chain of
//           additions per channel from the last chunk to the first (one workgroup, the totals staged through LDS DEC_CARRY_TILE
//           chunks at a time, lanes 0 and 1 add);
//   write   k_dec_sum<true> walks every chunk again and writes carry + running sum over the tap.
// A chunk's running sum starts from zero in both walks, so the value at its first tap is carry + total exactly, which is the
// carry of the chunk before: across a run of zero taps (a quiet lead, a band's output before the first sample) EDC stays
// bit for bit level, chunk borders included, as a sequential sum does.  L[o] = 10 log10(EDC[o] / EDC[o]) is 0 exactly.
//
// Memory.  k_dec_sum is chunkwalk.hip.h's chunk_walk, backward: its head says how the taps reach the lanes.  The map kernels read
// buf one double2 per lane, consecutively.
//
// Determinism.  Chunks, grids and the carry's order depend on N alone; no atomics; every reduction ends in one partial per
// workgroup, combined on the host in index order.  The same query on the same taps gives the same bits.
//
// Scratch (double2 [N], the chunk states, the partials) is allocated by the call and freed before it returns: an engine
// nobody asks holds nothing.
//
// The host side.  N, the scratch, the origin, a row group's fill and filter, the backward sum and the fetches are the operations
// of one struct, Measure, in the host section below (not in a header of its own: irfloor, irdensity, iriacc, irsti and
// irresponse.hip.h include this one for its kernels already).  Their *_measure functions are written on it as dec_measure is.
#pragma once
#include <limits>

#include "ireq.hip.h"

constexpr int DEC_CARRY_TILE = 2048;     // chunks of the carry pass in LDS at a time (x 2 channels x 8 bytes = 32 KiB)
constexpr int DEC_CARRY_THREADS = 256;
constexpr unsigned DEC_GRID = 512;       // workgroups of the member and fit reductions, at most
constexpr int DEC_SETS = 3, DEC_RANGES = 3, DEC_FITS = DEC_SETS * DEC_RANGES;
constexpr int DEC_MEMBER_PART = 2 * DEC_FITS + 2;  // per workgroup: 9 counts, 9 first taps, sum EDC_L, sum EDC_R
constexpr int DEC_FIT_PART = 4 * DEC_FITS;         // per workgroup: sum x, sum y, sum x^2, sum x y of each fit
constexpr int DEC_PICK_HEAD = 4;                   // k_dec_pick: EDC at o, N - 1, k50, k80, then the curve's points
constexpr double DEC_MIN_ONSET_DB = -120.0, DEC_CURVE_FLOOR = -400.0;
constexpr uint32_t DEC_MIN_RATE = 8000, DEC_MAX_RATE = 384000;
// (hi, lo) dB of EDT, T20, T30
constexpr double DEC_HI[DEC_RANGES] = {0.0, -5.0, -5.0}, DEC_LO[DEC_RANGES] = {-10.0, -25.0, -35.0};

struct DecLevels {
    double E[DEC_SETS];            // EDC[o] of L, R and L + R
    uint64_t first[DEC_FITS];      // (k_dec_fit) the first tap of fit 3 set + range
};

// buf[m] = tap m as double
__global__ __launch_bounds__(ISH_THREADS) void k_dec_fill(const float2* __restrict__ x, uint64_t n, double2* __restrict__ buf) {
    const uint64_t m = (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x;
    if (m >= n) return;
    const float2 v = x[m];
    buf[m] = make_double2((double)v.x, (double)v.y);
}

// One backward walk over buf [n] (the file's head).  tot: double [gridDim.x * IEQ_THREADS],
// entry 2 * chunk + channel.  WRITE = false: tot = the sum of y^2 over the chunk's taps in [o, n).  WRITE = true: tap m of buf
// becomes tot + the sum of y^2 over the chunk's taps in [max(m, o), n).  Taps at and past n read as zero and are not written.
template <bool WRITE>
__global__ __launch_bounds__(IEQ_THREADS) void k_dec_sum(double2* __restrict__ buf, uint64_t o, uint64_t n, double* __restrict__ tot) {
    const uint64_t entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    const double carry = WRITE ? tot[entry] : 0.0;
    double s = 0.0;
    chunk_walk<true, IEQ_TILE, double2>(
        WRITE, [&](uint64_t g, double2& v) { v = g < n ? buf[g] : make_double2(0.0, 0.0); },
        [&](double& tap, uint64_t m) {
            const double v = tap;
            if (m >= o) s += v * v;
            if (WRITE) tap = carry + s;
        },
        [&](uint64_t g, double2 v) {
            if (g < n) buf[g] = v;
        });
    if (!WRITE) tot[entry] = s;
}

// tot[2 c + ch], c < nchunks: in, the sum of chunk c; out, the sum of the chunks behind it, added up from the last chunk to
// the first in one chain per channel.  One workgroup.
__global__ __launch_bounds__(DEC_CARRY_THREADS) void k_dec_carry(double* __restrict__ tot, uint32_t nchunks) {
    __shared__ double tile[2 * DEC_CARRY_TILE];
    const int t = threadIdx.x;
    double S = 0.0;  // (lanes 0 and 1: their channel's running sum)
    for (int64_t hi = (int64_t)nchunks; hi > 0; hi -= DEC_CARRY_TILE) {
        const int64_t lo = hi > DEC_CARRY_TILE ? hi - DEC_CARRY_TILE : 0;
        const int cnt = 2 * (int)(hi - lo);
        for (int i = t; i < cnt; i += DEC_CARRY_THREADS) tile[i] = tot[2 * lo + i];
        __syncthreads();
        if (t < 2)
            for (int i = cnt - 2 + t; i >= 0; i -= 2) {
                const double v = tile[i];
                tile[i] = S;
                S += v;
            }
        __syncthreads();
        for (int i = t; i < cnt; i += DEC_CARRY_THREADS) tot[2 * lo + i] = tile[i];
        __syncthreads();
    }
}

// out[j] = EDC at o, n - 1, k50, k80 (j < 4; an index at or past n: zero) and at the K points of the curve,
// o + floor(j' (n - 1 - o) / (K - 1))
__global__ __launch_bounds__(ISH_THREADS) void k_dec_pick(const double2* __restrict__ buf, uint64_t o, uint64_t n, uint64_t k50, uint64_t k80,
                                                          uint32_t K, double2* __restrict__ out) {
    const uint32_t j = blockIdx.x * ISH_THREADS + threadIdx.x;
    if (j >= DEC_PICK_HEAD + K) return;
    uint64_t m;
    if (j < DEC_PICK_HEAD)
        m = j == 0 ? o : (j == 1 ? n - 1 : (j == 2 ? k50 : k80));
    else
        m = o + (uint64_t)(j - DEC_PICK_HEAD) * (n - 1 - o) / (uint64_t)(K - 1);
    out[j] = m < n ? buf[m] : make_double2(0.0, 0.0);
}

// EDC of set s at a tap and its level against E in dB (NaN when E = 0, -inf when the sum has run out)
__device__ inline double dec_edc(double2 v, int s) { return s == 0 ? v.x : (s == 1 ? v.y : v.x + v.y); }
__device__ inline double dec_level(double edc, double E) { return 10.0 * log10(edc / E); }

// part[DEC_MEMBER_PART b ..] of workgroup b over its taps in [o, n): for fit f = 3 set + range the number of taps with
// lo <= L <= hi (part[f]) and the first of them (part[9 + f], n when there is none; both exact in double), then the sums of
// EDC_L and EDC_R over the taps after o.
__global__ __launch_bounds__(ISH_THREADS) void k_dec_members(const double2* __restrict__ buf, uint64_t o, uint64_t n, DecLevels lv,
                                                             double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t stride = (uint64_t)gridDim.x * ISH_THREADS;
    double cnt[DEC_FITS], first[DEC_FITS], sum[2] = {0.0, 0.0};
    for (int f = 0; f < DEC_FITS; f++) cnt[f] = 0.0, first[f] = (double)n;
    for (uint64_t m = o + (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x; m < n; m += stride) {
        const double2 v = buf[m];
        if (m > o) sum[0] += v.x, sum[1] += v.y;
#pragma unroll
        for (int s = 0; s < DEC_SETS; s++) {
            const double L = dec_level(dec_edc(v, s), lv.E[s]);
#pragma unroll
            for (int r = 0; r < DEC_RANGES; r++)
                if (L >= DEC_LO[r] && L <= DEC_HI[r]) {
                    cnt[3 * s + r] += 1.0;
                    first[3 * s + r] = fmin(first[3 * s + r], (double)m);
                }
        }
    }
    double* mine = part + (uint64_t)DEC_MEMBER_PART * blockIdx.x;
    for (int f = 0; f < DEC_FITS; f++) {
        const double c = ish_block_reduce(cnt[f], red, [](double p, double q) { return p + q; });
        const double a = ish_block_reduce(first[f], red, [](double p, double q) { return fmin(p, q); });
        if (threadIdx.x == 0) mine[f] = c, mine[DEC_FITS + f] = a;
    }
    for (int k = 0; k < 2; k++) {
        const double r = ish_block_reduce(sum[k], red, [](double p, double q) { return p + q; });
        if (threadIdx.x == 0) mine[2 * DEC_FITS + k] = r;
    }
}

// part[DEC_FIT_PART b + 4 f ..] = workgroup b's share of sum x, sum y, sum x^2, sum x y over the taps of fit f, x = m - first[f],
// y = L[m]
__global__ __launch_bounds__(ISH_THREADS) void k_dec_fit(const double2* __restrict__ buf, uint64_t o, uint64_t n, DecLevels lv,
                                                         double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t stride = (uint64_t)gridDim.x * ISH_THREADS;
    double acc[DEC_FIT_PART];
    for (int k = 0; k < DEC_FIT_PART; k++) acc[k] = 0.0;
    for (uint64_t m = o + (uint64_t)blockIdx.x * ISH_THREADS + threadIdx.x; m < n; m += stride) {
        const double2 v = buf[m];
#pragma unroll
        for (int s = 0; s < DEC_SETS; s++) {
            const double L = dec_level(dec_edc(v, s), lv.E[s]);
#pragma unroll
            for (int r = 0; r < DEC_RANGES; r++)
                if (L >= DEC_LO[r] && L <= DEC_HI[r]) {
                    const int f = 3 * s + r;
                    const double x = (double)m - (double)lv.first[f];
                    acc[4 * f] += x;
                    acc[4 * f + 1] += L;
                    acc[4 * f + 2] += x * x;
                    acc[4 * f + 3] += x * L;
                }
        }
    }
    for (int k = 0; k < DEC_FIT_PART; k++) {
        const double r = ish_block_reduce(acc[k], red, [](double p, double q) { return p + q; });
        if (threadIdx.x == 0) part[(uint64_t)DEC_FIT_PART * blockIdx.x + k] = r;
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// What the queries of the measurements (this header, irfloor, irdensity, iriacc, irsti and irresponse) have in common.  The three checks write
// their message into the caller's buffer msg [cap] and return false; true and nothing written when the field is good.
inline bool dec_rate_ok(uint32_t rate, char* msg, size_t cap) {
    if (rate >= DEC_MIN_RATE && rate <= DEC_MAX_RATE) return true;
    std::snprintf(msg, cap, "rate %u outside [%u, %u]", rate, DEC_MIN_RATE, DEC_MAX_RATE);
    return false;
}
inline bool dec_onset_ok(float onset_db, char* msg, size_t cap) {
    const double on = (double)onset_db;
    if (on >= DEC_MIN_ONSET_DB && on <= 0.0) return true;
    std::snprintf(msg, cap, "onset_db %g outside [%g, 0]", on, DEC_MIN_ONSET_DB);
    return false;
}
// the n_bands (checked) centre frequencies at a checked rate, then the Q they share
inline bool dec_bands_ok(const float* centre_hz, uint32_t n_bands, float q, uint32_t rate, char* msg, size_t cap) {
    const double top = IEQ_MAX_NYQ * (double)rate, qq = (double)q;
    for (uint32_t b = 0; b < n_bands; b++) {
        const double f = (double)centre_hz[b];
        if (std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top) continue;
        std::snprintf(msg, cap, "centre_hz[%u] %g outside [%g, %g]", b, f, IEQ_MIN_HZ, top);
        return false;
    }
    if (std::isfinite(qq) && qq >= IEQ_MIN_Q && qq <= IEQ_MAX_Q) return true;
    std::snprintf(msg, cap, "q %g outside [%g, %g]", qq, IEQ_MIN_Q, IEQ_MAX_Q);
    return false;
}
// N, the taps a query analyses of n stored ones: all of them with end = 0
inline uint64_t dec_span(uint64_t end, uint64_t n) { return end ? std::min<uint64_t>(end, n) : n; }

// Every field of a query, checked without touching an engine or HIP; the message (thread-local) names the field.  Null when it
// is good.
inline const char* dec_check(const mc_decay_query* q) {
    static thread_local char msg[160];
    if (!q) return "null query";
    if (q->struct_size != sizeof(mc_decay_query)) return "mc_decay_query struct_size mismatch";
    if (!dec_rate_ok(q->rate, msg, sizeof(msg))) return msg;
    if (q->n_bands > MC_DECAY_MAX_BANDS)
        std::snprintf(msg, sizeof(msg), "n_bands %u above %d", q->n_bands, MC_DECAY_MAX_BANDS);
    else if (q->curve_points == 1 || q->curve_points > MC_DECAY_MAX_CURVE)
        std::snprintf(msg, sizeof(msg), "curve_points %u is neither 0 nor in [2, %d]", q->curve_points, MC_DECAY_MAX_CURVE);
    else if (dec_bands_ok(q->centre_hz, q->n_bands, q->q, q->rate, msg, sizeof(msg)) && dec_onset_ok(q->onset_db, msg, sizeof(msg)))
        return nullptr;
    return msg;
}

// one section of a band: the Audio-EQ-Cookbook band-pass with 0 dB peak gain, w0, c and al as ieq_coef has them
inline IeqCoef dec_coef(float centre_hz, float q, uint32_t rate) {
    const double w0 = 2.0 * M_PI * (double)centre_hz / (double)rate, c = std::cos(w0), al = std::sin(w0) / (2.0 * (double)q);
    const double a0 = 1.0 + al;
    return IeqCoef{al / a0, 0.0, -al / a0, -2.0 * c / a0, (1.0 - al) / a0};
}

// The eight numbers of a row and its K curve points from what the kernels reduced: pick = EDC of the set at o, N - 1, k50,
// k80 and the curve's points; cnt / first / fit = the three ranges' member counts, first taps and four sums; tsum = sum EDC
// over (o, N).
inline void dec_row(const double* pick, const double* cnt, const double (*fit)[4], double tsum, uint64_t o, uint64_t N, uint64_t k50,
                    uint64_t k80, uint32_t rate, uint32_t K, double* row, double* curve) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double E = pick[0];
    row[0] = E;
    for (int k = 1; k < 8; k++) row[k] = nan;
    for (uint32_t j = 0; j < K; j++) curve[j] = nan;
    if (!(E > 0.0)) return;  // (an all-zero row, or taps that are not numbers)
    const double Llast = 10.0 * std::log10(pick[1] / E);
    for (int r = 0; r < DEC_RANGES; r++) {
        const double n = cnt[r];
        if (Llast > DEC_LO[r] || n < 2.0) continue;
        const double sx = fit[r][0], sy = fit[r][1], sxx = fit[r][2], sxy = fit[r][3];
        const double a = (n * sxy - sx * sy) / (n * sxx - sx * sx);
        row[1 + r] = -60.0 / (a * (double)rate);
    }
    const uint64_t kk[2] = {k50, k80};
    for (int k = 0; k < 2; k++) {
        const double late = pick[2 + k];
        if (kk[k] >= N || late == 0.0) continue;
        row[4 + k] = 10.0 * std::log10((E - late) / late);
        if (k == 0) row[6] = (E - late) / E;
    }
    row[7] = tsum / E / (double)rate;
    for (uint32_t j = 0; j < K; j++) curve[j] = std::max(10.0 * std::log10(pick[DEC_PICK_HEAD + j] / E), DEC_CURVE_FLOOR);
}

// workgroups of the origin's two walks over N taps
inline unsigned dec_origin_grid(uint64_t N) { return (unsigned)std::min<uint64_t>(ISH_SCAN_GRID, (N / 2 + ISH_THREADS) / ISH_THREADS); }

// *o = the origin of taps [0, N) of d_x (mc_ir_decay's step 1): the shaped load's onset search, 0 with onset_db = 0 and for taps
// that compare false with everything.  d_part: 8 bytes per workgroup of dec_origin_grid(N).  Synchronises the stream.
inline hipError_t dec_origin(hipStream_t stream, const float2* d_x, uint64_t N, float onset_db, void* d_part, uint64_t* o) {
    *o = 0;
    if (!(onset_db < 0.f)) return hipSuccess;
    const unsigned ogrid = dec_origin_grid(N);
    hipLaunchKernelGGL(k_shape_peak, dim3(ogrid), dim3(ISH_THREADS), 0, stream, d_x, N, (float*)d_part);
    hipError_t er = hipGetLastError();
    std::vector<float> pk(ogrid);
    if (er == hipSuccess) er = hipMemcpyAsync(pk.data(), d_part, sizeof(float) * ogrid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    if (er != hipSuccess) return er;
    float peak = 0.f;
    for (float v : pk) peak = std::max(peak, v);
    const float t = peak * (float)std::pow(10.0, (double)onset_db / 20.0);
    hipLaunchKernelGGL(k_shape_onset, dim3(ogrid), dim3(ISH_THREADS), 0, stream, d_x, N, t, (unsigned long long*)d_part);
    er = hipGetLastError();
    std::vector<unsigned long long> at(ogrid);
    if (er == hipSuccess) er = hipMemcpyAsync(at.data(), d_part, sizeof(unsigned long long) * ogrid, hipMemcpyDeviceToHost, stream);
    if (er == hipSuccess) er = hipStreamSynchronize(stream);
    if (er != hipSuccess) return er;
    uint64_t onset = ISH_NONE;
    for (unsigned long long v : at) onset = std::min<uint64_t>(onset, v);
    *o = onset == ISH_NONE ? 0 : onset;
    return hipSuccess;
}

// The host side of a measurement: what dec_measure here and flr_measure, den_measure, iacc_measure, sti_measure and rsp_measure
// (irfloor, irdensity, iriacc, irsti, irresponse.hip.h) do around their own kernels.  It lives in this host section, not in a header of its own, because
// it needs this header's kernels and those four include this header already.  A *_measure constructs it (the span N and the chunk
// geometry), opens it (the scratch and the origin o) and strings its own launches between the operations below; every one of them
// does nothing once `er` is set, so a *_measure tests m.er where it has to stop.  The scratch goes when the struct goes: nothing
// stays allocated on any path.
struct Measure {
    hipStream_t stream;
    const float2* d_x;
    uint64_t N, o = 0;                           // the taps analysed are [0, N); the origin among them
    ChunkGeom cg;                                // k_eq_chunk, k_dec_sum and the carries over N taps
    hipError_t er = hipSuccess;
    DevArray<double2> d_buf, d_st;         // a row group's doubles [N]; the chunk states
    DevArray<double> d_tot, d_part, d_fin;  // the chunk totals [cg.lanes]; partials; folded sums

    Measure(hipStream_t stream, const float2* d_x, uint64_t n, uint64_t end) : stream(stream), d_x(d_x), N(dec_span(end, n)), cg(chunk_geom(N)) {}
    template <class T>
    void alloc(DevArray<T>& a, size_t count) {
        if (er == hipSuccess && count) er = a.alloc(count);
    }
    // The scratch, each buffer with the elements the measurement names (0: none; d_part holds the origin's partials at least),
    // then the origin (mc_ir_decay's step 1).  Synchronises the stream when onset_db < 0.  st0: what d_st starts as, nst double2
    // of the host that go onto the stream ahead of the origin's kernels (mc_ir_density's table); the caller keeps them until the
    // stream has run dry.
    void open(float onset_db, size_t nbuf, size_t nst, size_t ntot, size_t npart, size_t nfin, const double2* st0 = nullptr) {
        alloc(d_buf, nbuf), alloc(d_st, nst), alloc(d_tot, ntot), alloc(d_part, std::max<size_t>(npart, dec_origin_grid(N))), alloc(d_fin, nfin);
        if (er == hipSuccess && st0) er = hipMemcpyAsync(d_st, st0, sizeof(double2) * nst, hipMemcpyHostToDevice, stream);
        if (er == hipSuccess) er = dec_origin(stream, d_x, N, onset_db, d_part, &o);
    }
    // d_part [count] at least: what it held is dropped (grow waits for the stream before it frees: the wait hipFree implied, now said)
    void grow_part(size_t count) {
        if (er == hipSuccess) er = d_part.grow(count, stream);
    }
    void launched() { er = hipGetLastError(); }
    // dst = src [bytes] of the device, and the stream has run dry
    void fetch(void* dst, const void* src, size_t bytes) {
        if (er == hipSuccess) er = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
        if (er == hipSuccess) er = hipStreamSynchronize(stream);
    }
    // d_buf [N] = a row group's doubles (mc_ir_decay's step 2): the taps as double and, with centre_hz, run through that band's two
    // identical sections, the second riding as the `nxt` stage of the first's fix-up.  d_st: double2 [cg.lanes].
    void group(const float* centre_hz, float q, uint32_t rate) {
        if (er != hipSuccess) return;
        hipLaunchKernelGGL(k_dec_fill, dim3((unsigned)((N + ISH_THREADS - 1) / ISH_THREADS)), dim3(ISH_THREADS), 0, stream, d_x, N, d_buf);
        launched();
        if (!centre_hz) return;
        IeqStage sec{}, off{};
        sec.c = dec_coef(*centre_hz, q, rate), sec.on = 1;
        const IeqCarry cm = ieq_carry(sec.c, cg.K);
        for (int pass = 0; pass < 3 && er == hipSuccess; pass++) {
            if (pass > 0) {
                hipLaunchKernelGGL(k_eq_carry, dim3(1), dim3(2 * IEQ_RUNS), 0, stream, d_st, cg.nchunks, cg.K, cm.M, cm.MK);
                launched();
            }
            if (er != hipSuccess) break;
            hipLaunchKernelGGL(k_eq_chunk, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, N, pass > 0 ? sec : off, pass < 2 ? sec : off, d_st);
            launched();
        }
    }
    // d_buf = EDC, the backward sum over [o, N) (the file's head).  d_tot: double [cg.lanes].
    void edc() {
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_dec_sum<false>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, o, N, d_tot);
            launched();
        }
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_dec_carry, dim3(1), dim3(DEC_CARRY_THREADS), 0, stream, d_tot, cg.nchunks);
            launched();
        }
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_dec_sum<true>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, d_buf, o, N, d_tot);
            launched();
        }
    }
    void info(uint64_t out[2]) const { out[0] = o, out[1] = N; }
};

// The whole measurement of the n stored taps d_x for a checked query.  rows, curve, info as mc_ir_decay describes them.
// Synchronises the stream; leaves nothing allocated.
inline hipError_t dec_measure(hipStream_t stream, const float2* d_x, uint64_t n, const mc_decay_query& q, double* rows, double* curve,
                              uint64_t info[2]) {
    Measure m(stream, d_x, n, q.end);
    const uint64_t N = m.N;
    const uint32_t K = q.curve_points, npick = DEC_PICK_HEAD + K;
    const unsigned rgrid = std::min<unsigned>(DEC_GRID, (unsigned)((N + ISH_THREADS - 1) / ISH_THREADS));  // k_dec_members, k_dec_fit
    // (a vector of this function's own, not a member of m: the loops over it below vectorise only while its address stays here)
    std::vector<double> part(std::max<size_t>((size_t)DEC_FIT_PART * rgrid, (size_t)2 * npick));
    m.open(q.onset_db, N, m.cg.lanes, m.cg.lanes, part.size(), 0);
    const uint64_t o = m.o;
    const uint64_t k50 = o + (uint64_t)std::floor(0.05 * (double)q.rate + 0.5), k80 = o + (uint64_t)std::floor(0.08 * (double)q.rate + 0.5);

    for (uint32_t g = 0; g <= q.n_bands && m.er == hipSuccess; g++) {
        m.group(g ? &q.centre_hz[g - 1] : nullptr, q.q, q.rate);
        m.edc();
        if (m.er == hipSuccess) {
            hipLaunchKernelGGL(k_dec_pick, dim3((npick + ISH_THREADS - 1) / ISH_THREADS), dim3(ISH_THREADS), 0, stream, m.d_buf, o, N, k50, k80, K,
                               reinterpret_cast<double2*>(m.d_part.get()));
            m.launched();
        }
        m.fetch(part.data(), m.d_part, sizeof(double) * 2 * npick);
        if (m.er != hipSuccess) break;
        std::vector<double> pick[DEC_SETS];
        for (int s = 0; s < DEC_SETS; s++) {
            pick[s].resize(npick);
            for (uint32_t j = 0; j < npick; j++) pick[s][j] = s == 0 ? part[2 * j] : (s == 1 ? part[2 * j + 1] : part[2 * j] + part[2 * j + 1]);
        }
        DecLevels lv{};
        for (int s = 0; s < DEC_SETS; s++) lv.E[s] = pick[s][0];
        hipLaunchKernelGGL(k_dec_members, dim3(rgrid), dim3(ISH_THREADS), 0, stream, m.d_buf, o, N, lv, m.d_part);
        m.launched();
        m.fetch(part.data(), m.d_part, sizeof(double) * DEC_MEMBER_PART * rgrid);
        if (m.er != hipSuccess) break;
        double cnt[DEC_FITS], tsum[DEC_SETS] = {0.0, 0.0, 0.0};
        for (int f = 0; f < DEC_FITS; f++) cnt[f] = 0.0, lv.first[f] = N;
        for (unsigned b = 0; b < rgrid; b++) {
            const double* p = part.data() + (size_t)DEC_MEMBER_PART * b;
            for (int f = 0; f < DEC_FITS; f++) {
                cnt[f] += p[f];
                lv.first[f] = std::min<uint64_t>(lv.first[f], (uint64_t)p[DEC_FITS + f]);
            }
            tsum[0] += p[2 * DEC_FITS];
            tsum[1] += p[2 * DEC_FITS + 1];
        }
        tsum[2] = tsum[0] + tsum[1];
        hipLaunchKernelGGL(k_dec_fit, dim3(rgrid), dim3(ISH_THREADS), 0, stream, m.d_buf, o, N, lv, m.d_part);
        m.launched();
        m.fetch(part.data(), m.d_part, sizeof(double) * DEC_FIT_PART * rgrid);
        if (m.er != hipSuccess) break;
        double fit[DEC_FITS][4] = {};
        for (unsigned b = 0; b < rgrid; b++)
            for (int f = 0; f < DEC_FITS; f++)
                for (int k = 0; k < 4; k++) fit[f][k] += part[(size_t)DEC_FIT_PART * b + 4 * f + k];
        for (int s = 0; s < DEC_SETS; s++) {
            const size_t r = (size_t)g * DEC_SETS + s;
            dec_row(pick[s].data(), cnt + 3 * s, fit + 3 * s, tsum[s], o, N, k50, k80, q.rate, K, rows + 8 * r, curve ? curve + (size_t)K * r : nullptr);
        }
    }
    m.info(info);
    return m.er;
}
