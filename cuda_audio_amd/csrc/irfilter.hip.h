// irfilter.hip.h — the filter step of an impulse-response load (mc_load_ir_filter, mc_load_ir_sweep_filter): the F frames are
// convolved with a second impulse response of G frames, or that one is divided out of them (Kirkeby's regularised inverse).
// No reference equivalent.  Step 1c of the shaped load (include/mcconv.h has the definition, DESIGN.md 2.20 the reasons):
// shape_stage runs filter_run on the F frames that the source, the tail step and the phase step left and hands irshape.hip.h
// the Fo frames it makes.  tests/ir_filter_np.py states the same with numpy's FFT, one channel at a time.  It is the second
// user of fft64.hip.h.
//
// Per output channel c, in double, Nfft = max(16, smallest power of two >= F + G - 1):
//   A = FFT(a_c padded), B = FFT(f_c padded); f_c = b_c (stereo), b_L (left) or (b_L + b_R) / 2 (mid);
//   convolve:    Y = A B;
//   deconvolve:  p = |B|^2, pm = max p, eps = 10^(-reg_db / 10), Y = A conj(B) / (p + eps pm); pm = 0 stores zeros;
//   y = Re IFFT(Y); the first Fo of y, rounded to float once.
//
// Both channels ride one complex transform (fft64.hip.h), as in irphase.hip.h: z_a = a_L + i a_R -> Z_a, and with a stereo filter
// z_b = b_L + i b_R -> Z_b; Y_L + i Y_R -> IFFT: Re is y_L, Im is y_R.  Two forward transforms and one inverse.
//
// The spectral kernels of a stereo filter (k_fl_mul_pair, k_fl_div_pair, and k_fl_power for its maxima) need the channels'
// own spectra, X_L[k] = (Z[k] + conj Z[N - k]) / 2 and X_R[k] = (Z[k] - conj Z[N - k]) / (2 i), of both transforms.  One lane
// owns the pair of bins (k, N - k), k = 0 .. N / 2: it reads Z_a and Z_b at both, makes the four spectra at k once, and writes
// Y[k] = Y_L[k] + i Y_R[k] and Y[N - k] = conj Y_L[k] + i conj Y_R[k] (Y_L and Y_R are spectra of real signals).  Chosen over
// one lane per bin because every value is then read once, not twice, and because the lane that reads a location is the only
// one that writes it, so the product is stored over Z_a and the step needs no third spectrum.  k = 0 and k = N / 2 are their own
// mirrors ((N - k) & (N - 1) == k): those two lanes write once, and count once where bins are counted.  The lanes of a wave
// read Z[N - k] in descending order, which still fills whole lines.
// With one real filter signal for both channels (left, mid) nothing is split: its spectrum B = Z_b multiplies Z_a bin by bin
// (k_fl_mul_mono, k_fl_div_mono, one lane per bin), since (A_L + i A_R) B = A_L B + i A_R B.
//
// Kernels apart from the transform's passes, 256 lanes per workgroup, grids that depend on F, G, Fo and Nfft alone: k_fl_pack
// (pad, map and pack either input, the energy that goes in), the product or k_fl_power and the quotient (which counts the
// regularised bins: the count needs the maximum, so it lives there and not with the maximum), k_fl_unpack (round, store, the
// energy stored and the energy of y[Fo .. Nfft) left behind).  Every reduction ends in one partial per workgroup, which always
// covers the same 256 elements, added on the host in index order (as irphase.hip.h does): no atomics, and the same frames,
// filter and struct give the same bits.
#pragma once
#include <cstdio>
#include <cstring>

#include "irspectral.hip.h"

constexpr int FL_MAX_LOG2 = F64_MAX_LOG2;  // Nfft <= 2^22
constexpr int FL_THREADS = ISH_THREADS;

// a checked mc_ir_filter that is on, over F frames and a filter of G frames, both at the session's rate
struct FilterStep {
    uint64_t F, G, Fo, Nfft;
    uint32_t op, channels;
    double reg_db;
    Fft64Plan fft;
    SecondIr second;  // where the filter's frames come from
};

// z[i] = the frame x[i] as double for i < n, zero up to N; map = MC_FILTER_STEREO: (L, R), _LEFT: (L, 0), _MID: ((L + R) / 2, 0).
// Workgroups that hold a frame: part[2 b], part[2 b + 1] = the sums of Re^2 and of Im^2 over their frames.
__global__ __launch_bounds__(FL_THREADS) void k_fl_pack(const float2* __restrict__ x, uint64_t n, uint64_t N, uint32_t map, double2* __restrict__ z,
                                                        double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    double2 v = make_double2(0.0, 0.0);
    if (i < n) {
        const float2 f = x[i];
        v = map == MC_FILTER_STEREO ? make_double2((double)f.x, (double)f.y)
            : map == MC_FILTER_LEFT ? make_double2((double)f.x, 0.0)
                                    : make_double2(0.5 * ((double)f.x + (double)f.y), 0.0);
    }
    if (i < N) z[i] = v;
    if ((uint64_t)blockIdx.x * FL_THREADS >= n) return;  // (the whole workgroup)
    const auto add = [](double p, double q) { return p + q; };
    const double s0 = ish_block_reduce(v.x * v.x, red, add), s1 = ish_block_reduce(v.y * v.y, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = s0;
        part[2 * (uint64_t)blockIdx.x + 1] = s1;
    }
}

__device__ inline double2 fl_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// a conj(b) / d
__device__ inline double2 fl_mul_conj_over(double2 a, double2 b, double d) {
    return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

// The pair (k, N - k) of Y = Y_L + i Y_R from the two real signals' bins at k; the lane of k = 0 and of k = N / 2 stores once.
__device__ inline void fl_store_pair(double2* __restrict__ Y, uint64_t k, uint64_t km, double2 yl, double2 yr) {
    Y[k] = make_double2(yl.x - yr.y, yl.y + yr.x);
    if (km != k) Y[km] = make_double2(yl.x + yr.y, yr.x - yl.y);
}

// Stereo filter, convolution.  Lane k <= N / 2: Za[k], Za[N - k] <- the pair of (A_L B_L) + i (A_R B_R).
__global__ __launch_bounds__(FL_THREADS) void k_fl_mul_pair(double2* __restrict__ Za, const double2* __restrict__ Zb, uint64_t N) {
    const uint64_t k = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    if (k > N / 2) return;
    const uint64_t km = (N - k) & (N - 1);
    double2 al, ar, bl, br;
    fl_split(Za[k], Za[km], al, ar);
    fl_split(Zb[k], Zb[km], bl, br);
    fl_store_pair(Za, k, km, fl_mul(al, bl), fl_mul(ar, br));
}

// One real filter signal, convolution.  Lane k < N: Za[k] <- Za[k] Zb[k].
__global__ __launch_bounds__(FL_THREADS) void k_fl_mul_mono(double2* __restrict__ Za, const double2* __restrict__ Zb, uint64_t N) {
    const uint64_t k = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    if (k < N) Za[k] = fl_mul(Za[k], Zb[k]);
}

// part[2 b], part[2 b + 1] = the workgroup's maxima of |B_L|^2 and |B_R|^2.  Stereo: lane k <= N / 2 (the power at N - k is
// that at k).  mono: lane k < N, B = Zb for both.
__global__ __launch_bounds__(FL_THREADS) void k_fl_power(const double2* __restrict__ Zb, uint64_t N, int mono, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t k = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    double pl = 0.0, pr = 0.0;
    if (mono) {
        if (k < N) {
            const double2 b = Zb[k];
            pl = pr = b.x * b.x + b.y * b.y;
        }
    } else if (k <= N / 2) {
        double2 bl, br;
        fl_split(Zb[k], Zb[(N - k) & (N - 1)], bl, br);
        pl = bl.x * bl.x + bl.y * bl.y, pr = br.x * br.x + br.y * br.y;
    }
    const auto mx = [](double a, double b) { return fmax(a, b); };
    const double m0 = ish_block_reduce(pl, red, mx), m1 = ish_block_reduce(pr, red, mx);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = m0;
        part[2 * (uint64_t)blockIdx.x + 1] = m1;
    }
}

// Stereo filter, deconvolution.  Lane k <= N / 2: Za[k], Za[N - k] <- the pair of Q_L + i Q_R, Q = A conj(B) / (|B|^2 + reg), zero
// for a channel that is off (pm = 0); thr = eps pm, the same number.  part[2 b], part[2 b + 1] = the workgroup's bins with
// |B|^2 < thr, as doubles (a pair counts twice, k = 0 and k = N / 2 once).
__global__ __launch_bounds__(FL_THREADS) void k_fl_div_pair(double2* __restrict__ Za, const double2* __restrict__ Zb, uint64_t N, double thr_l,
                                                            double thr_r, int on_l, int on_r, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t k = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    double nl = 0.0, nr = 0.0;
    if (k <= N / 2) {
        const uint64_t km = (N - k) & (N - 1);
        double2 al, ar, bl, br;
        fl_split(Za[k], Za[km], al, ar);
        fl_split(Zb[k], Zb[km], bl, br);
        const double pl = bl.x * bl.x + bl.y * bl.y, pr = br.x * br.x + br.y * br.y, both = km != k ? 2.0 : 1.0;
        nl = on_l && pl < thr_l ? both : 0.0, nr = on_r && pr < thr_r ? both : 0.0;
        const double2 zero = make_double2(0.0, 0.0);
        fl_store_pair(Za, k, km, on_l ? fl_mul_conj_over(al, bl, pl + thr_l) : zero, on_r ? fl_mul_conj_over(ar, br, pr + thr_r) : zero);
    }
    const auto add = [](double a, double b) { return a + b; };
    const double c0 = ish_block_reduce(nl, red, add), c1 = ish_block_reduce(nr, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = c0;
        part[2 * (uint64_t)blockIdx.x + 1] = c1;
    }
}

// One real filter signal, deconvolution.  Lane k < N: Za[k] <- Za[k] conj(Zb[k]) / (|Zb[k]|^2 + thr), zero when off;
// part[b] = the workgroup's bins with |Zb|^2 < thr, as a double.
__global__ __launch_bounds__(FL_THREADS) void k_fl_div_mono(double2* __restrict__ Za, const double2* __restrict__ Zb, uint64_t N, double thr, int on,
                                                            double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t k = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    double n = 0.0;
    if (k < N) {
        const double2 b = Zb[k];
        const double p = b.x * b.x + b.y * b.y;
        n = on && p < thr ? 1.0 : 0.0;
        Za[k] = on ? fl_mul_conj_over(Za[k], b, p + thr) : make_double2(0.0, 0.0);
    }
    const double c = ish_block_reduce(n, red, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

// y[m] = ((float) Re z[m], (float) Im z[m]) for m < Fo, zero for a channel that is off.  Lane m < N: part[2 b] = the
// workgroup's energy as stored (m < Fo), part[2 b + 1] = its energy of z left behind (Fo <= m < N).
__global__ __launch_bounds__(FL_THREADS) void k_fl_unpack(const double2* __restrict__ z, uint64_t Fo, uint64_t N, int on_l, int on_r,
                                                          float2* __restrict__ y, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t m = (uint64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    double kept = 0.0, rest = 0.0;
    if (m < N) {
        double2 v = z[m];
        if (!on_l) v.x = 0.0;
        if (!on_r) v.y = 0.0;
        if (m < Fo) {
            const float2 f = make_float2((float)v.x, (float)v.y);
            y[m] = f;
            kept = (double)f.x * (double)f.x + (double)f.y * (double)f.y;
        } else {
            rest = v.x * v.x + v.y * v.y;
        }
    }
    const auto add = [](double p, double q) { return p + q; };
    const double s0 = ish_block_reduce(kept, red, add), s1 = ish_block_reduce(rest, red, add);
    if (threadIdx.x == 0) {
        part[2 * (uint64_t)blockIdx.x] = s0;
        part[2 * (uint64_t)blockIdx.x + 1] = s1;
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a filter step that is on but frames_out, in the struct's order, checked without touching an engine or HIP; the
// message (thread-local) names the field.  Null when it is good.
inline const char* filter_check(const mc_ir_filter* f) {
    static thread_local char msg[160];
    if (f->struct_size != sizeof(mc_ir_filter)) return "mc_ir_filter struct_size mismatch";
    if (f->op > MC_FILTER_DECONVOLVE) {
        std::snprintf(msg, sizeof(msg), "op %u is not an MC_FILTER_OFF / CONVOLVE / DECONVOLVE value", f->op);
        return msg;
    }
    if (f->channels > MC_FILTER_MID) {
        std::snprintf(msg, sizeof(msg), "channels %u is not an MC_FILTER_STEREO / LEFT / MID value", f->channels);
        return msg;
    }
    if (f->rate && (f->rate < RS_MIN_RATE || f->rate > RS_MAX_RATE)) {
        std::snprintf(msg, sizeof(msg), "the filter's rate %u outside [%u, %u] (0 = the session's)", f->rate, RS_MIN_RATE, RS_MAX_RATE);
        return msg;
    }
    if (!(f->reg_db >= 20.f && f->reg_db <= 200.f)) {
        std::snprintf(msg, sizeof(msg), "reg_db %g outside [20, 200]", (double)f->reg_db);
        return msg;
    }
    if (f->reserved) {
        std::snprintf(msg, sizeof(msg), "the filter's reserved word is %u, not 0", f->reserved);
        return msg;
    }
    return nullptr;
}

// log2 of the transform of F + G - 1 points
inline int filter_log2(uint64_t F, uint64_t G) { return spec_ceil_log2(F + G - 1, F64_MIN_LOG2); }

// the limits of a checked filter step over F frames and G filter frames at the session's rate: G >= 1, Nfft <= 2^22, and
// frames_out within what the transform holds (F = 0 is the load's own "empty IR")
inline const char* filter_check_frames(const mc_ir_filter* f, uint64_t F, uint64_t G) {
    static thread_local char msg[240];
    if (!F) return nullptr;
    if (!G) return "empty filter: filter_frames is 0";
    if (F > (1ull << FL_MAX_LOG2) || G > (1ull << FL_MAX_LOG2) || F + G - 1 > (1ull << FL_MAX_LOG2)) {
        std::snprintf(msg, sizeof(msg), "%llu frames and %llu filter frames at the session's rate need a transform of more than 2^%d points",
                      (unsigned long long)F, (unsigned long long)G, FL_MAX_LOG2);
        return msg;
    }
    const uint64_t most = f->op == MC_FILTER_DECONVOLVE ? 1ull << filter_log2(F, G) : F + G - 1;
    if (f->frames_out > most) {
        std::snprintf(msg, sizeof(msg), "frames_out %llu above %llu, what %llu frames and %llu filter frames give a %s",
                      (unsigned long long)f->frames_out, (unsigned long long)most, (unsigned long long)F, (unsigned long long)G,
                      f->op == MC_FILTER_DECONVOLVE ? "deconvolution" : "convolution");
        return msg;
    }
    return nullptr;
}

// The limits of a checked filter step in a load whose F frames at the session's rate are known: a rate to convert from
// needs the session's, filter_frames at f's rate become *G at the session's, then filter_check_frames.
inline const char* filter_check_load(const mc_ir_filter* f, uint32_t session_rate, uint64_t F, uint64_t filter_frames, uint64_t* G) {
    static thread_local char msg[200];
    *G = 0;
    if (!F) return nullptr;
    if (f->rate && f->rate != session_rate && !session_rate) {
        std::snprintf(msg, sizeof(msg), "the filter's rate %u needs the session's rate to convert to, and session_rate is 0", f->rate);
        return msg;
    }
    if (filter_frames > (1ull << 40)) {
        std::snprintf(msg, sizeof(msg), "filter of %llu frames (filter_frames)", (unsigned long long)filter_frames);
        return msg;
    }
    *G = second_frames_at(f->rate, session_rate, filter_frames);
    return filter_check_frames(f, F, *G);
}

// a checked filter step that is on, over F frames and G filter frames within the limits (the source of the filter's frames
// is the caller's to fill in)
inline FilterStep filter_step(const mc_ir_filter& f, uint64_t F, uint64_t G) {
    const int lg = filter_log2(std::max<uint64_t>(F, 1), std::max<uint64_t>(G, 1));
    const uint64_t Fo = f.frames_out ? f.frames_out : f.op == MC_FILTER_DECONVOLVE ? F : F + G - 1;
    return FilterStep{F, G, Fo, 1ull << lg, f.op, f.channels, (double)f.reg_db, fft64_plan(lg), SecondIr{}};
}

// what filter_run allocates on the device while it runs: the filter's G frames, two buffers of Nfft double2, a third when the
// transform has two passes, and the partials (the resampler's own temporaries for a filter at another rate are not counted)
inline uint64_t filter_device_bytes(const FilterStep& s) { return 8 * s.G + spec_work_bytes(s.fft, s.Nfft); }

// Step 1c: the s.Fo frames d_y from the s.F frames d_x and the filter's host frames, on the stream, after what the stream
// already holds.  Allocates the work buffers (SpectralWork), waits for the kernels and frees them.  info = mc_ir_filter_info's ten numbers.
inline hipError_t filter_run(hipStream_t stream, const float2* d_x, float2* d_y, const FilterStep& s, double info[10]) {
    const uint64_t F = s.F, G = s.G, Fo = s.Fo, N = s.Nfft, gF = spec_groups(F), gG = spec_groups(G), gN = spec_groups(N);
    const uint64_t gH = spec_groups(N / 2 + 1);
    const bool mono = s.channels != MC_FILTER_STEREO;
    DevArray<float2> d_f;
    SpectralWork wk;
    hipError_t er = d_f.alloc(G);
    if (er == hipSuccess) er = wk.alloc(s.fft, N);
    if (er == hipSuccess) er = second_upload(stream, s.second, d_f, G);
    double2 *const d_a = wk.d_a, *const d_b = wk.d_b, *const d_w = wk.d_w;
    double* const d_part = wk.d_part;
    const std::vector<double>& part = wk.part;
    const auto fetch = [&](uint64_t count) { return wk.fetch(stream, count); };
    // A filter channel whose frames are all zero has pm = 0; the packed transform leaves rounding noise of the other channel in
    // its spectrum, so its energy before the transform decides (zero exactly when every frame is), not the maximum after it.
    double Ein = 0.0, Ef[2] = {0.0, 0.0}, Eout = 0.0, Erest = 0.0, pm[2] = {0.0, 0.0}, reg[2] = {0.0, 0.0};
    int on[2] = {1, 1};
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_fl_pack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, d_x, F, N, (uint32_t)MC_FILTER_STEREO, d_a, d_part);
        er = fetch(2 * gF);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < 2 * gF; b++) Ein += part[b];
        hipLaunchKernelGGL(k_fl_pack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, (const float2*)d_f, G, N, s.channels, d_b, d_part);
        er = fetch(2 * gG);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gG; b++) Ef[0] += part[2 * b], Ef[1] += part[2 * b + 1];
        if (mono) Ef[1] = Ef[0];  // (the one signal is both channels' filter)
        er = fft64_run(stream, s.fft, d_a, d_a, d_w, false);
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_b, d_b, d_w, false);
    if (er == hipSuccess && s.op == MC_FILTER_CONVOLVE) {
        if (mono)
            hipLaunchKernelGGL(k_fl_mul_mono, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, d_a, (const double2*)d_b, N);
        else
            hipLaunchKernelGGL(k_fl_mul_pair, dim3((unsigned)gH), dim3(FL_THREADS), 0, stream, d_a, (const double2*)d_b, N);
        er = hipGetLastError();
    }
    if (er == hipSuccess && s.op == MC_FILTER_DECONVOLVE) {
        const uint64_t g = mono ? gN : gH;
        hipLaunchKernelGGL(k_fl_power, dim3((unsigned)g), dim3(FL_THREADS), 0, stream, (const double2*)d_b, N, (int)mono, d_part);
        er = fetch(2 * g);
        if (er == hipSuccess) {
            for (uint64_t b = 0; b < g; b++) pm[0] = std::max(pm[0], part[2 * b]), pm[1] = std::max(pm[1], part[2 * b + 1]);
            const double eps = std::pow(10.0, -s.reg_db / 10.0);
            for (int c = 0; c < 2; c++) on[c] = Ef[c] > 0.0 && pm[c] > 0.0;
            if (mono)
                hipLaunchKernelGGL(k_fl_div_mono, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, d_a, (const double2*)d_b, N, eps * pm[0], on[0], d_part);
            else
                hipLaunchKernelGGL(k_fl_div_pair, dim3((unsigned)gH), dim3(FL_THREADS), 0, stream, d_a, (const double2*)d_b, N, eps * pm[0], eps * pm[1],
                                   on[0], on[1], d_part);
            er = fetch(mono ? gN : 2 * gH);
        }
        if (er == hipSuccess) {
            if (mono) {
                for (uint64_t b = 0; b < gN; b++) reg[0] += part[b];
                reg[1] = reg[0];
            } else {
                for (uint64_t b = 0; b < gH; b++) reg[0] += part[2 * b], reg[1] += part[2 * b + 1];
            }
        }
    }
    if (er == hipSuccess) er = fft64_run(stream, s.fft, d_a, d_a, d_w, true);
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_fl_unpack, dim3((unsigned)gN), dim3(FL_THREADS), 0, stream, (const double2*)d_a, Fo, N, on[0], on[1], d_y, d_part);
        er = fetch(2 * gN);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gN; b++) Eout += part[2 * b], Erest += part[2 * b + 1];
        const double inf[10] = {(double)F, (double)G, (double)Fo, (double)N, Ein, Ef[0] + Ef[1], Eout, Erest, reg[0], reg[1]};
        std::copy(inf, inf + 10, info);
    } else {
        (void)hipStreamSynchronize(stream);
    }
    return er;
}
