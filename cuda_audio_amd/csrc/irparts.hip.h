// irparts.hip.h — the parts step of an impulse-response load (mc_load_ir_parts, mc_load_ir_sweep_parts): the F frames are split
// into the direct sound, the early reflections and the late tail by two boundaries with raised-cosine cross-fades, and each
// part gets a gain, a delay in whole frames, a stereo width and a balance of its own, and may be muted, inverted or have its
// channels exchanged.  No reference equivalent.  Step 1e of the shaped load (include/mcconv.h has the definition, DESIGN.md
// 2.22 the reasons): shape_stage runs parts_run on the F frames that the source and the steps 1a to 1d left and hands
// irshape.hip.h the Fo frames it makes.  tests/ir_parts_np.py states the same in float64, one channel pair at a time.
//
// Weights of input frame m, s_k = b_k - floor(x_k / 2):
//   u_k(m) = 0 for m < s_k, 1 for m >= s_k + x_k, else (1 - cos(pi (m - s_k + 1) / (x_k + 1))) / 2;
//   w_0 = 1 - u_0, w_1 = u_0 - u_1, w_2 = u_1.
// Output frame n, parts in the order 0, 1, 2, everything in double: m = n - delay_p, used when 0 <= m < F and w_p(m) > 0;
//   t = w_p(m) x[m]; acc_L += fma(c_LR, t_R, c_LL t_L); acc_R += fma(c_RL, t_L, c_RR t_R); the frame is (float) acc.
// The 12 coefficients come from the host (parts_step), made there in double; the kernels see numbers only.
//
// Two kernels, 256 lanes per workgroup, grids that depend on F and Fo alone: k_pt_mix (one lane per output frame: up to three
// shifted reads of float2, which a wave makes from consecutive addresses, one store, and the stored energy) and k_pt_energy
// (one lane per input frame: the parts' weighted energies and what falls outside [0, Fo)).  Both call pt_weight.  Every
// reduction ends in one partial per workgroup, which always covers the same 256 frames, added on the host in index order
// (as irfilter.hip.h does): no atomics, and the same frames and struct give the same bits.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>

#include "irspectral.hip.h"

constexpr int PT_THREADS = ISH_THREADS;
constexpr int PT_PARTS = 3;
constexpr uint64_t PT_MAX_BOUNDARY = 1ull << 40;  // b_0, b_1
constexpr int32_t PT_MAX_DELAY = 1 << 24;         // |delay_p|, and what frames_out may add to F
constexpr uint32_t PT_FLAG_BITS = 0x777u;         // mute, swap, invert of the three parts

// a checked mc_ir_parts that is on, over F frames: what the kernels take by value
struct PartsStep {
    uint64_t F, Fo;
    uint64_t s[2];          // where the cross-fades begin
    uint32_t x[2];          // their lengths
    int32_t delay[PT_PARTS];
    uint32_t mute;          // bit p: part p contributes nothing
    double c[PT_PARTS][4];  // c_LL, c_LR, c_RL, c_RR
    uint64_t b[2];          // the boundaries clamped to F (mc_ir_parts_info)
};

// u_k(m) of the cross-fade that begins at s and is x frames long
__device__ inline double pt_fade(uint64_t m, uint64_t s, uint32_t x) {
    if (m < s) return 0.0;
    if (m - s >= (uint64_t)x) return 1.0;
    return 0.5 * (1.0 - cos(M_PI * (double)(m - s + 1) / ((double)x + 1.0)));
}

// w_p(m)
__device__ inline double pt_weight(const PartsStep& st, int p, uint64_t m) {
    if (p == 0) return 1.0 - pt_fade(m, st.s[0], st.x[0]);
    if (p == 2) return pt_fade(m, st.s[1], st.x[1]);
    return pt_fade(m, st.s[0], st.x[0]) - pt_fade(m, st.s[1], st.x[1]);
}

// y[n] for n < Fo; part[b] = the workgroup's energy as stored.
__global__ __launch_bounds__(PT_THREADS) void k_pt_mix(const float2* __restrict__ x, PartsStep st, float2* __restrict__ y, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t n = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    double kept = 0.0;
    if (n < st.Fo) {
        double accl = 0.0, accr = 0.0;
#pragma unroll
        for (int p = 0; p < PT_PARTS; p++) {
            if (st.mute >> p & 1) continue;
            const int64_t m = (int64_t)n - (int64_t)st.delay[p];
            if (m < 0 || (uint64_t)m >= st.F) continue;
            const double w = pt_weight(st, p, (uint64_t)m);
            if (!(w > 0.0)) continue;
            const float2 f = x[m];
            const double tl = w * (double)f.x, tr = w * (double)f.y;
            accl += fma(st.c[p][1], tr, st.c[p][0] * tl);
            accr += fma(st.c[p][2], tl, st.c[p][3] * tr);
        }
        const float2 f = make_float2((float)accl, (float)accr);
        y[n] = f;
        kept = (double)f.x * (double)f.x + (double)f.y * (double)f.y;
    }
    const double s = ish_block_reduce(kept, red, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Lane m < F.  part[5 b + p] = the workgroup's sum of w_p^2 (x_L^2 + x_R^2), muted parts too; part[5 b + 3] = that sum over the
// contributions of parts that are not muted which land outside [0, Fo), part[5 b + 4] = their count, as a double.
__global__ __launch_bounds__(PT_THREADS) void k_pt_energy(const float2* __restrict__ x, PartsStep st, double* __restrict__ part) {
    __shared__ double red[ISH_WAVES];
    const uint64_t m = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < st.F) {
        const float2 f = x[m];
        const double e = (double)f.x * (double)f.x + (double)f.y * (double)f.y;
#pragma unroll
        for (int p = 0; p < PT_PARTS; p++) {
            const double w = pt_weight(st, p, m);
            if (!(w > 0.0)) continue;
            v[p] = w * w * e;
            const int64_t n = (int64_t)m + (int64_t)st.delay[p];
            if (!(st.mute >> p & 1) && (n < 0 || (uint64_t)n >= st.Fo)) v[3] += v[p], v[4] += 1.0;
        }
    }
    const auto add = [](double a, double b) { return a + b; };
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const double s = ish_block_reduce(v[k], red, add);
        if (threadIdx.x == 0) part[5 * (uint64_t)blockIdx.x + k] = s;
    }
}

// -- host ------------------------------------------------------------------------------------------------------------
// Every field of a parts step that is on but frames_out, in the struct's order, checked without touching an engine or HIP; the
// message (thread-local) names the field.  Null when it is good.
inline const char* parts_check(const mc_ir_parts* p) {
    static thread_local char msg[200];
    static const char* const part[PT_PARTS] = {"direct", "early", "late"};
    if (p->struct_size != sizeof(mc_ir_parts)) return "mc_ir_parts struct_size mismatch";
    if (p->mode > MC_PARTS_ON) {
        std::snprintf(msg, sizeof(msg), "the parts' mode %u is not an MC_PARTS_OFF / ON value", p->mode);
        return msg;
    }
    if (p->flags & ~PT_FLAG_BITS) {
        std::snprintf(msg, sizeof(msg), "the parts' flags 0x%x hold bits outside 0x%x", p->flags, PT_FLAG_BITS);
        return msg;
    }
    if (p->reserved0) {
        std::snprintf(msg, sizeof(msg), "the parts' reserved0 word is %u, not 0", p->reserved0);
        return msg;
    }
    if (p->direct_end > PT_MAX_BOUNDARY) {
        std::snprintf(msg, sizeof(msg), "direct_end %llu above 2^40", (unsigned long long)p->direct_end);
        return msg;
    }
    if (p->early_end > PT_MAX_BOUNDARY || p->early_end < p->direct_end) {
        std::snprintf(msg, sizeof(msg), "early_end %llu outside [direct_end = %llu, 2^40]", (unsigned long long)p->early_end, (unsigned long long)p->direct_end);
        return msg;
    }
    const int64_t s0 = (int64_t)p->direct_end - (int64_t)(p->xfade[0] / 2), s1 = (int64_t)p->early_end - (int64_t)(p->xfade[1] / 2);
    if (s0 < 0) {
        std::snprintf(msg, sizeof(msg), "xfade[0] %u begins before frame 0: direct_end %llu is below half of it", p->xfade[0], (unsigned long long)p->direct_end);
        return msg;
    }
    if (s0 + (int64_t)p->xfade[0] > s1) {
        std::snprintf(msg, sizeof(msg), "xfade[1] %u begins at frame %lld, before xfade[0] %u ends at frame %lld", p->xfade[1], (long long)s1, p->xfade[0],
                      (long long)(s0 + (int64_t)p->xfade[0]));
        return msg;
    }
    for (int k = 0; k < PT_PARTS; k++)
        if (p->delay[k] < -PT_MAX_DELAY || p->delay[k] > PT_MAX_DELAY) {
            std::snprintf(msg, sizeof(msg), "delay[%d] %d (%s) outside [-2^24, 2^24]", k, p->delay[k], part[k]);
            return msg;
        }
    for (int k = 0; k < PT_PARTS; k++)
        if (!(p->gain_db[k] >= -120.f && p->gain_db[k] <= 24.f)) {
            std::snprintf(msg, sizeof(msg), "gain_db[%d] %g (%s) outside [-120, 24]", k, (double)p->gain_db[k], part[k]);
            return msg;
        }
    for (int k = 0; k < PT_PARTS; k++)
        if (!(p->width[k] >= 0.f && p->width[k] <= 2.f)) {
            std::snprintf(msg, sizeof(msg), "width[%d] %g (%s) outside [0, 2]", k, (double)p->width[k], part[k]);
            return msg;
        }
    for (int k = 0; k < PT_PARTS; k++)
        if (!(p->balance[k] >= -1.f && p->balance[k] <= 1.f)) {
            std::snprintf(msg, sizeof(msg), "balance[%d] %g (%s) outside [-1, 1]", k, (double)p->balance[k], part[k]);
            return msg;
        }
    if (p->reserved[0] || p->reserved[1]) {
        std::snprintf(msg, sizeof(msg), "the parts' reserved words are %u, %u, not 0", p->reserved[0], p->reserved[1]);
        return msg;
    }
    return nullptr;
}

// a checked parts step that is on, over F frames; Fo = 0 when no part that is not muted holds a frame or nothing of them
// lands at or after frame 0 (parts_check_frames refuses that)
inline PartsStep parts_step(const mc_ir_parts& p, uint64_t F) {
    PartsStep st{};
    st.F = F;
    for (int k = 0; k < 2; k++) {
        const uint64_t b = k ? p.early_end : p.direct_end;
        st.x[k] = p.xfade[k], st.s[k] = b - p.xfade[k] / 2, st.b[k] = std::min(b, F);
    }
    st.mute = p.flags & 7u;
    for (int k = 0; k < PT_PARTS; k++) {
        st.delay[k] = p.delay[k];
        const double g = std::pow(10.0, (double)p.gain_db[k] / 20.0) * (p.flags >> (8 + k) & 1 ? -1.0 : 1.0);
        const double w = (double)p.width[k], bal = (double)p.balance[k];
        const double a = (1.0 + w) / 2.0, b = (1.0 - w) / 2.0, gl = bal > 0.0 ? 1.0 - bal : 1.0, gr = bal < 0.0 ? 1.0 + bal : 1.0;
        double c[4] = {g * gl * a, g * gl * b, g * gr * b, g * gr * a};
        if (p.flags >> (4 + k) & 1) std::swap(c[0], c[1]), std::swap(c[2], c[3]);  // (the input's channels change places)
        std::copy(c, c + 4, st.c[k]);
    }
    // where each part's support inside [0, F) begins and ends
    const uint64_t lo[PT_PARTS] = {0, st.s[0], st.s[1]};
    const uint64_t hi[PT_PARTS] = {std::min(F, st.s[0] + st.x[0]), std::min(F, st.s[1] + st.x[1]), F};
    int64_t most = 0;
    for (int k = 0; k < PT_PARTS; k++)
        if (!(st.mute >> k & 1) && lo[k] < hi[k]) most = std::max(most, (int64_t)hi[k] + (int64_t)st.delay[k]);
    st.Fo = p.frames_out ? p.frames_out : (uint64_t)most;
    return st;
}

// the limits of a checked parts step over F frames at the session's rate (F = 0 is the load's own "empty IR"): frames_out
// within [1, F + 2^24], and a part that is neither muted nor empty whose frames reach frame 0 or later
inline const char* parts_check_frames(const mc_ir_parts* p, uint64_t F) {
    static thread_local char msg[200];
    if (!F) return nullptr;
    if (p->frames_out > F + (uint64_t)PT_MAX_DELAY) {
        std::snprintf(msg, sizeof(msg), "the parts' frames_out %llu above %llu frames + 2^24", (unsigned long long)p->frames_out, (unsigned long long)F);
        return msg;
    }
    mc_ir_parts at = *p;
    at.frames_out = 0;
    if (!parts_step(at, F).Fo) {
        std::snprintf(msg, sizeof(msg), "every part is muted, empty or delayed to before frame 0: the parts leave no frame of %llu", (unsigned long long)F);
        return msg;
    }
    return nullptr;
}

// what parts_run allocates on the device while it runs: the partials
inline uint64_t parts_device_bytes(const PartsStep& s) { return 8 * std::max(spec_groups(s.Fo), 5 * spec_groups(s.F)); }

// Step 1e: the s.Fo frames d_y from the s.F frames d_x, on the stream, after what the stream already holds.  Allocates the
// partials, waits for the kernels and frees them.  info = mc_ir_parts_info's ten numbers.
inline hipError_t parts_run(hipStream_t stream, const float2* d_x, float2* d_y, const PartsStep& s, double info[10]) {
    const uint64_t gF = spec_groups(s.F), gO = spec_groups(s.Fo), count = std::max(gO, 5 * gF);
    DevArray<double> d_part;
    std::vector<double> part(count);
    hipError_t er = d_part.alloc(count);
    const auto fetch = [&](uint64_t n) {
        hipError_t e2 = hipGetLastError();
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(part.data(), d_part, sizeof(double) * n, hipMemcpyDeviceToHost, stream);
        return e2 == hipSuccess ? hipStreamSynchronize(stream) : e2;
    };
    double E[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, Eout = 0.0;
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_pt_energy, dim3((unsigned)gF), dim3(PT_THREADS), 0, stream, d_x, s, d_part);
        er = fetch(5 * gF);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gF; b++)
            for (int k = 0; k < 5; k++) E[k] += part[5 * b + k];
        hipLaunchKernelGGL(k_pt_mix, dim3((unsigned)gO), dim3(PT_THREADS), 0, stream, d_x, s, d_y, d_part);
        er = fetch(gO);
    }
    if (er == hipSuccess) {
        for (uint64_t b = 0; b < gO; b++) Eout += part[b];
        const double inf[10] = {(double)s.F, (double)s.Fo, (double)s.b[0], (double)s.b[1], E[0], E[1], E[2], Eout, E[3], E[4]};
        std::copy(inf, inf + 10, info);
    } else {
        (void)hipStreamSynchronize(stream);
    }
    return er;
}
