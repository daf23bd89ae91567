// irsynth.hip.h — synthesis of an impulse response on the device from a seed (mc_synth_ir): a decaying noise tail whose echo
// density builds up, a direct sound and a handful of early reflections.  No reference equivalent: the reference convolves with
// the frames of a WAV file.
//
// The F stereo frames are written straight into the buffer the shaping stage reads (irshape.hip.h); they never exist on the
// host.  Frame m is a pure function of (seed, m, the struct): no state runs from frame to frame, so the same struct gives the
// same bits whatever the grid.  include/mcconv.h has the definition and tests/ir_synth_np.py states it in float64:
//   W(i, s)      Philox4x32-10, counter {i, 0, s, 0}, key {seed lo, seed hi}; u(w) = (w + 0.5) / 2^32 as double (exact);
//   late field   m >= late_start, t = m - late_start: two Box-Muller normals from W(m, 0), the right one mixed from both by
//                rho = 1 - width; envelope late_gain * ish_tap's decay; with build_up = B > t + 1 the frame is occupied with
//                probability p = max(1/16, ((t + 1) / B)^2), decided by W(m, 1) in integer arithmetic, and scaled by 1 / sqrt(p);
//   direct       added to both channels of frame 0;
//   reflections  the host's table (syn_plan: position and the two gains of each, in double), added in table order.
// A frame is late + direct + reflections in double, rounded to float once.
//
// The work is arithmetic (two Philox blocks, two logs, two cosines and an exp2 per late frame, all in double), not traffic: 8
// bytes are stored per frame.  A thread makes two consecutive frames and stores them as one 16-byte store; the table is
// walked only by frames before its last position, so nearly every wave skips it.  No LDS, no atomics, no reductions: the peak
// and the sums are the shaping stage's.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/mcconv.h"
#include "irshape.hip.h"

constexpr int SYN_THREADS = 256;
constexpr uint64_t SYN_MAX_FRAMES = 1ull << 24;
constexpr uint32_t SYN_MAX_BUILD_UP = 65535;  // B^2 (t + 1)^2 stays inside 64 bits

// a checked mc_ir_synth as the kernel takes it
struct SynPlan {
    uint64_t F, late_start, t60;
    uint32_t key0, key1;
    uint32_t build_up;
    uint32_t n_early;    // reflections kept (pos < F), in ascending j
    uint32_t early_end;  // one past the last kept position; 0 with none
    double late_gain, direct, rho, rho_c;  // rho_c = sqrt(1 - rho^2)
    uint32_t pos[MC_SYNTH_MAX_EARLY];
    double gL[MC_SYNTH_MAX_EARLY], gR[MC_SYNTH_MAX_EARLY];
};

struct SynWords {
    uint32_t w0, w1, w2, w3;
};

__host__ __device__ inline uint32_t syn_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10 (Salmon et al., SC'11) of the counter {c0, c1, c2, c3} under the key {k0, k1}
__host__ __device__ inline SynWords syn_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = syn_mulhi(M0, c0), l0 = M0 * c0, h1 = syn_mulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    return SynWords{c0, c1, c2, c3};
}

// W(i, s) of the header
__host__ __device__ inline SynWords syn_words(const SynPlan& p, uint32_t i, uint32_t s) { return syn_philox(i, 0u, s, 0u, p.key0, p.key1); }

__host__ __device__ inline double syn_u(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

// frame m < F before its rounding: late + direct + reflections in double (irroom.hip.h adds a fourth term before it rounds)
__host__ __device__ inline double2 syn_frame64(const SynPlan& p, uint64_t m) {
    double L = 0.0, R = 0.0;
    if (m >= p.late_start) {
        const uint64_t t = m - p.late_start;
        bool on = true;
        double occ = 1.0;
        if (t + 1 < (uint64_t)p.build_up) {
            const uint64_t B = p.build_up, a = t + 1;  // a < B <= 65535
            const uint32_t w = syn_words(p, (uint32_t)m, 1u).w0;
            on = w < (1u << 28) || (uint64_t)w * (B * B) < ((a * a) << 32);
            const double r = (double)a / (double)B;
            occ = 1.0 / sqrt(fmax(1.0 / 16.0, r * r));
        }
        if (on) {
            const SynWords w = syn_words(p, (uint32_t)m, 0u);
            const double gA = sqrt(-2.0 * log(syn_u(w.w0))) * cos(2.0 * M_PI * syn_u(w.w1));
            const double gB = sqrt(-2.0 * log(syn_u(w.w2))) * cos(2.0 * M_PI * syn_u(w.w3));
            const double env = p.late_gain * (p.t60 ? exp2(-((double)t * ISH_DECAY_K) / (double)p.t60) : 1.0);
            L = gA * env * occ;
            R = (p.rho * gA + p.rho_c * gB) * env * occ;
        }
    }
    if (m == 0) {
        L += p.direct;
        R += p.direct;
    }
    if (m < (uint64_t)p.early_end)
        for (uint32_t j = 0; j < p.n_early; j++)
            if ((uint64_t)p.pos[j] == m) {
                L += p.gL[j];
                R += p.gR[j];
            }
    return make_double2(L, R);
}

// frame m < F
__host__ __device__ inline float2 syn_frame(const SynPlan& p, uint64_t m) {
    const double2 v = syn_frame64(p, m);
    return make_float2((float)v.x, (float)v.y);
}

// x[0 .. F): two consecutive frames per thread as one 16-byte store.  x is 8-byte aligned; when it is not 16-byte aligned
// frame 0 is stored alone, and so is a last odd frame (ish_walk's head and tail), both by thread 0 of workgroup 0.
// gridDim.x * SYN_THREADS >= max(pairs, 1).
__global__ __launch_bounds__(SYN_THREADS) void k_synth(float2* __restrict__ x, SynPlan p) {
    const uint64_t n = p.F;
    const uint64_t head = ((uintptr_t)x & 8) && n ? 1 : 0, pairs = (n - head) / 2;
    float4* __restrict__ x2 = reinterpret_cast<float4*>(x + head);
    const uint64_t i = (uint64_t)blockIdx.x * SYN_THREADS + threadIdx.x;
    if (i < pairs) {
        const float2 a = syn_frame(p, head + 2 * i), b = syn_frame(p, head + 2 * i + 1);
        x2[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    if (i == 0) {
        if (head) x[0] = syn_frame(p, 0);
        if (head + 2 * pairs < n) x[n - 1] = syn_frame(p, n - 1);
    }
}

// Every field of a synthesis, in field order, checked without touching an engine or HIP; the message names the field.  Null
// when it is good.
inline const char* syn_check(const mc_ir_synth* s) {
    static thread_local char msg[200];
    if (!s) return "null synth";
    if (s->struct_size != sizeof(mc_ir_synth)) return "mc_ir_synth struct_size mismatch";
    msg[0] = 0;
    if (s->n_early > MC_SYNTH_MAX_EARLY)
        std::snprintf(msg, sizeof(msg), "n_early %u above %d", s->n_early, MC_SYNTH_MAX_EARLY);
    else if (s->frames < 1 || s->frames > SYN_MAX_FRAMES)
        std::snprintf(msg, sizeof(msg), "frames %llu outside [1, %llu]", (unsigned long long)s->frames, (unsigned long long)SYN_MAX_FRAMES);
    else if (s->build_up > SYN_MAX_BUILD_UP)
        std::snprintf(msg, sizeof(msg), "build_up %u above %u", s->build_up, SYN_MAX_BUILD_UP);
    else if (!(std::isfinite(s->late_gain) && s->late_gain >= 0.f))
        std::snprintf(msg, sizeof(msg), "late_gain %g must be finite and >= 0", (double)s->late_gain);
    else if (!std::isfinite(s->direct))
        std::snprintf(msg, sizeof(msg), "direct %g must be finite", (double)s->direct);
    else if (!std::isfinite(s->early_gain))
        std::snprintf(msg, sizeof(msg), "early_gain %g must be finite", (double)s->early_gain);
    else if (!(s->width >= 0.f && s->width <= 1.f))
        std::snprintf(msg, sizeof(msg), "width %g outside [0, 1]", (double)s->width);
    else if (s->rate && (s->rate < 8000 || s->rate > 384000))
        std::snprintf(msg, sizeof(msg), "rate %u outside [8000, 384000] (0 = none: no EQ band and no damping)", s->rate);
    else if (s->n_early && s->early_first > s->early_last)
        std::snprintf(msg, sizeof(msg), "early_first %llu above early_last %llu", (unsigned long long)s->early_first, (unsigned long long)s->early_last);
    else if (s->n_early && s->early_last >= SYN_MAX_FRAMES)
        std::snprintf(msg, sizeof(msg), "early_last %llu not below %llu", (unsigned long long)s->early_last, (unsigned long long)SYN_MAX_FRAMES);
    return msg[0] ? msg : nullptr;
}

// A checked synthesis as the kernel takes it.  The reflection table is made here, in double: W(j, 2) gives reflection j its
// position (integer arithmetic), its sign, and its pan under the engine's pan law (conv.cu:386-387).
inline SynPlan syn_plan(const mc_ir_synth& s) {
    SynPlan p{};
    p.F = s.frames;
    p.late_start = s.late_start;
    p.t60 = s.t60;
    p.key0 = (uint32_t)(s.seed & 0xffffffffull);
    p.key1 = (uint32_t)(s.seed >> 32);
    p.build_up = s.build_up;
    p.late_gain = (double)s.late_gain;
    p.direct = (double)s.direct;
    p.rho = 1.0 - (double)s.width;
    p.rho_c = std::sqrt(1.0 - p.rho * p.rho);
    if (!s.n_early) return p;
    const uint64_t span = s.early_last - s.early_first + 1;
    for (uint32_t j = 0; j < s.n_early; j++) {
        const SynWords w = syn_words(p, j, 2u);
        const uint64_t pos = s.early_first + (((uint64_t)w.w0 * span) >> 32);
        if (pos >= s.frames) continue;
        const double g = (double)s.early_gain * ((w.w1 & 1u) ? -1.0 : 1.0) * (double)(s.early_first + 1) / (double)(pos + 1);
        const double pan = (double)s.width * (2.0 * syn_u(w.w2) - 1.0);
        p.pos[p.n_early] = (uint32_t)pos;
        p.gL[p.n_early] = g * (pan >= 0.0 ? 1.0 - pan : 1.0);
        p.gR[p.n_early] = g * (pan <= 0.0 ? 1.0 + pan : 1.0);
        p.n_early++;
        if (pos + 1 > p.early_end) p.early_end = (uint32_t)(pos + 1);
    }
    return p;
}

// the p.F frames into d_x (8-byte aligned, p.F float2), on `stream`; does not synchronise
inline hipError_t syn_generate(hipStream_t stream, const SynPlan& p, float2* d_x) {
    const uint64_t pairs = p.F / 2;  // (an unaligned d_x has at most as many)
    const unsigned grid = (unsigned)((std::max<uint64_t>(pairs, 1) + SYN_THREADS - 1) / SYN_THREADS);
    hipLaunchKernelGGL(k_synth, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, p);
    return hipGetLastError();
}
