// irroom.hip.h — the reflections of a rectangular room on the device (mc_synth_ir_room): Allen and Berkley's image-source
// method, every image a Hann-windowed sinc of 32 taps at its fractional delay, summed in 64-bit integers.  No reference
// equivalent: the reference convolves with the frames of a WAV file.
//
// include/mcconv.h has the definition and tests/ir_room_np.py states it in float64:
//   images    n in [-N, N]^3, u in {0, 1}^3: p_a = ((1 - 2 u_a) s_a + 2 n_a L_a) - r_a per receiver, d = |p|,
//             a = gain * prod_a beta_(a,0)^|n_a - u_a| beta_(a,1)^|n_a| / d, tau = d rate / c, k0 = floor(tau), f = tau - k0;
//   taps      k = -15 .. 16, x = k - f: w_k = (k odd ? s : -s) / (pi x) * (1 + cos(pi x / 16)) / 2, s = sin(pi f); f == 0: one tap;
//   sum       q = llrint(a w_k 2^40) added into acc[k0 + k][channel], int64: the sum does not depend on the order of arrival,
//             so the same struct gives the same bits whatever the grid and however many images share a frame;
//   frame     (float)(late + direct + reflections + acc 2^-40): irsynth.hip.h's three terms and this one, rounded once.
//
// k_room walks the lattice in one launch.  A wave takes 64 images at a time, one per lane, for the geometry: both receivers'
// distances and k0, which prune an image before any transcendental when neither channel arrives before frame E (most of the
// cube's corners go that way), then the amplitude (the powers of beta come from the host's table) and the one sine per channel.
// The kept images are then scattered one per step with lane = (tap, channel): a wave instruction adds up to 64 neighbouring
// 8-byte words (atomicAdd(unsigned long long*): one global_atomic_add_x2 per lane, no compare-and-swap loop).  The accumulator
// holds min(E + 16, F) frames, is zeroed on the stream before the launch and freed after k_synth_room has read it; the images
// kept per channel are counted with one add per wave and counter.
//
// Directional microphones and a directional source (mc_synth_ir_room_mics) are k_room's second instantiation: where a lane
// holds one image and has its b, it multiplies b / d by gs gr, two first-order patterns of two dot products with p, the
// source's aim mirrored with the image.  Nothing else differs: the delays, the prune, the counts and the scatter are shared,
// and the instantiation without microphones is the kernel as it was.
//
// Walls and air per frequency band (mc_synth_ir_room_bands): k_room runs once per band into that band's own accumulator, with
// the band's table of powers and, through a second template flag, its air factor exp2(-(d k_j)) on b / d; the instantiations
// without air are the kernels as they were.  The accumulators are joined by irdamp.hip.h's band split, written by its differences:
// D_k = (acc_(k-1) - acc_k) 2^-40 through crossover k's two sections (damp_step) over all F frames, chunked as every recurrence
// of the IR tools is (chunkwalk.hip.h):
//   local  k_room_join<false>, a workgroup row per crossover, runs every chunk from rest and keeps the end states;
//   carry  k_damp_carry, unchanged, over all X crossovers at once;
//   fix-up k_room_join<true>, one launch per crossover low to high, runs every chunk from its true state and adds P_k into
//          r [F]; the last one adds acc_X 2^-40 after it.  The order of the additions is the definition's.
// k_synth_room_bands then adds r where k_synth_room adds one accumulator's term.  Chunks and runs depend on F alone and the join
// has no atomics: the same struct stores the same bits whatever the grid.  Equal accumulators give D_k = 0, P_k = +0.0 and r the
// unbanded term: a banded room whose bands are alike stores the unbanded room's bits.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/mcconv.h"
#include "irdamp.hip.h"
#include "irsynth.hip.h"

constexpr int ROOM_THREADS = 256;
constexpr int ROOM_MAX_GRID = 2048;
constexpr int ROOM_REACH = 16;               // taps k = -(ROOM_REACH - 1) .. ROOM_REACH: two per lane pair of a wave
constexpr double ROOM_Q = 1099511627776.0;   // 2^40: the quantum of a contribution is 2^-40
constexpr double ROOM_MIN_DIRECT = 0.1;      // metres
constexpr double ROOM_MAX_SUM = 4194304.0;   // 2^22: 8 (2N + 1)^3 gain / d below it keeps the sum inside 2^62 (with microphones
                                             // too: |gs gr| <= 1 makes no image louder)

// checked mc_ir_room_mics as the kernel takes them, fifteen doubles that room_factors knows by their place: the unit vectors
// of the aims of receiver L, receiver R and the source, and their patterns as alpha and as 1 - alpha
struct RoomMics {
    double aim[3][3], alpha[3], oma[3];
};

// a checked mc_ir_room as the kernels take it, everything in double from the float fields
struct RoomPlan {
    uint32_t N, S;      // the order used and 2N + 1
    uint32_t total;     // 8 S^3 images
    uint32_t mics;      // m is set (in the gap before E: with air in the place this flag had, the kernels' arguments lie where they lay)
    uint64_t E, F, A;   // images arriving at or after E are left out; A = min(E + 16, F) accumulator frames
    uint64_t complete;  // floor(2 N min(L) rate / c)
    double rate, speed, gain;
    double size[3], src[3], rcv[2][3];
    double tau[2];      // the direct sound's delay per channel, frames
    double bpow[6][MC_ROOM_MAX_ORDER + 2];  // bpow[w][j] = pow(beta[w], j), 0^0 = 1
    RoomMics m;         // mc_ir_room_mics, when `mics` is set
    double air;         // k_j of a band of mc_ir_room_bands, right behind m's fifteen numbers: the sixteenth; 0 = no factor
    double head[8];     // mc_ir_room_head, when `headed` is set: the ear axes e_L, e_R, a and shadow (behind everything the
    uint64_t shadow_at; // kernels without a head read); the shadow accumulator lies shadow_at words behind the plain one
    uint32_t headed;
};

// g(cos) of a first-order pattern: exactly 1 for alpha = 1 (oma = 0), whatever the cosine
__host__ __device__ inline double room_pattern(double alpha, double oma, double cosine) { return fma(oma, cosine, alpha); }

// a . p in the definition's order
__host__ __device__ inline double room_dot(double ax, double ay, double az, double px, double py, double pz) { return fma(pz, az, fma(py, ay, px * ax)); }

// {gs, gr} of channel c for the image at p (from the receiver), d = |p|, whose axes are mirrored where sx, sy, sz = 1 - 2 u_a
// are -1; get(j) is number j of a RoomMics
template <class Get>
__host__ __device__ inline double2 room_factors(Get get, int c, double sx, double sy, double sz, double px, double py, double pz, double d) {
    const double cr = room_dot(get(3 * c), get(3 * c + 1), get(3 * c + 2), px, py, pz) / d;
    const double cs = -room_dot(sx * get(6), sy * get(7), sz * get(8), px, py, pz) / d;  // (times 1 or -1: exact)
    return make_double2(room_pattern(get(11), get(14), cs), room_pattern(get(9 + c), get(12 + c), cr));
}

// {g, th} of an ear whose axis is e for an arrival from p, d = |p|: the angle th between them and the path's excess over d in
// units of the radius
__host__ __device__ inline double2 room_ear(double ex, double ey, double ez, double px, double py, double pz, double d) {
    const double cs = fmin(1.0, fmax(-1.0, room_dot(ex, ey, ez, px, py, pz) / d));
    const double th = acos(cs);
    return make_double2(cs >= 0.0 ? -cs : th - M_PI / 2, th);
}

// h = alpha - 1 of Brown and Duda's shelf at the angle th from the ear's axis
__host__ __device__ inline double room_shadow(double shadow, double th) { return shadow * fma(0.95, cos(1.2 * th), 0.05); }

// One launch over the lattice; gridDim.x * ROOM_THREADS / 64 waves stride over it 64 images at a time.  acc: p.A frames of two
// int64, zero; kept: two zeroed counters.  MICS: p.mics is set, and an image's amplitude takes its factor gs gr.  AIR: p.air is
// not 0, and b / d takes the factor exp2(-(d p.air)) before that.  HEAD: p.headed is set, both receivers are the head's centre,
// each ear has its own delay and shadow factor, and acc + p.shadow_at is a second accumulator as large as the first, zero too.
template <bool MICS, bool AIR, bool HEAD = false>
__global__ __launch_bounds__(ROOM_THREADS) void k_room(unsigned long long* __restrict__ acc, unsigned* __restrict__ kept, RoomPlan p) {
    const unsigned lane = threadIdx.x & 63u;
    uint32_t wave = (blockIdx.x * ROOM_THREADS + threadIdx.x) >> 6;
    const uint32_t nwaves = gridDim.x * (ROOM_THREADS / 64);
    if (MICS) wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);  // (the same in every lane: the walk below becomes scalar)
    const int ch = (int)(lane & 1u), k = (int)(lane >> 1) - (ROOM_REACH - 1);
    unsigned nkept[2] = {0u, 0u};
    // The microphones' fifteen numbers, one per lane of a register pair, and read from there where an image needs them: the
    // kernel without them already fills the scalar registers (102 of 102), and thirty more for the whole walk would spill.
    // (v_readlane does not look at EXEC: the lanes that hold the numbers need not be among those that hold a kept image.)
    // The air constant travels the same way, as number 15, and with it the receivers' six coordinates, as numbers 16 to 21:
    // the double exp2 wants scalar registers for its constants as the sine does, and without those twelve back hipcc spills two.
    // The head's eight numbers are numbers 22 to 29, and a head takes the receivers' coordinates from the lanes as the air does.
    const double mics = HEAD && lane >= 22 && lane < 30                ? p.head[lane - 22]
                        : (AIR || HEAD) && lane >= 16 && lane < 22     ? (&p.rcv[0][0])[lane - 16]
                        : (MICS && lane < 15) || (AIR && lane == 15) ? reinterpret_cast<const double*>(&p.m)[lane]
                                                                     : 0.0;
    const auto mic = [mics](int j) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mics), j), __builtin_amdgcn_readlane(__double2loint(mics), j));
    };
    for (uint64_t base = (uint64_t)wave * 64; base < p.total; base += (uint64_t)nwaves * 64) {
        const uint64_t i = base + lane;
        long long k0[2] = {0, 0};
        double f[2] = {0.0, 0.0}, s[2] = {0.0, 0.0}, a[2] = {0.0, 0.0};  // (a stays 0 for a channel that is not kept)
        double sh[2] = {0.0, 0.0};                                       // HEAD: a h, the shadow accumulator's amplitude
        bool keep[2] = {false, false};
        if (i < p.total) {
            const uint32_t cell = (uint32_t)(i >> 3);
            const int u[3] = {(int)(i & 1), (int)((i >> 1) & 1), (int)((i >> 2) & 1)};
            const int n[3] = {(int)(cell % p.S) - (int)p.N, (int)((cell / p.S) % p.S) - (int)p.N, (int)(cell / (p.S * p.S)) - (int)p.N};
            double q[3], b = p.gain;
#pragma unroll
            for (int ax = 0; ax < 3; ax++) q[ax] = (double)(1 - 2 * u[ax]) * p.src[ax] + (double)(2 * n[ax]) * p.size[ax];
            double d[2], tau[2], th[2] = {0.0, 0.0};
            if (HEAD) {
                const double px = q[0] - mic(16), py = q[1] - mic(17), pz = q[2] - mic(18);
                d[0] = d[1] = sqrt(px * px + py * py + pz * pz);
                // An ear's path is at most the radius shorter than d: an image that even so arrives a frame or more past E is
                // kept by neither ear, and is pruned before any arc cosine.
                if ((d[0] - mic(28)) * p.rate / p.speed < (double)p.E + 1.0) {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const double2 e = room_ear(mic(22 + 3 * c), mic(23 + 3 * c), mic(24 + 3 * c), px, py, pz, d[c]);
                        th[c] = e.y;
                        tau[c] = fma(mic(28), e.x, d[c]) * p.rate / p.speed;
                        const double fl = floor(tau[c]);
                        keep[c] = fl < (double)p.E;
                        k0[c] = (long long)fl;
                        f[c] = tau[c] - fl;
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const double px = q[0] - (AIR ? mic(16 + 3 * c) : p.rcv[c][0]), py = q[1] - (AIR ? mic(17 + 3 * c) : p.rcv[c][1]),
                                 pz = q[2] - (AIR ? mic(18 + 3 * c) : p.rcv[c][2]);
                    d[c] = sqrt(px * px + py * py + pz * pz);
                    tau[c] = d[c] * p.rate / p.speed;
                    const double fl = floor(tau[c]);
                    keep[c] = fl < (double)p.E;
                    k0[c] = (long long)fl;
                    f[c] = tau[c] - fl;
                }
            }
            if (keep[0] || keep[1]) {
#pragma unroll
                for (int ax = 0; ax < 3; ax++) b *= p.bpow[2 * ax][abs(n[ax] - u[ax])] * p.bpow[2 * ax + 1][abs(n[ax])];
                double air[2] = {1.0, 1.0};
                if (AIR) {  // (for both channels, kept or not: no branch, and before the sine)
                    const double kj = mic(15);
#pragma unroll
                    for (int c = 0; c < 2; c++) air[c] = exp2(-(d[c] * kj));
                }
#pragma unroll
                for (int c = 0; c < 2; c++)
                    if (keep[c]) {
                        a[c] = b / d[c];
                        if (AIR) a[c] *= air[c];
                        s[c] = sin(M_PI * f[c]);
                        if (MICS) {  // (after the sine, whose constants want the scalar registers too: before it hipcc reserves scratch)
                            const double2 g = room_factors(mic, c, (double)(1 - 2 * u[0]), (double)(1 - 2 * u[1]), (double)(1 - 2 * u[2]),
                                                           q[0] - (AIR || HEAD ? mic(16 + 3 * c) : p.rcv[c][0]), q[1] - (AIR || HEAD ? mic(17 + 3 * c) : p.rcv[c][1]),
                                                           q[2] - (AIR || HEAD ? mic(18 + 3 * c) : p.rcv[c][2]), d[c]);
                            a[c] *= g.x * g.y;
                        }
                        if (HEAD) sh[c] = a[c] * room_shadow(mic(29), th[c]);
                    }
            }
        }
        nkept[0] += (unsigned)__popcll(__ballot(keep[0]));
        nkept[1] += (unsigned)__popcll(__ballot(keep[1]));
        unsigned long long todo = __ballot(a[0] != 0.0 || a[1] != 0.0);
        while (todo) {  // (wave-uniform: one kept image per step, this lane's tap and channel of it)
            const int j = __ffsll(todo) - 1;
            todo &= todo - 1;
            const long long k0L = __shfl(k0[0], j), k0R = __shfl(k0[1], j);
            const double fL = __shfl(f[0], j), fR = __shfl(f[1], j), sL = __shfl(s[0], j), sR = __shfl(s[1], j);
            const double aL = __shfl(a[0], j), aR = __shfl(a[1], j);
            const long long kj = ch ? k0R : k0L;
            const double fj = ch ? fR : fL, sj = ch ? sR : sL, aj = ch ? aR : aL;
            double hj = 0.0;
            if (HEAD) {
                const double hL = __shfl(sh[0], j), hR = __shfl(sh[1], j);
                hj = ch ? hR : hL;
            }
            if (aj != 0.0) {
                double w;
                if (fj == 0.0) {
                    w = k == 0 ? 1.0 : 0.0;
                } else {
                    const double x = (double)k - fj;
                    w = ((k & 1) ? sj : -sj) / (M_PI * x) * ((1.0 + cos(M_PI * x / 16.0)) / 2.0);
                }
                const long long v = llrint(aj * w * ROOM_Q), m = kj + k;
                if (v != 0 && m >= 0 && (uint64_t)m < p.A) atomicAdd(&acc[2 * (uint64_t)m + ch], (unsigned long long)v);
                if (HEAD && hj != 0.0) {  // (a h is 0 only where a is or the shadow is: the same taps of the same image)
                    const long long vs = llrint(hj * w * ROOM_Q);
                    if (vs != 0 && m >= 0 && (uint64_t)m < p.A) atomicAdd(&acc[p.shadow_at + 2 * (uint64_t)m + ch], (unsigned long long)vs);
                }
            }
        }
    }
    if (lane == 0) {
        if (nkept[0]) atomicAdd(&kept[0], nkept[0]);
        if (nkept[1]) atomicAdd(&kept[1], nkept[1]);
    }
}

// frame m < F with the room's term: irsynth.hip.h's three terms and acc 2^-40, added in that order in double, rounded once
__device__ inline float2 room_frame(const SynPlan& p, uint64_t m, const long long* __restrict__ acc, uint64_t A) {
    double2 v = syn_frame64(p, m);
    if (m < A) {
        v.x += (double)acc[2 * m] * (1.0 / ROOM_Q);
        v.y += (double)acc[2 * m + 1] * (1.0 / ROOM_Q);
    }
    return make_float2((float)v.x, (float)v.y);
}

// k_synth with the room's term: the same walk and the same stores
__global__ __launch_bounds__(SYN_THREADS) void k_synth_room(float2* __restrict__ x, SynPlan p, const long long* __restrict__ acc, uint64_t A) {
    const uint64_t n = p.F;
    const uint64_t head = ((uintptr_t)x & 8) && n ? 1 : 0, pairs = (n - head) / 2;
    float4* __restrict__ x2 = reinterpret_cast<float4*>(x + head);
    const uint64_t i = (uint64_t)blockIdx.x * SYN_THREADS + threadIdx.x;
    if (i < pairs) {
        const float2 a = room_frame(p, head + 2 * i, acc, A), b = room_frame(p, head + 2 * i + 1, acc, A);
        x2[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    if (i == 0) {
        if (head) x[0] = room_frame(p, 0, acc, A);
        if (head + 2 * pairs < n) x[n - 1] = room_frame(p, n - 1, acc, A);
    }
}

// the crossovers of a checked mc_ir_room_bands as the join takes them: one section of crossover k + 1 (damp_plan's)
struct RoomJoin {
    int X;
    IeqCoef c[MC_DAMP_MAX_XOVERS];
};

static_assert(offsetof(RoomPlan, air) == offsetof(RoomPlan, m) + 15 * sizeof(double), "k_room reads the air constant as number 15 behind the microphones'");

// One pass of the join over F frames for crossover k + 1, k = k0 + blockIdx.y: its input D[m] = (acc_k[m] - acc_(k+1)[m]) 2^-40
// below A and 0 from there, formed where the walk loads it.  acc: [B][A] pairs of int64 (16-byte aligned).  st: double2
// [X][gridDim.x * IEQ_THREADS][2], k_damp_chunk's layout, which k_damp_carry scans.  FIX = false: from rest, the end states to st.
// FIX = true (gridDim.y = 1, k0 = 0 .. X - 1 in that order): from the state st holds, r[m] = P (k == 0) or r[m] + P, and the
// last crossover adds acc_X[m] 2^-40 after it.  Frames at and past F read as zero and are not written.
template <bool FIX>
__global__ __launch_bounds__(IEQ_THREADS) void k_room_join(const longlong2* __restrict__ acc, uint64_t A, uint64_t F, RoomJoin pl, int k0, double2* __restrict__ st,
                                                           double2* __restrict__ r) {
    const int k = k0 + (int)blockIdx.y;
    const uint64_t lanes = (uint64_t)gridDim.x * IEQ_THREADS, entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    const longlong2* __restrict__ lo = acc + A * (uint64_t)k;
    const longlong2* __restrict__ hi = lo + A;
    const IeqCoef c = pl.c[k];
    DampState s{0.0, 0.0, 0.0, 0.0};
    if (FIX) s = damp_load(st, (uint64_t)k * lanes + entry);
    chunk_walk<false, IEQ_TILE, double2>(
        FIX,
        [&](uint64_t g, double2& v) {
            v = make_double2(0.0, 0.0);
            if (g < A) {
                const longlong2 a = lo[g], b = hi[g];
                v = make_double2((double)(a.x - b.x) * (1.0 / ROOM_Q), (double)(a.y - b.y) * (1.0 / ROOM_Q));
            }
        },
        [&](double& tap, uint64_t) {
            const double y = damp_step(c, s, tap);
            if (FIX) tap = y;
        },
        [&](uint64_t g, double2 v) {
            if (g < F) {
                if (k) {
                    const double2 sum = r[g];
                    v = make_double2(sum.x + v.x, sum.y + v.y);
                }
                if (k + 1 == pl.X && g < A) {
                    const longlong2 top = hi[g];
                    v = make_double2(v.x + (double)top.x * (1.0 / ROOM_Q), v.y + (double)top.y * (1.0 / ROOM_Q));
                }
                r[g] = v;
            }
        });
    if (!FIX) damp_store(st, (uint64_t)k * lanes + entry, s);
}

// frame m < F with the banded room's term r[m]
__device__ inline float2 room_frame(const SynPlan& p, uint64_t m, const double2* __restrict__ r) {
    double2 v = syn_frame64(p, m);
    const double2 t = r[m];
    v.x += t.x;
    v.y += t.y;
    return make_float2((float)v.x, (float)v.y);
}

// k_synth_room with the join's r [F] in place of one accumulator's term
__global__ __launch_bounds__(SYN_THREADS) void k_synth_room_bands(float2* __restrict__ x, SynPlan p, const double2* __restrict__ r) {
    const uint64_t n = p.F;
    const uint64_t head = ((uintptr_t)x & 8) && n ? 1 : 0, pairs = (n - head) / 2;
    float4* __restrict__ x2 = reinterpret_cast<float4*>(x + head);
    const uint64_t i = (uint64_t)blockIdx.x * SYN_THREADS + threadIdx.x;
    if (i < pairs) {
        const float2 a = room_frame(p, head + 2 * i, r), b = room_frame(p, head + 2 * i + 1, r);
        x2[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    if (i == 0) {
        if (head) x[0] = room_frame(p, 0, r);
        if (head + 2 * pairs < n) x[n - 1] = room_frame(p, n - 1, r);
    }
}

// the fixed high-pass of the head's shelf: K = tan(c / (a rate)), y = b0 v + s, s' = b1 v - a1 y
struct RoomShelf {
    double K, b0, b1, a1;
};

// One pass of the head's high-pass over F frames.  Its input is accS[m] 2^-40 below A (accS: A pairs of int64, 16-byte aligned)
// or, with rS, rS[m] (the join of the bands' shadow accumulators), and 0 from A or F on.  st: double2 [gridDim.x * IEQ_THREADS],
// k_eq_chunk's layout, which k_eq_carry scans: (s, 0).  FIX = false: from rest, the end states to st.  FIX = true: from the state
// st holds, r[m] = S[m] + (m < A ? accP[m] 2^-40 : 0) or, with accP null, S[m] + r[m] (the join of the plain accumulators, in
// place).  Frames at and past F read as zero and are not written.
template <bool FIX>
__global__ __launch_bounds__(IEQ_THREADS) void k_room_head(const longlong2* __restrict__ accS, const double2* __restrict__ rS, const longlong2* __restrict__ accP,
                                                           uint64_t A, uint64_t F, RoomShelf c, double2* __restrict__ st, double2* r) {
    const uint64_t entry = (uint64_t)blockIdx.x * IEQ_THREADS + threadIdx.x;
    double s = FIX ? st[entry].x : 0.0;
    chunk_walk<false, IEQ_TILE, double2>(
        FIX,
        [&](uint64_t g, double2& v) {
            v = make_double2(0.0, 0.0);
            if (rS) {
                if (g < F) v = rS[g];
            } else if (g < A) {
                const longlong2 a = accS[g];
                v = make_double2((double)a.x * (1.0 / ROOM_Q), (double)a.y * (1.0 / ROOM_Q));
            }
        },
        [&](double& tap, uint64_t) {
            const double v = tap, y = c.b0 * v + s;
            s = c.b1 * v - c.a1 * y;
            if (FIX) tap = y;
        },
        [&](uint64_t g, double2 v) {
            if (g < F) {
                double2 plain = make_double2(0.0, 0.0);
                if (!accP) {
                    plain = r[g];
                } else if (g < A) {
                    const longlong2 a = accP[g];
                    plain = make_double2((double)a.x * (1.0 / ROOM_Q), (double)a.y * (1.0 / ROOM_Q));
                }
                r[g] = make_double2(v.x + plain.x, v.y + plain.y);
            }
        });
    if (!FIX) st[entry] = make_double2(s, 0.0);
}

// -- host ------------------------------------------------------------------------------------------------------------
inline double room_min_size(const mc_ir_room& r) { return (double)std::min(r.size_m[0], std::min(r.size_m[1], r.size_m[2])); }

// E of the definition
inline uint64_t room_last(const mc_ir_room& r, uint64_t F) { return r.last ? std::min<uint64_t>(r.last, F) : F; }

// the order `order` 0 stands for: the smallest N whose lattice holds every image that arrives before frame E (as a double:
// it may lie far above MC_ROOM_MAX_ORDER)
inline double room_auto_order(const mc_ir_room& r, uint32_t rate, uint64_t F) {
    return std::ceil((double)room_last(r, F) * (double)r.speed / ((double)rate * 2.0 * room_min_size(r)));
}

// the receiver of channel c along axis ax
inline double room_receiver(const mc_ir_room& r, int c, int ax) {
    const double centre = (double)r.receiver_m[ax];
    if ((uint32_t)ax != r.axis) return centre;
    return c ? centre + (double)r.spacing_m / 2.0 : centre - (double)r.spacing_m / 2.0;
}

inline double room_direct(const mc_ir_room& r, int c) {
    double sq = 0.0;
    for (int ax = 0; ax < 3; ax++) {
        const double p = (double)r.source_m[ax] - room_receiver(r, c, ax);
        sq += p * p;
    }
    return std::sqrt(sq);
}

// Every field of a room, in the struct's order, then what follows from them and from the session's rate and F (a checked
// synthesis's), without touching an engine or HIP; the message names the field.  Null when it is good.
inline const char* room_check(const mc_ir_room* r, uint32_t rate, uint64_t F) {
    static thread_local char msg[240];
    if (!r) return "null room";
    if (r->struct_size != sizeof(mc_ir_room)) return "mc_ir_room struct_size mismatch";
    msg[0] = 0;
    if (r->order > MC_ROOM_MAX_ORDER) {
        std::snprintf(msg, sizeof(msg), "order %u above %d", r->order, MC_ROOM_MAX_ORDER);
        return msg;
    }
    for (int ax = 0; ax < 3; ax++)
        if (!(std::isfinite(r->size_m[ax]) && r->size_m[ax] >= 0.5f && r->size_m[ax] <= 200.f)) {
            std::snprintf(msg, sizeof(msg), "size_m[%d] %g outside [0.5, 200]", ax, (double)r->size_m[ax]);
            return msg;
        }
    for (int ax = 0; ax < 3; ax++)
        if (!(r->source_m[ax] > 0.f && r->source_m[ax] < r->size_m[ax])) {
            std::snprintf(msg, sizeof(msg), "source_m[%d] %g not strictly inside (0, %g)", ax, (double)r->source_m[ax], (double)r->size_m[ax]);
            return msg;
        }
    for (int ax = 0; ax < 3; ax++)
        if (!(r->receiver_m[ax] > 0.f && r->receiver_m[ax] < r->size_m[ax])) {
            std::snprintf(msg, sizeof(msg), "receiver_m[%d] %g not strictly inside (0, %g)", ax, (double)r->receiver_m[ax], (double)r->size_m[ax]);
            return msg;
        }
    for (int w = 0; w < 6; w++)
        if (!(r->beta[w] >= -1.f && r->beta[w] <= 1.f)) {
            std::snprintf(msg, sizeof(msg), "beta[%d] %g outside [-1, 1]", w, (double)r->beta[w]);
            return msg;
        }
    if (!(std::isfinite(r->spacing_m) && r->spacing_m >= 0.f)) {
        std::snprintf(msg, sizeof(msg), "spacing_m %g must be finite and >= 0", (double)r->spacing_m);
        return msg;
    }
    if (r->axis > 2) {
        std::snprintf(msg, sizeof(msg), "axis %u above 2", r->axis);
        return msg;
    }
    if (!(room_receiver(*r, 0, (int)r->axis) > 0.0 && room_receiver(*r, 1, (int)r->axis) < (double)r->size_m[r->axis])) {
        std::snprintf(msg, sizeof(msg), "spacing_m %g puts a receiver outside (0, %g) along axis %u", (double)r->spacing_m, (double)r->size_m[r->axis], r->axis);
        return msg;
    }
    if (!(std::isfinite(r->speed) && r->speed >= 100.f && r->speed <= 2000.f)) {
        std::snprintf(msg, sizeof(msg), "speed %g outside [100, 2000]", (double)r->speed);
        return msg;
    }
    if (!(std::isfinite(r->gain) && r->gain > 0.f && r->gain <= 16.f)) {
        std::snprintf(msg, sizeof(msg), "gain %g outside (0, 16]", (double)r->gain);
        return msg;
    }
    if (r->reserved) {
        std::snprintf(msg, sizeof(msg), "reserved %u must be 0", r->reserved);
        return msg;
    }
    if (rate < 8000 || rate > 384000) {
        std::snprintf(msg, sizeof(msg), "rate %u outside [8000, 384000]: the room needs the session's rate", rate);
        return msg;
    }
    const double dmin = std::min(room_direct(*r, 0), room_direct(*r, 1));
    if (!(dmin >= ROOM_MIN_DIRECT)) {
        std::snprintf(msg, sizeof(msg), "source_m and receiver_m are %g m apart, below %g", dmin, ROOM_MIN_DIRECT);
        return msg;
    }
    double N = (double)r->order;
    if (!r->order) {
        N = room_auto_order(*r, rate, F);
        if (!(N <= (double)MC_ROOM_MAX_ORDER)) {
            std::snprintf(msg, sizeof(msg), "order 0 needs order %.0f for %llu frames, above %d: set last or order", N,
                          (unsigned long long)room_last(*r, F), MC_ROOM_MAX_ORDER);
            return msg;
        }
    }
    const double images = 8.0 * (2.0 * N + 1.0) * (2.0 * N + 1.0) * (2.0 * N + 1.0);
    if (!(images * (double)r->gain / dmin < ROOM_MAX_SUM)) {
        std::snprintf(msg, sizeof(msg), "gain %g: %.0f images of at most gain / %g m each may sum to 2^22 or more", (double)r->gain, images, dmin);
        return msg;
    }
    return nullptr;
}

// a checked room as the kernels take it
inline RoomPlan room_plan(const mc_ir_room& r, uint32_t rate, uint64_t F) {
    RoomPlan p{};
    p.N = r.order ? r.order : (uint32_t)room_auto_order(r, rate, F);
    p.S = 2 * p.N + 1;
    p.total = 8u * p.S * p.S * p.S;
    p.F = F;
    p.E = room_last(r, F);
    p.A = std::min<uint64_t>(p.E + ROOM_REACH, F);
    p.rate = (double)rate;
    p.speed = (double)r.speed;
    p.gain = (double)r.gain;
    p.complete = (uint64_t)std::floor((double)(2 * p.N) * room_min_size(r) * p.rate / p.speed);
    for (int ax = 0; ax < 3; ax++) {
        p.size[ax] = (double)r.size_m[ax];
        p.src[ax] = (double)r.source_m[ax];
        for (int c = 0; c < 2; c++) p.rcv[c][ax] = room_receiver(r, c, ax);
    }
    for (int c = 0; c < 2; c++) p.tau[c] = room_direct(r, c) * p.rate / p.speed;
    for (int w = 0; w < 6; w++)
        for (int j = 0; j < MC_ROOM_MAX_ORDER + 2; j++) p.bpow[w][j] = std::pow((double)r.beta[w], (double)j);
    return p;
}

// Every field of the microphones, in the struct's order, without touching an engine or HIP; the message names the field.
// Null when they are good.
inline const char* room_mics_check(const mc_ir_room_mics* m) {
    static thread_local char msg[160];
    if (!m) return "null mics";
    if (m->struct_size != sizeof(mc_ir_room_mics)) return "mc_ir_room_mics struct_size mismatch";
    msg[0] = 0;
    const auto outside = [](const char* name, int j, float v, double lo, double hi) {
        if (std::isfinite(v) && (double)v >= lo && (double)v <= hi) return false;
        if (j < 0)
            std::snprintf(msg, sizeof(msg), "%s %g outside [%g, %g]", name, (double)v, lo, hi);
        else
            std::snprintf(msg, sizeof(msg), "%s[%d] %g outside [%g, %g]", name, j, (double)v, lo, hi);
        return true;
    };
    if (m->flags) {
        std::snprintf(msg, sizeof(msg), "mics flags %u must be 0", m->flags);
        return msg;
    }
    for (int c = 0; c < 2; c++)
        if (outside("mic_pattern", c, m->mic_pattern[c], 0.0, 1.0)) return msg;
    for (int c = 0; c < 2; c++)
        if (outside("mic_az_deg", c, m->mic_az_deg[c], -360.0, 360.0)) return msg;
    for (int c = 0; c < 2; c++)
        if (outside("mic_el_deg", c, m->mic_el_deg[c], -90.0, 90.0)) return msg;
    if (outside("src_pattern", -1, m->src_pattern, 0.0, 1.0)) return msg;
    if (outside("src_az_deg", -1, m->src_az_deg, -360.0, 360.0)) return msg;
    if (outside("src_el_deg", -1, m->src_el_deg, -90.0, 90.0)) return msg;
    if (m->reserved) {
        std::snprintf(msg, sizeof(msg), "mics reserved %u must be 0", m->reserved);
        return msg;
    }
    return nullptr;
}

// checked microphones into a room's plan: the aims as unit vectors, the patterns as alpha and 1 - alpha
inline void room_plan_mics(RoomPlan& p, const mc_ir_room_mics& m) {
    const float alpha[3] = {m.mic_pattern[0], m.mic_pattern[1], m.src_pattern};
    const float az[3] = {m.mic_az_deg[0], m.mic_az_deg[1], m.src_az_deg}, el[3] = {m.mic_el_deg[0], m.mic_el_deg[1], m.src_el_deg};
    for (int j = 0; j < 3; j++) {
        const double a = (double)az[j] * M_PI / 180, e = (double)el[j] * M_PI / 180;
        p.m.aim[j][0] = std::cos(e) * std::cos(a);
        p.m.aim[j][1] = std::cos(e) * std::sin(a);
        p.m.aim[j][2] = std::sin(e);
        p.m.alpha[j] = (double)alpha[j];
        p.m.oma[j] = 1.0 - (double)alpha[j];
    }
    p.mics = 1;
}

// what mc_ir_room_mics_plan and mc_ir_room_mics_info report: the direct sound's gs L, R, gr L, R, gs gr L, R, 0, 0
inline void room_mics_report(const RoomPlan& p, double out[8]) {
    const double* numbers = &p.m.aim[0][0];
    const auto mic = [numbers](int j) { return numbers[j]; };
    for (int c = 0; c < 2; c++) {
        const double px = p.src[0] - p.rcv[c][0], py = p.src[1] - p.rcv[c][1], pz = p.src[2] - p.rcv[c][2];
        const double2 g = room_factors(mic, c, 1.0, 1.0, 1.0, px, py, pz, std::sqrt(px * px + py * py + pz * pz));
        out[c] = g.x, out[2 + c] = g.y, out[4 + c] = g.x * g.y;
    }
    out[6] = out[7] = 0.0;
}

// what mc_ir_room_plan reports of a checked room
inline void room_report(const mc_ir_room& r, uint32_t rate, uint64_t F, double out[8]) {
    const RoomPlan p = room_plan(r, rate, F);
    const double Lx = p.size[0], Ly = p.size[1], Lz = p.size[2], V = Lx * Ly * Lz;
    const double area[6] = {Ly * Lz, Ly * Lz, Lx * Lz, Lx * Lz, Lx * Ly, Lx * Ly};
    double S = 0.0, A = 0.0;
    for (int w = 0; w < 6; w++) {
        S += area[w];
        A += area[w] * (1.0 - (double)r.beta[w] * (double)r.beta[w]);
    }
    const double K = 24.0 * std::log(10.0) / p.speed;
    out[0] = (double)p.N;
    out[1] = (double)p.total;
    out[2] = (double)p.complete;
    out[3] = p.tau[0];
    out[4] = p.tau[1];
    out[5] = V;
    out[6] = A > 0.0 ? K * V / A : 0.0;
    out[7] = A > 0.0 ? K * V / (-S * std::log1p(-A / S)) : 0.0;  // (every wall fully absorbing: the logarithm is -inf and the time 0)
}

// Every field of the bands, in the struct's order (of beta and air the bands in use), against the session's rate, which
// room_check has looked at; no engine, no HIP; the message names the field.  Null when they are good.
inline const char* room_bands_check(const mc_ir_room_bands* b, uint32_t rate) {
    static thread_local char msg[200];
    if (!b) return "null bands";
    if (b->struct_size != sizeof(mc_ir_room_bands)) return "mc_ir_room_bands struct_size mismatch";
    msg[0] = 0;
    if (b->n_xovers > MC_DAMP_MAX_XOVERS) {
        std::snprintf(msg, sizeof(msg), "bands n_xovers %u above %d", b->n_xovers, MC_DAMP_MAX_XOVERS);
        return msg;
    }
    const double top = IEQ_MAX_NYQ * (double)rate;
    for (uint32_t k = 0; k < b->n_xovers; k++) {
        const double f = (double)b->xover_hz[k];
        if (!(std::isfinite(f) && f >= IEQ_MIN_HZ && f <= top)) {
            std::snprintf(msg, sizeof(msg), "bands xover_hz[%u] %g outside [%g, %g]", k, f, IEQ_MIN_HZ, top);
            return msg;
        }
        if (k && !(b->xover_hz[k] > b->xover_hz[k - 1])) {
            std::snprintf(msg, sizeof(msg), "bands xover_hz[%u] %g not above xover_hz[%u] %g: the crossovers must ascend strictly", k, f, k - 1,
                          (double)b->xover_hz[k - 1]);
            return msg;
        }
    }
    for (uint32_t j = 0; j <= b->n_xovers; j++)
        for (int w = 0; w < 6; w++)
            if (!(b->beta[j][w] >= -1.f && b->beta[j][w] <= 1.f)) {
                std::snprintf(msg, sizeof(msg), "bands beta[%u][%d] %g outside [-1, 1]", j, w, (double)b->beta[j][w]);
                return msg;
            }
    for (uint32_t j = 0; j <= b->n_xovers; j++)
        if (!(std::isfinite(b->air_db_per_m[j]) && b->air_db_per_m[j] >= 0.f && b->air_db_per_m[j] <= 1.f)) {
            std::snprintf(msg, sizeof(msg), "bands air_db_per_m[%u] %g outside [0, 1]", j, (double)b->air_db_per_m[j]);
            return msg;
        }
    if (b->flags) {
        std::snprintf(msg, sizeof(msg), "bands flags %u must be 0", b->flags);
        return msg;
    }
    if (b->reserved) {
        std::snprintf(msg, sizeof(msg), "bands reserved %u must be 0", b->reserved);
        return msg;
    }
    return nullptr;
}

// checked bands as the kernels take them: the room's plan once per band (with the microphones, when it has them), each with
// its band's powers of beta and air constant, and the crossovers
struct RoomBands {
    int B;
    RoomPlan plan[MC_DAMP_MAX_XOVERS + 1];
    RoomJoin join;
    double report[16];  // what mc_ir_room_bands_plan and mc_ir_room_bands_info hand out
};

// what mc_ir_room_bands_plan reports of checked bands in a checked room
inline void room_bands_report(const mc_ir_room& r, const mc_ir_room_bands& b, double out[16]) {
    const double Lx = (double)r.size_m[0], Ly = (double)r.size_m[1], Lz = (double)r.size_m[2], V = Lx * Ly * Lz;
    const double area[6] = {Ly * Lz, Ly * Lz, Lx * Lz, Lx * Lz, Lx * Ly, Lx * Ly};
    const double K = 24.0 * std::log(10.0) / (double)r.speed;
    std::fill(out, out + 16, 0.0);
    out[0] = (double)(b.n_xovers + 1);
    for (uint32_t k = 0; k < b.n_xovers; k++) out[1 + k] = (double)b.xover_hz[k];
    for (uint32_t j = 0; j <= b.n_xovers; j++) {
        double S = 0.0, A = 0.0;
        for (int w = 0; w < 6; w++) {
            S += area[w];
            A += area[w] * (1.0 - (double)b.beta[j][w] * (double)b.beta[j][w]);
        }
        const double air = 4.0 * ((double)b.air_db_per_m[j] * std::log(10.0) / 10.0) * V;
        const double sabine = A + air, eyring = -S * std::log1p(-A / S) + air;  // (every wall fully absorbing: inf, and the time 0)
        out[4 + j] = sabine > 0.0 ? K * V / sabine : 0.0;
        out[8 + j] = eyring > 0.0 ? K * V / eyring : 0.0;
    }
}

// `base` = the room's plan, its microphones in it when it has them
inline RoomBands room_bands_plan(const RoomPlan& base, const mc_ir_room& r, const mc_ir_room_bands& b, uint32_t rate) {
    RoomBands rb{};
    rb.B = (int)b.n_xovers + 1;
    rb.join.X = (int)b.n_xovers;
    for (int k = 0; k < rb.join.X; k++) rb.join.c[k] = ieq_coef(mc_eq_band{MC_EQ_HIGHCUT, b.xover_hz[k], 0.f, 0.70710678f}, rate);
    for (int j = 0; j < rb.B; j++) {
        RoomPlan& p = rb.plan[j];
        p = base;
        for (int w = 0; w < 6; w++)
            for (int q = 0; q < MC_ROOM_MAX_ORDER + 2; q++) p.bpow[w][q] = std::pow((double)b.beta[j][w], (double)q);
        p.air = (double)b.air_db_per_m[j] * std::log2(10.0) / 20.0;
    }
    room_bands_report(r, b, rb.report);
    return rb;
}

// frames up to which the lattice of order N is complete for a head of radius a: an image outside it is at least 2 N min(L) away
// and its sound reaches an ear at most a / c before d / c
inline double room_head_complete(const mc_ir_room& r, double a, uint32_t rate, double N) {
    return std::floor((2.0 * N * room_min_size(r) - a) * (double)rate / (double)r.speed);
}

// the order `order` 0 stands for with a head: the smallest N whose lattice is complete up to E (as a double: it may lie above
// MC_ROOM_MAX_ORDER)
inline double room_head_auto_order(const mc_ir_room& r, double a, uint32_t rate, uint64_t F) {
    double N = std::max(1.0, room_auto_order(r, rate, F));  // (the room's own is never too large, and at most one too small)
    while (room_head_complete(r, a, rate, N) < (double)room_last(r, F)) N += 1.0;
    return N;
}

// the head's centre to the source
inline double room_head_direct(const mc_ir_room& r) {
    double sq = 0.0;
    for (int ax = 0; ax < 3; ax++) {
        const double p = (double)r.source_m[ax] - (double)r.receiver_m[ax];
        sq += p * p;
    }
    return std::sqrt(sq);
}

// Every field of the head, then what follows from it in a room that room_check has passed, at the session's rate and F, and
// with the microphones (or null) that room_mics_check has passed; no engine, no HIP; the message names the field.  Null when
// it is good.
inline const char* room_head_check(const mc_ir_room_head* h, const mc_ir_room& r, const mc_ir_room_mics* mics, uint32_t rate, uint64_t F) {
    static thread_local char msg[240];
    if (!h) return "null head";
    if (h->struct_size != sizeof(mc_ir_room_head)) return "mc_ir_room_head struct_size mismatch";
    msg[0] = 0;
    const auto outside = [](const char* name, float v, double lo, double hi) {
        if (std::isfinite(v) && v >= (float)lo && v <= (float)hi) return false;  // (as floats: 0.05f and 0.15f are in)
        std::snprintf(msg, sizeof(msg), "head %s %g outside [%g, %g]", name, (double)v, lo, hi);
        return true;
    };
    if (outside("radius_m", h->radius_m, 0.05, 0.15)) return msg;
    if (outside("facing_az_deg", h->facing_az_deg, -360.0, 360.0)) return msg;
    if (outside("ear_deg", h->ear_deg, 60.0, 120.0)) return msg;
    if (outside("shadow", h->shadow, 0.0, 1.0)) return msg;
    if (h->flags) {
        std::snprintf(msg, sizeof(msg), "head flags %u must be 0", h->flags);
        return msg;
    }
    for (int k = 0; k < 2; k++)
        if (h->reserved[k]) {
            std::snprintf(msg, sizeof(msg), "head reserved[%d] %u must be 0", k, h->reserved[k]);
            return msg;
        }
    const double a = (double)h->radius_m, x = (double)r.speed / (a * (double)rate);
    if (!(x < 1.5)) {
        std::snprintf(msg, sizeof(msg), "head radius_m %g at rate %u: the head's corner lies above the rate (c / (a rate) = %g, not below 1.5)", a, rate, x);
        return msg;
    }
    const double direct = room_head_direct(r);
    if (!(direct >= a + ROOM_MIN_DIRECT)) {
        std::snprintf(msg, sizeof(msg), "source_m is %g m from the head's centre, below radius_m + %g = %g", direct, ROOM_MIN_DIRECT, a + ROOM_MIN_DIRECT);
        return msg;
    }
    double N = (double)r.order;
    if (!r.order) {
        N = room_head_auto_order(r, a, rate, F);
        if (!(N <= (double)MC_ROOM_MAX_ORDER)) {
            std::snprintf(msg, sizeof(msg), "order 0 needs order %.0f for %llu frames with a head, above %d: set last or order", N,
                          (unsigned long long)room_last(r, F), MC_ROOM_MAX_ORDER);
            return msg;
        }
    }
    const double images = 8.0 * (2.0 * N + 1.0) * (2.0 * N + 1.0) * (2.0 * N + 1.0);
    if (!(images * (double)r.gain / direct < ROOM_MAX_SUM)) {
        std::snprintf(msg, sizeof(msg), "gain %g: %.0f images of at most gain / %g m each may sum to 2^22 or more", (double)r.gain, images, direct);
        return msg;
    }
    if (mics)
        for (int c = 0; c < 2; c++)
            if (mics->mic_pattern[c] != 1.f) {
                std::snprintf(msg, sizeof(msg), "mic_pattern[%d] %g must be 1 with a head: ears are not microphones", c, (double)mics->mic_pattern[c]);
                return msg;
            }
    return nullptr;
}

// the head's high-pass at the session's rate
inline RoomShelf room_shelf(double a, double speed, double rate) {
    const double K = std::tan(speed / (a * rate)), b0 = 1.0 / (1.0 + K);
    return RoomShelf{K, b0, -b0, -(1.0 - K) / (1.0 + K)};
}

// A checked head into the plan of its room, before the microphones and the bands: both receivers at the centre, the ear axes,
// the order, the completeness and the ears' direct delays by the head's rules.  report = what mc_ir_room_head_plan and
// mc_ir_room_head_info hand out.
inline void room_plan_head(RoomPlan& p, const mc_ir_room& r, const mc_ir_room_head& h, double report[12]) {
    const double a = (double)h.radius_m, az = (double)h.facing_az_deg * M_PI / 180, ear = (double)h.ear_deg * M_PI / 180;
    p.N = r.order ? r.order : (uint32_t)room_head_auto_order(r, a, (uint32_t)p.rate, p.F);
    p.S = 2 * p.N + 1;
    p.total = 8u * p.S * p.S * p.S;
    p.complete = (uint64_t)room_head_complete(r, a, (uint32_t)p.rate, (double)p.N);
    for (int c = 0; c < 2; c++) {
        const double at = c ? az - ear : az + ear;
        p.head[3 * c] = std::cos(at), p.head[3 * c + 1] = std::sin(at), p.head[3 * c + 2] = 0.0;
        for (int ax = 0; ax < 3; ax++) p.rcv[c][ax] = (double)r.receiver_m[ax];
    }
    p.head[6] = a;
    p.head[7] = (double)h.shadow;
    p.headed = 1;
    const double px = p.src[0] - p.rcv[0][0], py = p.src[1] - p.rcv[0][1], pz = p.src[2] - p.rcv[0][2], d = std::sqrt(px * px + py * py + pz * pz);
    std::fill(report, report + 12, 0.0);
    for (int c = 0; c < 2; c++) {
        const double2 e = room_ear(p.head[3 * c], p.head[3 * c + 1], p.head[3 * c + 2], px, py, pz, d);
        p.tau[c] = std::fma(a, e.x, d) * p.rate / p.speed;
        report[2 + c] = p.tau[c];
        report[5 + c] = e.y * 180 / M_PI;
        report[7 + c] = room_shadow(p.head[7], e.y);
    }
    report[0] = (double)p.N;
    report[1] = (double)p.complete;
    report[4] = (p.tau[1] - p.tau[0]) / p.rate;
    report[9] = p.speed / (M_PI * a);
    report[10] = room_shelf(a, p.speed, p.rate).K;
}

// k_room over room's lattice into acc (room.A frames, zero) and kept (two zeroed counters)
inline hipError_t room_launch(hipStream_t stream, const RoomPlan& room, unsigned long long* d_acc, unsigned* d_kept) {
    const uint64_t waves = ((uint64_t)room.total + 63) / 64, per = ROOM_THREADS / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>((waves + per - 1) / per, ROOM_MAX_GRID);
    const bool air = room.air != 0.0;
    if (room.headed && room.mics && air)
        hipLaunchKernelGGL((k_room<true, true, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (room.headed && air)
        hipLaunchKernelGGL((k_room<false, true, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (room.headed && room.mics)
        hipLaunchKernelGGL((k_room<true, false, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (room.headed)
        hipLaunchKernelGGL((k_room<false, false, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (room.mics && air)
        hipLaunchKernelGGL((k_room<true, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (air)
        hipLaunchKernelGGL((k_room<false, true>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else if (room.mics)
        hipLaunchKernelGGL((k_room<true, false>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    else
        hipLaunchKernelGGL((k_room<false, false>), dim3(grid), dim3(ROOM_THREADS), 0, stream, d_acc, d_kept, room);
    return hipGetLastError();
}

// The join of the X + 1 accumulators at acc2 ([X + 1][A] pairs of int64) into d_r [F], X >= 1: the local pass, the carry and one
// fix-up per crossover, low to high.  d_st: 2 X cg.lanes double2, cg = chunk_geom(F).
inline hipError_t room_join(hipStream_t stream, const longlong2* acc2, uint64_t A, uint64_t F, const RoomJoin& join, const ChunkGeom& cg, double2* d_st,
                            double2* d_r) {
    const int X = join.X;
    hipLaunchKernelGGL(k_room_join<false>, dim3(cg.grid, X), dim3(IEQ_THREADS), 0, stream, acc2, A, F, join, 0, d_st, d_r);
    hipError_t er = hipGetLastError();
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_damp_carry, dim3(X), dim3(2 * IEQ_RUNS), 0, stream, d_st, cg.lanes, cg.nchunks, cg.K, damp_carry(join.c, X, cg.K));
        er = hipGetLastError();
    }
    for (int k = 0; k < X && er == hipSuccess; k++) {
        hipLaunchKernelGGL(k_room_join<true>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, acc2, A, F, join, k, d_st, d_r);
        er = hipGetLastError();
    }
    return er;
}

// room_generate and room_generate_bands for a room with a head: plans = the B band plans (B = 1 and X = 0 without bands), each
// headed.  One k_room per band into its own pair of accumulators, the plain ones [B][A] and behind them the shadow ones [B][A];
// with X crossovers the join of each block (rP into r, rS); the head's pass over the shadow accumulator or rS, which leaves
// r = S + the plain term; k_synth_room_bands.  One allocation holds the accumulators and the counters (zeroed with one memset),
// r, rS and the states, and is freed after the synth kernel.
inline hipError_t room_generate_head(hipStream_t stream, const SynPlan& syn, const RoomPlan* plans, int B, const RoomJoin* join, float2* d_x, uint32_t kept[2]) {
    const uint64_t A = plans[0].A, F = syn.F;
    const int X = join ? join->X : 0;
    const ChunkGeom cg = chunk_geom(F);
    const RoomShelf shelf = room_shelf(plans[0].head[6], plans[0].speed, plans[0].rate);
    const size_t block_bytes = sizeof(unsigned long long) * 2 * A * (size_t)B, zero_bytes = 2 * block_bytes + 16 * (size_t)B;  // (16: two counters, padded)
    const size_t r_bytes = sizeof(double2) * F * (X ? 2 : 1), st_bytes = sizeof(double2) * (size_t)std::max(2 * X, 1) * cg.lanes;
    DevArray<char> d_buf;
    hipError_t er = d_buf.alloc(zero_bytes + r_bytes + st_bytes);
    if (er != hipSuccess) return er;
    char* const d_all = d_buf;  // view
    unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(d_all);
    unsigned* d_kept = reinterpret_cast<unsigned*>(d_all + 2 * block_bytes);
    double2* d_r = reinterpret_cast<double2*>(d_all + zero_bytes);
    double2* d_rs = X ? d_r + F : nullptr;
    double2* d_st = reinterpret_cast<double2*>(d_all + zero_bytes + r_bytes);
    er = hipMemsetAsync(d_all, 0, zero_bytes, stream);
    for (int j = 0; j < B && er == hipSuccess; j++) {
        RoomPlan p = plans[j];
        p.shadow_at = 2 * A * (uint64_t)B;  // (from band j's plain accumulator to band j's shadow accumulator)
        er = room_launch(stream, p, d_acc + 2 * A * (size_t)j, d_kept + 4 * j);
    }
    const longlong2* plain = reinterpret_cast<const longlong2*>(d_acc);
    const longlong2* shadow = plain + A * (size_t)B;
    if (er == hipSuccess && X) er = room_join(stream, plain, A, F, *join, cg, d_st, d_r);
    if (er == hipSuccess && X) er = room_join(stream, shadow, A, F, *join, cg, d_st, d_rs);
    const longlong2 *in = X ? nullptr : shadow, *add = X ? nullptr : plain;
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_room_head<false>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, in, d_rs, add, A, F, shelf, d_st, d_r);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        const IeqCarry cm = ieq_carry(IeqCoef{shelf.b0, shelf.b1, 0.0, shelf.a1, 0.0}, cg.K);  // (a tap's matrix is the scalar -a1)
        hipLaunchKernelGGL(k_eq_carry, dim3(1), dim3(2 * IEQ_RUNS), 0, stream, d_st, cg.nchunks, cg.K, cm.M, cm.MK);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        hipLaunchKernelGGL(k_room_head<true>, dim3(cg.grid), dim3(IEQ_THREADS), 0, stream, in, d_rs, add, A, F, shelf, d_st, d_r);
        er = hipGetLastError();
    }
    if (er == hipSuccess) {
        const unsigned grid = (unsigned)((std::max<uint64_t>(F / 2, 1) + SYN_THREADS - 1) / SYN_THREADS);
        hipLaunchKernelGGL(k_synth_room_bands, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, d_r);
        er = hipGetLastError();
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (also after a failed launch: the memset may still be running)
    if (er == hipSuccess) er = waited;
    if (er == hipSuccess) er = hipMemcpy(kept, d_kept, 2 * sizeof(unsigned), hipMemcpyDeviceToHost);
    return er;
}

// room_generate for a banded room: one k_room per band into its own accumulator, the join, k_synth_room_bands.  One allocation
// holds the B accumulators and the counters (zeroed with one memset), r and the join's states; kept = band 0's counts (they
// are a matter of geometry and the same in every band).  With one band there is nothing to join: k_synth_room reads its
// accumulator.  With a head: room_generate_head.
inline hipError_t room_generate_bands(hipStream_t stream, const SynPlan& syn, const RoomBands& rb, float2* d_x, uint32_t kept[2]) {
    if (rb.plan[0].headed) return room_generate_head(stream, syn, rb.plan, rb.B, &rb.join, d_x, kept);
    const uint64_t A = rb.plan[0].A, F = syn.F;
    const int B = rb.B, X = rb.join.X;
    const ChunkGeom cg = chunk_geom(F);
    const size_t acc_bytes = sizeof(unsigned long long) * 2 * A * (size_t)B, zero_bytes = acc_bytes + 16 * (size_t)B;  // (16: two counters, padded)
    const size_t r_bytes = X ? sizeof(double2) * F : 0, st_bytes = sizeof(double2) * 2 * (size_t)X * cg.lanes;
    DevArray<char> d_buf;
    hipError_t er = d_buf.alloc(zero_bytes + r_bytes + st_bytes);
    if (er != hipSuccess) return er;
    char* const d_all = d_buf;  // view
    unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(d_all);
    unsigned* d_kept = reinterpret_cast<unsigned*>(d_all + acc_bytes);
    double2* d_r = reinterpret_cast<double2*>(d_all + zero_bytes);
    double2* d_st = reinterpret_cast<double2*>(d_all + zero_bytes + r_bytes);
    er = hipMemsetAsync(d_all, 0, zero_bytes, stream);
    for (int j = 0; j < B && er == hipSuccess; j++) er = room_launch(stream, rb.plan[j], d_acc + 2 * A * (size_t)j, d_kept + 4 * j);
    if (er == hipSuccess && X) er = room_join(stream, reinterpret_cast<const longlong2*>(d_acc), A, F, rb.join, cg, d_st, d_r);
    if (er == hipSuccess) {
        const unsigned grid = (unsigned)((std::max<uint64_t>(F / 2, 1) + SYN_THREADS - 1) / SYN_THREADS);
        if (X)
            hipLaunchKernelGGL(k_synth_room_bands, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, d_r);
        else
            hipLaunchKernelGGL(k_synth_room, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, reinterpret_cast<const long long*>(d_acc), A);
        er = hipGetLastError();
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (also after a failed launch: the memset may still be running)
    if (er == hipSuccess) er = waited;
    if (er == hipSuccess) er = hipMemcpy(kept, d_kept, 2 * sizeof(unsigned), hipMemcpyDeviceToHost);
    return er;
}

// The syn.F frames with the room's reflections into d_x (8-byte aligned), on `stream`, which is waited for: kept[c] = the
// images of channel c that arrive before frame E.  The accumulator lives only inside this call.  With a head: room_generate_head.
inline hipError_t room_generate(hipStream_t stream, const SynPlan& syn, const RoomPlan& room, float2* d_x, uint32_t kept[2]) {
    if (room.headed) return room_generate_head(stream, syn, &room, 1, nullptr, d_x, kept);
    DevArray<unsigned long long> d_buf;  // the accumulators, then the two counts (a word of 8 bytes)
    const size_t acc_bytes = sizeof(unsigned long long) * 2 * room.A;
    hipError_t er = d_buf.alloc(2 * room.A + 1);
    if (er != hipSuccess) return er;
    unsigned long long* const d_acc = d_buf;  // view
    unsigned* d_kept = reinterpret_cast<unsigned*>(d_acc + 2 * room.A);
    er = hipMemsetAsync(d_acc, 0, acc_bytes + 2 * sizeof(unsigned), stream);
    if (er == hipSuccess) er = room_launch(stream, room, d_acc, d_kept);
    if (er == hipSuccess) {
        const uint64_t pairs = syn.F / 2;
        const unsigned grid = (unsigned)((std::max<uint64_t>(pairs, 1) + SYN_THREADS - 1) / SYN_THREADS);
        hipLaunchKernelGGL(k_synth_room, dim3(grid), dim3(SYN_THREADS), 0, stream, d_x, syn, reinterpret_cast<const long long*>(d_acc), room.A);
        er = hipGetLastError();
    }
    const hipError_t waited = hipStreamSynchronize(stream);  // (also after a failed launch: the memset may still be running)
    if (er == hipSuccess) er = waited;
    if (er == hipSuccess) er = hipMemcpy(kept, d_kept, 2 * sizeof(unsigned), hipMemcpyDeviceToHost);
    return er;
}
