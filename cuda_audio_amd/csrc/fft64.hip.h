// fft64.hip.h — a complex FFT in double for the IR tools: power-of-two lengths N = 2^4 .. 2^22, forward and inverse, data in
// device memory as double2.  No reference equivalent.  It is a load-time tool (irphase.hip.h is its first user, irfilter.hip.h its second, irmatch.hip.h its third): correctness
// and the same bits on every run come first; the engine's own float transforms (fft512.hip.h, ossave.hip.h) stay what they are.
//
// Four-step form.  S = 2^11: a sub-transform of up to S points runs in LDS in one workgroup.
//   N <= S        one pass: the N points are one sub-transform.
//   S < N <= S^2  two passes, N = N1 N2 with N1 = 2^floor(log2 N / 2) and N2 = N / N1 (N1 <= N2 <= S), n = n1 N2 + n2,
//                 k = k1 + N1 k2:
//     pass A  for every n2: the N1-point transform over n1 (stride N2), times the twiddle W_N^(n2 k1), stored at [k1 N2 + n2];
//     pass B  for every k1: the N2-point transform over n2 (contiguous), stored at [k1 + N1 k2]: the transpose is this store.
// The factorisation is a pure function of N; so are the grids.  Nothing depends on the device's CU count, there are no
// atomics and nothing is combined out of order: the same input stores the same bits on every run.
//
// A workgroup of 512 holds a tile of C sub-transforms ("columns") of L points, C L <= F64_TILE = 4096 double2 = 64 KB of LDS,
// and a table of L / 2 twiddles beside it (16 KB at most): two workgroups per CU.  C = min(F64_TILE / L, columns of the pass).
// The C columns are neighbours in memory on the strided side of either pass (n2 in pass A's load and store, k1 in pass B's
// store), so a row of the tile is 16 C contiguous bytes: whole 128-byte lines while L <= 512 (N <= 2^18 in balanced form),
// 64 bytes at L = 1024 and 32 bytes at L = 2048 (N = 2^21, 2^22), where eight columns of 2048 points would need 256 KB of LDS.
// There the neighbouring workgroups, which run at the same time, read the rest of each line; pass B's load reads every column
// contiguously.  A tile of 8192 points (128 KB, one workgroup per CU: 64-byte pieces at L = 2048, whole lines at 1024) was
// measured and is no faster at 2^20 or 2^22 points (profiles/irphase.md): the width of the pieces is not what bounds a pass.
//
// In LDS.  Column c's point r lies at c L + (r ^ ((r >> 4 ^ r >> 8 ^ c) & 15)): every access is one 16-byte (b128) access, and
// the XOR only permutes the 16 slots of an aligned run of 16 points, so
//   - a radix-2 stage with half-size s >= 16 has 16 consecutive lanes on 16 consecutive points: 16 distinct slots;
//   - the last four stages (s = 8 .. 1) run in registers on 16 consecutive points per lane; lane q's m-th point lies in slot
//     m ^ q ^ (constant over 16 lanes): distinct;
//   - the tile's rows come in and go out with c fastest (distinct by ^ c) and the bit-reversed read of the store differs in
//     r >> 8 or r >> 4 between neighbouring k.
// (The hardware serves a b128 read in 16-lane groups that are not runs of consecutive lanes, so a group can straddle two
// runs whose constants differ; that costs at most one extra cycle on such a group.)
//
// The transform inside a tile is decimation in frequency, radix 2, in place: natural order in, bit-reversed order in LDS,
// natural order out through the store's index.  Twiddles come from sincospi in double on arguments that are exact in double;
// the engine's float tables are not read.  A workgroup computes W_L^m = sincospi(m / (L / 2)), m < L / 2, once into LDS, and the
// stage with half-size s reads every (L / 2 s)-th of them (W_2s^j = W_L^(j L / 2 s): the same argument j / s and so the same
// twiddle as computing it in the butterfly, a tenth faster over the whole transform); the last four stages take theirs from
// constants, and the twiddle between the passes is sincospi(2 ((n2 k1) mod N) / N) in the store.  The inverse conjugates the
// twiddles and scales by 1 / N (a power of two: exact) in its last store.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

constexpr int F64_S_LOG2 = 11;                   // S = 2048
constexpr int F64_MIN_LOG2 = 4, F64_MAX_LOG2 = 2 * F64_S_LOG2;
constexpr int F64_TILE_LOG2 = 12, F64_TILE = 1 << F64_TILE_LOG2;  // double2 per workgroup
constexpr int F64_THREADS = 512;

// one pass: `cols` sub-transforms of 2^lgL points, 2^lgC of them per workgroup.  Column c's point r is read at
// in[r in_r + c in_c] and its bin k stored at out[k out_r + c out_c].
struct Fft64Pass {
    int lgL, lgC;
    uint32_t cols;
    uint64_t in_r, in_c, out_r, out_c;
    int load_c_fast;  // lanes run over c first when loading (the strided side has c contiguous); else over r
    int twiddle;      // multiply bin k of column c by W_N^(c k) (pass A)
};

struct Fft64Plan {
    int lgN, passes;
    Fft64Pass p[2];
};

// the plan of N = 2^lgN, F64_MIN_LOG2 <= lgN <= F64_MAX_LOG2 (the caller checks)
inline Fft64Plan fft64_plan(int lgN) {
    Fft64Plan pl{};
    pl.lgN = lgN;
    if (lgN <= F64_S_LOG2) {
        pl.passes = 1;
        pl.p[0] = Fft64Pass{lgN, 0, 1u, 1, 0, 1, 0, 0, 0};
        return pl;
    }
    const int lg1 = lgN / 2, lg2 = lgN - lg1;
    const uint64_t N1 = 1ull << lg1, N2 = 1ull << lg2;
    pl.passes = 2;
    pl.p[0] = Fft64Pass{lg1, std::min(F64_TILE_LOG2 - lg1, lg2), (uint32_t)N2, N2, 1, N2, 1, 1, 1};
    pl.p[1] = Fft64Pass{lg2, std::min(F64_TILE_LOG2 - lg2, lg1), (uint32_t)N1, 1, N2, N1, 1, 0, 0};
    return pl;
}

__device__ inline uint32_t f64_at(uint32_t c, uint32_t r, int lgL) { return (c << lgL) + (r ^ (((r >> 4) ^ (r >> 8) ^ c) & 15u)); }

__device__ inline double2 f64_mul(double2 a, double cs, double sn) { return make_double2(a.x * cs - a.y * sn, a.x * sn + a.y * cs); }

// One pass.  Workgroup b transforms columns [b 2^lgC, (b + 1) 2^lgC).  in == out is allowed when every workgroup stores
// where it loaded (one pass; pass A): all loads of a workgroup come before its first store.
template <bool INV>
__global__ __launch_bounds__(F64_THREADS) void k_fft64_pass(const double2* in, double2* out, Fft64Pass p, int lgN, double scale) {
    __shared__ double2 t[F64_TILE];
    __shared__ double2 tw[1 << (F64_S_LOG2 - 1)];  // W_L^m, m < L / 2: every LDS stage's twiddles (stage s reads every (L / 2 s)-th)
    const int lgL = p.lgL, lgC = p.lgC;
    const uint32_t L = 1u << lgL, C = 1u << lgC, n = L << lgC;
    const uint64_t c0 = (uint64_t)blockIdx.x << lgC;
    for (uint32_t i = threadIdx.x; i < n; i += F64_THREADS) {
        const uint32_t c = p.load_c_fast ? i & (C - 1) : i >> lgL, r = p.load_c_fast ? i >> lgC : i & (L - 1);
        t[f64_at(c, r, lgL)] = in[(uint64_t)r * p.in_r + (c0 + c) * p.in_c];
    }
    for (uint32_t m = threadIdx.x; m < L / 2; m += F64_THREADS) {
        double sn, cs;
        sincospi((double)m / (double)(L / 2), &sn, &cs);
        tw[m] = make_double2(cs, INV ? sn : -sn);
    }
    __syncthreads();
    // stages with half-size s = L / 2 .. 16 through LDS
    for (int lgs = lgL - 1; lgs >= 4; lgs--) {
        const uint32_t s = 1u << lgs;
        for (uint32_t i = threadIdx.x; i < n / 2; i += F64_THREADS) {
            const uint32_t c = i >> (lgL - 1), q = i & (L / 2 - 1), j = q & (s - 1);
            const uint32_t r0 = ((q >> lgs) << (lgs + 1)) + j, i0 = f64_at(c, r0, lgL), i1 = f64_at(c, r0 + s, lgL);
            const double2 a = t[i0], b = t[i1];
            const double2 w = tw[j << (lgL - 1 - lgs)];  // W_2s^j = W_L^(j L / 2 s)
            t[i0] = make_double2(a.x + b.x, a.y + b.y);
            t[i1] = f64_mul(make_double2(a.x - b.x, a.y - b.y), w.x, w.y);
        }
        __syncthreads();
    }
    // stages s = 8 .. 1 in registers, 16 consecutive points per lane (L >= 16)
    for (uint32_t i = threadIdx.x; i < n / 16; i += F64_THREADS) {
        const uint32_t c = i >> (lgL - 4), r = (i & (L / 16 - 1)) << 4;
        // cos and sin of pi j / 8
        const double wc[8] = {1.0, 0.92387953251128674, 0.70710678118654752, 0.38268343236508977, 0.0, -0.38268343236508977, -0.70710678118654752, -0.92387953251128674};
        const double ws[8] = {0.0, 0.38268343236508977, 0.70710678118654752, 0.92387953251128674, 1.0, 0.92387953251128674, 0.70710678118654752, 0.38268343236508977};
        double2 v[16];
#pragma unroll
        for (int m = 0; m < 16; m++) v[m] = t[f64_at(c, r + m, lgL)];
#pragma unroll
        for (int lgs = 3; lgs >= 0; lgs--) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int s = 1 << lgs, j = q & (s - 1), r0 = ((q >> lgs) << (lgs + 1)) + j, w = j << (3 - lgs);
                const double2 a = v[r0], b = v[r0 + s];
                v[r0] = make_double2(a.x + b.x, a.y + b.y);
                v[r0 + s] = f64_mul(make_double2(a.x - b.x, a.y - b.y), wc[w], INV ? ws[w] : -ws[w]);
            }
        }
#pragma unroll
        for (int m = 0; m < 16; m++) t[f64_at(c, r + m, lgL)] = v[m];
    }
    __syncthreads();
    // bin k lies at the bit-reversed point
    const uint64_t Nmask = (1ull << lgN) - 1;
    const double inv_half_N = 2.0 / (double)(1ull << lgN);
    for (uint32_t i = threadIdx.x; i < n; i += F64_THREADS) {
        const uint32_t c = i & (C - 1), k = i >> lgC;
        double2 v = t[f64_at(c, __brev(k) >> (32 - lgL), lgL)];
        if (p.twiddle) {
            double sn, cs;
            sincospi((double)(((c0 + c) * k) & Nmask) * inv_half_N, &sn, &cs);
            v = f64_mul(v, cs, INV ? sn : -sn);
        }
        out[(uint64_t)k * p.out_r + (c0 + c) * p.out_c] = make_double2(v.x * scale, v.y * scale);
    }
}

// The transform of pl's N points `in` into `out` on the stream.  `work` (N points) is needed when pl.passes == 2 and must be
// neither in nor out; in == out is allowed.  The inverse includes the 1 / N.
inline hipError_t fft64_run(hipStream_t stream, const Fft64Plan& pl, const double2* in, double2* out, double2* work, bool inverse) {
    for (int a = 0; a < pl.passes; a++) {
        const Fft64Pass& p = pl.p[a];
        const bool last = a + 1 == pl.passes;
        const double2* src = a ? work : in;
        double2* dst = last ? out : work;
        const double scale = inverse && last ? 1.0 / (double)(1ull << pl.lgN) : 1.0;
        const dim3 grid(p.cols >> p.lgC);
        if (inverse)
            hipLaunchKernelGGL(k_fft64_pass<true>, grid, dim3(F64_THREADS), 0, stream, src, dst, p, pl.lgN, scale);
        else
            hipLaunchKernelGGL(k_fft64_pass<false>, grid, dim3(F64_THREADS), 0, stream, src, dst, p, pl.lgN, scale);
        const hipError_t er = hipGetLastError();
        if (er != hipSuccess) return er;
    }
    return hipSuccess;
}
