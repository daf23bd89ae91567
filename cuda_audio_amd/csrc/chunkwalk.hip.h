// chunkwalk.hip.h — the walk of a workgroup over its chunks, shared by the chunked-recurrence kernels of the IR tools:
// k_eq_chunk (ireq.hip.h), k_damp_chunk (irdamp.hip.h), k_tail_chunk (irtail.hip.h), k_flr_band (irfloor.hip.h) and k_dec_sum
// (irdecay.hip.h).  No reference equivalent.  The host side of the measurements that launch them (the scratch, the origin, the
// order of a row group's launches) is irdecay.hip.h's Measure.
//
// The n taps of a buffer are cut into chunks of IEQ_CHUNK, a function of n alone; a lane owns one (chunk, channel) and runs a
// recurrence over its chunk's taps in order, first to last or last to first.  What the recurrence is, where a tap comes from and
// where it goes is the kernel's; how the taps reach the lane is here.
//
// Memory.  A lane walking its own chunk in global memory would put the lanes of a wave 4 KiB apart.  A workgroup (128 lanes: 64
// chunks x 2 channels, IEQ_SPAN taps) therefore stages IEQ_TILE taps of each of its chunks through LDS: 16 consecutive lanes
// move one chunk's 256 contiguous bytes, the next tile's loads fly under the current tile's arithmetic (registers), and the
// lanes read their own rows with ds_read_b64.  Rows are IEQ_TILE + 1 double2 long: lane (c, ch) reads dword 68 c + 4 k + 2 ch, so
// the 32 lanes of a half wave (c = 0 .. 15) fall on 32 different pairs of the 64 banks: no conflict.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int IEQ_CHUNK = 256;                                 // taps one lane filters
constexpr int IEQ_TILE = 16;                                   // taps of each chunk in LDS at a time
constexpr int IEQ_ROW = IEQ_TILE + 1;                          // double2 per LDS row (one of padding)
constexpr int IEQ_WG_CHUNKS = 64;                              // chunks per workgroup
constexpr int IEQ_THREADS = 2 * IEQ_WG_CHUNKS;                 // one lane per (chunk, channel)
constexpr int IEQ_SPAN = IEQ_WG_CHUNKS * IEQ_CHUNK;            // taps per workgroup
constexpr int IEQ_PER = IEQ_WG_CHUNKS * IEQ_TILE / IEQ_THREADS;  // double2 a lane moves per tile
constexpr int IEQ_RUNS = 128;                                  // runs of chunks per channel in the carry pass

// The walk of workgroup blockIdx.x (IEQ_THREADS lanes) over its IEQ_SPAN taps, a tile of every chunk at a time, the tiles
// first to last or, BACK, last to first, and the taps of a tile the same way.
//   load(g, v)   v = tap g as a Pre (double2, or float2 that is widened on its way into the tile), zero past the kernel's bound.
//                (Through v, not returned: a float2 a callable returns is passed as two integers, and taking them apart makes
//                every prefetch wait for its load on the spot.)
//   tap(v, m)    the lane's own tap m, in walk order; v is its place in the tile, and what is left there is what `store` gets;
//   store(g, v)  tap g of the result, a double2, under the kernel's bound.
// write: the tiles go back through `store` (the same for every lane of the workgroup; without it what `tap` leaves is dropped).
// UNROLL: the tap loop's unroll count (IEQ_TILE: all of it).
template <bool BACK, int UNROLL, class Pre, class Load, class Tap, class Store>
__device__ __forceinline__ void chunk_walk(bool write, Load&& load, Tap&& tap, Store&& store) {
    __shared__ double2 tile[IEQ_WG_CHUNKS * IEQ_ROW];
    constexpr int PHASES = IEQ_CHUNK / IEQ_TILE;
    const int t = threadIdx.x, c = t >> 1, ch = t & 1;
    const uint64_t base = (uint64_t)blockIdx.x * IEQ_SPAN;
    // element j of the lane's share of a tile: chunk i / IEQ_TILE, tap i % IEQ_TILE of it, i = t + j IEQ_THREADS
    Pre pre[IEQ_PER];
    const auto fetch = [&](int ph) {
#pragma unroll
        for (int j = 0; j < IEQ_PER; j++) {
            const int i = t + j * IEQ_THREADS;
            load(base + (uint64_t)(i / IEQ_TILE) * IEQ_CHUNK + ph * IEQ_TILE + i % IEQ_TILE, pre[j]);
        }
    };
    // BACK counts ph down itself, and its prefetch asks ph > 0: derived from a forward counter, ph costs k_dec_sum<true> 46 VGPRs
    constexpr int FIRST = BACK ? PHASES - 1 : 0, STEP = BACK ? -1 : 1;
    fetch(FIRST);
    for (int ph = FIRST; BACK ? ph >= 0 : ph < PHASES; ph += STEP) {
#pragma unroll
        for (int j = 0; j < IEQ_PER; j++) {
            const int i = t + j * IEQ_THREADS;
            tile[(i / IEQ_TILE) * IEQ_ROW + i % IEQ_TILE] = make_double2((double)pre[j].x, (double)pre[j].y);
        }
        __syncthreads();
        if (BACK ? ph > 0 : ph + 1 < PHASES) fetch(ph + STEP);
        double* row = reinterpret_cast<double*>(tile + c * IEQ_ROW) + ch;
        const uint64_t m0 = base + (uint64_t)c * IEQ_CHUNK + ph * IEQ_TILE;
#pragma unroll UNROLL
        for (int q = 0; q < IEQ_TILE; q++) {
            const int k = BACK ? IEQ_TILE - 1 - q : q;
            tap(row[2 * k], m0 + k);
        }
        __syncthreads();
        if (write) {
#pragma unroll
            for (int j = 0; j < IEQ_PER; j++) {
                const int i = t + j * IEQ_THREADS;
                const uint64_t g = base + (uint64_t)(i / IEQ_TILE) * IEQ_CHUNK + ph * IEQ_TILE + i % IEQ_TILE;
                store(g, tile[(i / IEQ_TILE) * IEQ_ROW + i % IEQ_TILE]);
            }
            __syncthreads();
        }
    }
}
