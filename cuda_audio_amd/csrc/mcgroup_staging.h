// mcgroup_staging.h - the group driver's staging (mcgroup.hip): four device arrays of [2][cap] frames per rank, grown together.
// Host only, over owned.h: tests/stub/owned_fake_hip.cpp runs the capacity rule against its fake of the runtime.
#pragma once
#include <cstdint>
#include <vector>

#include "owned.h"

struct RankStaging {
    int device = 0;
    hipStream_t stream = nullptr;  // view: the stream of the rank's engine
    DevArray<float> d_in, d_part, d_sum, d_out;
    static constexpr int kCreations = 4;
};
// Every rank (an R is a RankStaging) holds `frames` per channel.  cap reads 0 from before the first rank is touched until the last
// one has grown: after a failure midway no later, smaller batch passes for one that fits.
template <class R>
hipError_t ensure_staging(std::vector<R>& ranks, uint64_t& cap, uint64_t frames) {
    if (cap >= frames) return hipSuccess;
    cap = 0;
    for (RankStaging& k : ranks) {
        hipError_t er = hipSetDevice(k.device);
        for (DevArray<float>* a : {&k.d_in, &k.d_part, &k.d_sum, &k.d_out})
            if (er == hipSuccess) er = a->grow(2 * frames, k.stream);
        if (er != hipSuccess) return er;
    }
    cap = frames;
    return hipSuccess;
}
