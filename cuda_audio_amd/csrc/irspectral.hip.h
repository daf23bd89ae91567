// irspectral.hip.h — what the three spectral steps of an impulse-response load (irphase.hip.h, irfilter.hip.h, irmatch.hip.h)
// share around their transforms (fft64.hip.h): the split of a packed spectrum into its two channels', the host arithmetic of
// their grids and transform lengths, the second impulse response of a filter or a match step, and the work buffers of a run.
#pragma once
#include <vector>

#include "fft64.hip.h"
#include "irshape.hip.h"
#include "resample.hip.h"

// the two channels' bins k of Z = FFT(x_L + i x_R), x real, from a = Z[k] and b = Z[N - k]:
// (Z[k] + conj Z[N - k]) / 2 and (Z[k] - conj Z[N - k]) / (2 i)
__device__ inline void fl_split(double2 a, double2 b, double2& l, double2& r) {
    l = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
    r = make_double2(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));
}

// workgroups of ISH_THREADS lanes that hold n elements, one each
inline uint64_t spec_groups(uint64_t n) { return (n + ISH_THREADS - 1) / ISH_THREADS; }

// log2 of the smallest power of two >= n that is not below 2^least; F64_MAX_LOG2 + 1 when n is beyond the longest transform,
// whatever n is (the loop ends there: no caller's length is trusted to have been bounded first)
inline int spec_ceil_log2(uint64_t n, int least = 0) {
    int lg = least;
    while (lg <= F64_MAX_LOG2 && (1ull << lg) < n) lg++;
    return lg;
}

// The second impulse response of a filter or a match step: `frames` host frames, interleaved, converted on the device from rs[0]
// to rs[1] Hz when they differ.
struct SecondIr {
    const float* lr = nullptr;
    uint64_t frames = 0;
    uint32_t rs[2] = {0, 0};
};

// `frames` host frames at `rate` Hz (0 = the session's) for a load at session_rate
inline SecondIr second_ir(const float* lr, uint64_t frames, uint32_t rate, uint32_t session_rate) {
    return SecondIr{lr, frames, {rate ? rate : session_rate, session_rate}};
}

// the frames at the session's rate of `frames` at `rate` Hz (0 = the session's; frames <= 2^40)
inline uint64_t second_frames_at(uint32_t rate, uint32_t session_rate, uint64_t frames) {
    return rate && rate != session_rate ? rs_out_frames(rs_geom(rate, session_rate), frames) : frames;
}

// its G frames at the session's rate into d
inline hipError_t second_upload(hipStream_t stream, const SecondIr& s, float2* d, uint64_t G) {
    double unused[4];
    return s.rs[0] != s.rs[1] ? rs_convert(stream, s.rs[0], s.rs[1], s.lr, s.frames, d, G, unused) : hipMemcpy(d, s.lr, sizeof(float2) * G, hipMemcpyHostToDevice);
}

// The work buffers of one run of a spectral step over a transform of N points: two spectra, a third that the transform works in
// when it has two passes, and a pair of partials per workgroup of N with their host copy.  Freed with the owner; a run that
// failed waits for the stream before it returns, so nothing is freed under a kernel.
struct SpectralWork {
    DevArray<double2> d_a, d_b, d_w;
    DevArray<double> d_part;
    std::vector<double> part;
    hipError_t alloc(const Fft64Plan& fft, uint64_t N) {
        part.resize(2 * (size_t)spec_groups(N));
        hipError_t er = d_a.alloc(N);
        if (er == hipSuccess) er = d_b.alloc(N);
        if (er == hipSuccess && fft.passes == 2) er = d_w.alloc(N);
        if (er == hipSuccess) er = d_part.alloc(part.size());
        return er;
    }
    // the first `count` partials, once the stream has run dry
    hipError_t fetch(hipStream_t stream, uint64_t count) {
        hipError_t er = hipGetLastError();
        if (er == hipSuccess) er = hipMemcpyAsync(part.data(), d_part, sizeof(double) * count, hipMemcpyDeviceToHost, stream);
        if (er == hipSuccess) er = hipStreamSynchronize(stream);
        return er;
    }
};

// what SpectralWork::alloc takes of the device
inline uint64_t spec_work_bytes(const Fft64Plan& fft, uint64_t N) { return (fft.passes == 2 ? 3 : 2) * 16 * N + 16 * spec_groups(N); }
