// time_irphase.cpp — times the phase step of an IR load (csrc/irphase.hip.h) and its transform (csrc/fft64.hip.h) alone, with HIP
// events, outside the engine.  profiles/irphase.md records what it printed.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-unused-function -o time_irphase scripts/time_irphase.cpp && ./time_irphase [log2 F = 19] [over_log2 = 3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cuda_audio_amd/csrc/irphase.hip.h"
#include "../cuda_audio_amd/csrc/irdamp.hip.h"  // (irshape.hip.h declares what ireq.hip.h and this define)

#define TRY(x)                                                                              \
    do {                                                                                    \
        const hipError_t er_ = (x);                                                         \
        if (er_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(er_), __LINE__); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

int main(int argc, char** argv) {
    const int lgF = argc > 1 ? std::atoi(argv[1]) : 19, over = argc > 2 ? std::atoi(argv[2]) : 3;
    if (lgF < 0 || lgF > 21 || over < 1 || over > 6 || lgF + over > PH_MAX_LOG2) {
        std::fprintf(stderr, "log2 F in [0, 21], over_log2 in [1, 6], their sum at most %d\n", PH_MAX_LOG2);
        return 2;
    }
    const uint64_t F = 1ull << lgF;
    mc_ir_phase ph{(uint32_t)sizeof(mc_ir_phase), MC_PHASE_MINIMUM, 120.f, (uint32_t)over};
    const PhaseStep step = phase_step(ph, F);
    // decaying noise behind a delay (a linear congruential generator: the figures do not depend on the data)
    std::vector<float2> x(F);
    uint32_t s = 12345;
    for (uint64_t m = 0; m < F; m++) {
        const double env = m < F / 8 ? 0.0 : std::exp(-13.8 * (double)(m - F / 8) / (double)F * 2.0);
        s = s * 1664525u + 1013904223u;
        const float a = (float)(env * ((double)(s >> 8) / 8388608.0 - 1.0));
        s = s * 1664525u + 1013904223u;
        x[m] = make_float2(a, (float)(0.7 * env * ((double)(s >> 8) / 8388608.0 - 1.0)));
    }
    hipStream_t stream;
    hipEvent_t e0, e1;
    float2 *d_x = nullptr, *d_y = nullptr;
    TRY(hipStreamCreate(&stream));
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    TRY(hipMalloc(&d_x, sizeof(float2) * F));
    TRY(hipMalloc(&d_y, sizeof(float2) * F));
    TRY(hipMemcpy(d_x, x.data(), sizeof(float2) * F, hipMemcpyHostToDevice));
    double info[8];
    std::vector<float2> first(F), again(F);
    float best = 1e30f;
    for (int run = 0; run < 4; run++) {  // (the first run warms up)
        TRY(hipEventRecord(e0, stream));
        TRY(phase_run(stream, d_x, d_y, step, info));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        std::printf("phase step, run %d: %.3f ms\n", run, ms);
        if (run) best = std::min(best, ms);
        TRY(hipMemcpy((run ? again : first).data(), d_y, sizeof(float2) * F, hipMemcpyDeviceToHost));
        if (run && std::memcmp(first.data(), again.data(), sizeof(float2) * F)) {
            std::fprintf(stderr, "run %d stored other bits than run 0\n", run);
            return 1;
        }
    }
    std::printf("F %llu, Nfft %llu, passes %d: the step takes %.3f ms (allocations and four host round trips included); delay removed %.1f frames, "
                "E_out / E_in - 1 = %.3e, clamped %g and %g; every run stored the same bits\n",
                (unsigned long long)F, (unsigned long long)step.Nfft, step.fft.passes, best, info[4] - info[5], info[3] / info[2] - 1.0, info[6], info[7]);
    // the four transforms alone
    const uint64_t N = step.Nfft;
    double2 *d_a = nullptr, *d_w = nullptr;
    TRY(hipMalloc(&d_a, sizeof(double2) * N));
    TRY(hipMalloc(&d_w, sizeof(double2) * N));
    TRY(hipMemset(d_a, 0, sizeof(double2) * N));
    float fbest = 1e30f;
    for (int run = 0; run < 4; run++) {
        TRY(hipEventRecord(e0, stream));
        for (int t = 0; t < 4; t++) TRY(fft64_run(stream, step.fft, d_a, d_a, d_w, (t & 1) != 0));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        if (run) fbest = std::min(fbest, ms);
    }
    const double bytes = 4.0 * step.fft.passes * 2.0 * (double)N * 16.0;
    std::printf("four transforms alone: %.3f ms for %.1f MB that their passes must move = %.1f GB/s\n", fbest, bytes / 1e6, bytes / 1e6 / fbest);
    (void)hipFree(d_a);
    (void)hipFree(d_w);
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    return 0;
}
