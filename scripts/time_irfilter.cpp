// time_irfilter.cpp — times the filter step of an IR load (csrc/irfilter.hip.h) and its three transforms (csrc/fft64.hip.h) alone,
// with HIP events, outside the engine.  profiles/irfilter.md records what it printed.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-unused-function -o time_irfilter scripts/time_irfilter.cpp && ./time_irfilter [log2 Nfft = 20]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mcconv.h"
#include "../cuda_audio_amd/csrc/irfilter.hip.h"
#include "../cuda_audio_amd/csrc/irdamp.hip.h"  // (irshape.hip.h declares what ireq.hip.h and this define)

#define TRY(x)                                                                              \
    do {                                                                                    \
        const hipError_t er_ = (x);                                                         \
        if (er_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(er_), __LINE__); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

constexpr int RUNS = 8;  // the first warms up; the median of the other seven is reported

static float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const int lgN = argc > 1 ? std::atoi(argv[1]) : 20;
    if (lgN < 5 || lgN > FL_MAX_LOG2) {
        std::fprintf(stderr, "log2 Nfft in [5, %d]\n", FL_MAX_LOG2);
        return 2;
    }
    const uint64_t F = 1ull << (lgN - 1), G = F;  // F + G - 1 = Nfft - 1
    // decaying noise, the filter's first frame lifted (a linear congruential generator: the times do not depend on the data)
    std::vector<float2> x(F), b(G);
    uint32_t s = 12345;
    const auto noise = [&s](double env) {
        s = s * 1664525u + 1013904223u;
        return (float)(env * ((double)(s >> 8) / 8388608.0 - 1.0));
    };
    for (uint64_t m = 0; m < F; m++) {
        const double env = std::exp(-6.9 * (double)m / (double)F);
        x[m] = make_float2(noise(env), noise(0.7 * env));
        b[m] = make_float2(noise(env), noise(env / 3.0));
    }
    b[0].x += 64.f, b[0].y += 64.f;
    hipStream_t stream;
    hipEvent_t e0, e1;
    float2 *d_x = nullptr, *d_y = nullptr;
    TRY(hipStreamCreate(&stream));
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    TRY(hipMalloc(&d_x, sizeof(float2) * F));
    TRY(hipMalloc(&d_y, sizeof(float2) * (F + G - 1)));
    TRY(hipMemcpy(d_x, x.data(), sizeof(float2) * F, hipMemcpyHostToDevice));
    Fft64Plan plan{};
    for (uint32_t op : {(uint32_t)MC_FILTER_CONVOLVE, (uint32_t)MC_FILTER_DECONVOLVE}) {
        mc_ir_filter f{(uint32_t)sizeof(mc_ir_filter), op, MC_FILTER_STEREO, 0, 60.f, 0, 0};
        FilterStep step = filter_step(f, F, G);
        step.second = second_ir(&b[0].x, G, 0, 0);
        plan = step.fft;
        double info[10];
        std::vector<float2> first(step.Fo), again(step.Fo);
        std::vector<float> warm;
        for (int run = 0; run < RUNS; run++) {
            TRY(hipEventRecord(e0, stream));
            TRY(filter_run(stream, d_x, d_y, step, info));
            TRY(hipEventRecord(e1, stream));
            TRY(hipEventSynchronize(e1));
            float ms = 0.f;
            TRY(hipEventElapsedTime(&ms, e0, e1));
            std::printf("%s, run %d: %.3f ms\n", op == MC_FILTER_CONVOLVE ? "convolution" : "deconvolution", run, ms);
            if (run) warm.push_back(ms);
            TRY(hipMemcpy((run ? again : first).data(), d_y, sizeof(float2) * step.Fo, hipMemcpyDeviceToHost));
            if (run && std::memcmp(first.data(), again.data(), sizeof(float2) * step.Fo)) {
                std::fprintf(stderr, "run %d stored other bits than run 0\n", run);
                return 1;
            }
        }
        std::printf("%s: F %llu, G %llu, Fo %llu, Nfft %llu, passes %d: the step takes %.3f ms (median of %d warm runs; the filter's upload, the "
                    "allocations and the host round trips included); E_out / E_in = %.3e, E_rest / E_out = %.3e, regularised %g and %g; every run stored the same bits\n",
                    op == MC_FILTER_CONVOLVE ? "convolution" : "deconvolution", (unsigned long long)F, (unsigned long long)G, (unsigned long long)step.Fo,
                    (unsigned long long)step.Nfft, step.fft.passes, median(warm), RUNS - 1, info[6] / info[4], info[7] / info[6], info[8], info[9]);
    }
    // the three transforms alone
    const uint64_t N = 1ull << lgN;
    double2 *d_a = nullptr, *d_w = nullptr;
    TRY(hipMalloc(&d_a, sizeof(double2) * N));
    TRY(hipMalloc(&d_w, sizeof(double2) * N));
    TRY(hipMemset(d_a, 0, sizeof(double2) * N));
    std::vector<float> warm;
    for (int run = 0; run < RUNS; run++) {
        TRY(hipEventRecord(e0, stream));
        for (int t = 0; t < 3; t++) TRY(fft64_run(stream, plan, d_a, d_a, d_w, t == 2));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        if (run) warm.push_back(ms);
    }
    const double bytes = 3.0 * plan.passes * 2.0 * (double)N * 16.0;
    std::printf("three transforms alone (k_fft64_pass, %d launches): %.3f ms (median of %d warm runs) for %.1f MB that their passes must move = %.1f GB/s\n",
                3 * plan.passes, median(warm), RUNS - 1, bytes / 1e6, bytes / 1e6 / median(warm));
    (void)hipFree(d_a);
    (void)hipFree(d_w);
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    return 0;
}
