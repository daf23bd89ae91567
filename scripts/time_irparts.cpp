// time_irparts.cpp — times the parts step of an IR load (csrc/irparts.hip.h) with HIP events: the step alone, outside the engine,
// and one whole load through the engine with the step and without it.  profiles/irparts.md records what it printed.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-unused-function -o time_irparts scripts/time_irparts.cpp -Lcuda_audio_amd -lmcconv
//         -Wl,-rpath,$PWD/cuda_audio_amd && ./time_irparts [log2 F = 20]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mcconv.h"
#include "../cuda_audio_amd/csrc/irparts.hip.h"
#include "../cuda_audio_amd/csrc/irdamp.hip.h"  // (irshape.hip.h declares what ireq.hip.h and this define)

#define TRY(x)                                                                              \
    do {                                                                                    \
        const hipError_t er_ = (x);                                                         \
        if (er_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(er_), __LINE__); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)
#define MC(x)                                                                       \
    do {                                                                            \
        if ((x) != MC_OK) {                                                         \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, mc_last_error(), __LINE__); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

constexpr int RUNS = 6;  // the first allocates; the median of the other five is reported

static float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const int lgF = argc > 1 ? std::atoi(argv[1]) : 20;
    if (lgF < 8 || lgF > 22) {
        std::fprintf(stderr, "log2 F in [8, 22]\n");
        return 2;
    }
    const uint64_t F = 1ull << lgF;
    std::vector<float2> x(F);
    uint32_t s = 12345;
    const auto noise = [&s](double env) {
        s = s * 1664525u + 1013904223u;
        return (float)(env * ((double)(s >> 8) / 8388608.0 - 1.0));
    };
    for (uint64_t m = 0; m < F; m++) {
        const double env = 0.25 * std::exp(-6.9 * (double)m / (double)F);
        x[m] = make_float2(noise(env), noise(env / 3.0));
    }
    // all three parts on, both cross-fades, the tail 20 ms later at 48 kHz: three reads per output frame around the boundaries
    mc_ir_parts p;
    mc_default_ir_parts(&p);
    p.mode = MC_PARTS_ON;
    p.direct_end = 120, p.early_end = std::min<uint64_t>(3840, F / 2), p.xfade[0] = 16, p.xfade[1] = 256;
    p.delay[2] = 960, p.gain_db[1] = -4.f, p.width[1] = 0.5f, p.balance[2] = 0.25f;
    const PartsStep step = parts_step(p, F);
    hipStream_t stream;
    hipEvent_t e0, e1;
    float2 *d_x = nullptr, *d_y = nullptr;
    TRY(hipStreamCreate(&stream));
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    TRY(hipMalloc(&d_x, sizeof(float2) * F));
    TRY(hipMalloc(&d_y, sizeof(float2) * step.Fo));
    TRY(hipMemcpy(d_x, x.data(), sizeof(float2) * F, hipMemcpyHostToDevice));
    double info[10];
    std::vector<float2> first(step.Fo), again(step.Fo);
    std::vector<float> warm;
    for (int run = 0; run < RUNS; run++) {
        TRY(hipEventRecord(e0, stream));
        TRY(parts_run(stream, d_x, d_y, step, info));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        std::printf("step, run %d: %.3f ms\n", run, ms);
        if (run) warm.push_back(ms);
        TRY(hipMemcpy((run ? again : first).data(), d_y, sizeof(float2) * step.Fo, hipMemcpyDeviceToHost));
        if (run && std::memcmp(first.data(), again.data(), sizeof(float2) * step.Fo)) {
            std::fprintf(stderr, "run %d stored other bits than run 0\n", run);
            return 1;
        }
    }
    const double bytes = 8.0 * ((double)F * 2.0 + (double)step.Fo);  // k_pt_energy reads F frames, k_pt_mix reads about F and writes Fo
    std::printf("step: F %llu, Fo %llu: %.3f ms (median of %d runs after one that allocates; the allocation of the partials and the two host round trips "
                "included) for %.1f MB that the two kernels must move = %.1f GB/s; E_out / E_in = %.4f, lost %g; every run stored the same bits\n",
                (unsigned long long)F, (unsigned long long)step.Fo, median(warm), RUNS - 1, bytes / 1e6, bytes / 1e6 / median(warm),
                info[7] / (info[4] + info[5] + info[6]), info[9]);
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    // one whole load through the engine, the same shape (a fade over the last frame, so that both are shaped loads), with the step and without
    mc_config cfg;
    mc_default_config(&cfg);
    cfg.n_ref = 2 * F + 4096;
    cfg.max_batch = 8;
    mc_engine* e = nullptr;
    MC(mc_create(&cfg, &e));
    mc_ir_shape sh;
    mc_default_ir_shape(&sh);
    sh.fade_out = 1;
    hipStream_t es = (hipStream_t)mc_get_stream(e);
    for (int with = 0; with < 2; with++) {
        warm.clear();
        for (int run = 0; run < RUNS; run++) {
            TRY(hipEventRecord(e0, es));
            MC(mc_load_ir_parts(e, 0, &x[0].x, F, 1024, 0, 0, &sh, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, with ? &p : nullptr));
            TRY(hipEventRecord(e1, es));
            TRY(hipEventSynchronize(e1));
            float ms = 0.f;
            TRY(hipEventElapsedTime(&ms, e0, e1));
            if (run) warm.push_back(ms);
        }
        std::printf("load %s the step: F %llu: %.3f ms (median of %d loads after one that allocates)\n", with ? "with" : "without", (unsigned long long)F,
                    median(warm), RUNS - 1);
    }
    mc_destroy(e);
    return 0;
}
