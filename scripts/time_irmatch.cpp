// time_irmatch.cpp — times the match step of an IR load (csrc/irmatch.hip.h), its five transforms (csrc/fft64.hip.h) alone and its
// smoothing kernel alone, with HIP events, outside the engine.  profiles/irmatch.md records what it printed.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-unused-function -o time_irmatch scripts/time_irmatch.cpp && ./time_irmatch [log2 Nfft ...]
// Without arguments: Nfft = 2^16, 2^20 and 2^22, F = G = Nfft / 2, the default grid at 48 kHz, linked, minimum phase.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mcconv.h"
#include "../cuda_audio_amd/csrc/irmatch.hip.h"
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

static int one_size(int lgN) {
    const uint64_t N = 1ull << lgN, F = N / 2, G = F;
    // decaying noise (a linear congruential generator: the times do not depend on the data)
    std::vector<float2> x(F), t(G);
    uint32_t s = 12345;
    const auto noise = [&s](double env) {
        s = s * 1664525u + 1013904223u;
        return (float)(env * ((double)(s >> 8) / 8388608.0 - 1.0));
    };
    float2 prev = make_float2(0.f, 0.f);
    for (uint64_t m = 0; m < F; m++) {
        const double env = std::exp(-6.9 * (double)m / (double)F);
        const float2 w = make_float2(noise(env), noise(0.7 * env));
        x[m] = make_float2(0.3f * w.x + 0.7f * prev.x, 0.3f * w.y + 0.7f * prev.y);  // (a one-pole colour to match away)
        prev = x[m];
        t[m] = make_float2(noise(env), noise(env / 3.0));
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
    mc_ir_match m;
    std::memset(&m, 0, sizeof(m));
    m.struct_size = (uint32_t)sizeof(m), m.mode = MC_MATCH_TARGET, m.phase = MC_MATCH_MINIMUM, m.link = 1, m.per_octave = 12;
    m.lo_hz = 20.0, m.octaves = 1.0 / 3.0, m.amount = 1.f, m.boost_db = 12.f, m.cut_db = 24.f, m.floor_db = 120.f;
    if (const char* bad = match_check(&m)) {
        std::fprintf(stderr, "%s\n", bad);
        return 1;
    }
    MatchStep step = match_step(m, 48000, F, G);
    step.second = second_ir(&t[0].x, G, 0, 48000);
    MatchFacts facts;
    std::vector<float2> first(step.Fo), again(step.Fo);
    std::vector<float> warm;
    for (int run = 0; run < RUNS; run++) {
        TRY(hipEventRecord(e0, stream));
        TRY(match_run(stream, d_x, d_y, step, &facts));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        std::printf("Nfft 2^%d, run %d: %.3f ms\n", lgN, run, ms);
        if (run) warm.push_back(ms);
        TRY(hipMemcpy((run ? again : first).data(), d_y, sizeof(float2) * step.Fo, hipMemcpyDeviceToHost));
        if (run && std::memcmp(first.data(), again.data(), sizeof(float2) * step.Fo)) {
            std::fprintf(stderr, "run %d stored other bits than run 0\n", run);
            return 1;
        }
    }
    double least = 0.0, most = 0.0;
    for (uint32_t j = 0; j < step.J; j++) least = std::min(least, facts.curve[3 * step.J + 2 * j]), most = std::max(most, facts.curve[3 * step.J + 2 * j]);
    std::printf("match: F %llu, G %llu, Nfft 2^%d, passes %d, J %u, %llu window bins per signal: the step takes %.3f ms (median of %d warm runs; the target's "
                "upload, the allocations and the host round trips included); gain %+.2f .. %+.2f dB, %g clamped, E_out / E_in = %.3e; every run stored the same bits\n",
                (unsigned long long)F, (unsigned long long)G, lgN, step.fft.passes, step.J, (unsigned long long)step.window_bins, median(warm), RUNS - 1, least, most,
                facts.info[11], facts.info[7] / facts.info[5]);
    // the five transforms alone: two forward, the cepstrum's inverse and forward, the last inverse
    double2 *d_a = nullptr, *d_w = nullptr, *d_P = nullptr, *d_S = nullptr;
    uint2* d_win = nullptr;
    TRY(hipMalloc(&d_a, sizeof(double2) * N));
    TRY(hipMalloc(&d_w, sizeof(double2) * N));
    TRY(hipMemset(d_a, 0, sizeof(double2) * N));
    warm.clear();
    for (int run = 0; run < RUNS; run++) {
        TRY(hipEventRecord(e0, stream));
        for (int k = 0; k < 5; k++) TRY(fft64_run(stream, step.fft, d_a, d_a, d_w, k == 2 || k == 4));
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        if (run) warm.push_back(ms);
    }
    const double bytes = 5.0 * step.fft.passes * 2.0 * (double)N * 16.0;
    std::printf("five transforms alone (k_fft64_pass, %d launches): %.3f ms (median of %d warm runs) for %.1f MB that their passes must move = %.1f GB/s\n",
                5 * step.fft.passes, median(warm), RUNS - 1, bytes / 1e6, bytes / 1e6 / median(warm));
    // the smoothing alone: both signals' windows over powers that are all ones
    const uint64_t stride = match_stride(step);
    std::vector<double2> ones(2 * stride, make_double2(1.0, 1.0));
    TRY(hipMalloc(&d_P, sizeof(double2) * 2 * stride));
    TRY(hipMalloc(&d_S, sizeof(double2) * 2 * step.J));
    TRY(hipMalloc(&d_win, sizeof(uint2) * step.J));
    TRY(hipMemcpy(d_P, ones.data(), sizeof(double2) * 2 * stride, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_win, step.win.data(), sizeof(uint2) * step.J, hipMemcpyHostToDevice));
    warm.clear();
    for (int run = 0; run < RUNS; run++) {
        TRY(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(k_mt_smooth, dim3(step.J, 2), dim3(MT_THREADS), 0, stream, (const double2*)d_P, stride, (const uint2*)d_win, step.J, N / 2, d_S);
        TRY(hipGetLastError());
        TRY(hipEventRecord(e1, stream));
        TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        TRY(hipEventElapsedTime(&ms, e0, e1));
        if (run) warm.push_back(ms);
    }
    std::vector<double2> S(2 * step.J);
    TRY(hipMemcpy(S.data(), d_S, sizeof(double2) * 2 * step.J, hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < step.J; j++)
        if (S[j].x != (double)(step.win[2 * j + 1] - step.win[2 * j] + 1) || S[step.J + j].y != S[j].x) {
            std::fprintf(stderr, "window %u of ones sums to %g and %g, not its %u bins\n", j, S[j].x, S[step.J + j].y, step.win[2 * j + 1] - step.win[2 * j] + 1);
            return 1;
        }
    const double loads = 2.0 * (double)step.window_bins;
    std::printf("k_mt_smooth alone (%u x 2 workgroups): %.3f ms (median of %d warm runs) for %.2e loads of 16 bytes = %.1f GB/s; every window of ones sums to its width\n",
                step.J, median(warm), RUNS - 1, loads, loads * 16.0 / 1e6 / median(warm));
    (void)hipFree(d_a);
    (void)hipFree(d_w);
    (void)hipFree(d_P);
    (void)hipFree(d_S);
    (void)hipFree(d_win);
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(stream);
    return 0;
}

int main(int argc, char** argv) {
    std::vector<int> sizes;
    for (int a = 1; a < argc; a++) sizes.push_back(std::atoi(argv[a]));
    if (sizes.empty()) sizes = {16, 20, 22};
    for (int lgN : sizes) {
        if (lgN < 5 || lgN > MT_MAX_LOG2) {
            std::fprintf(stderr, "log2 Nfft in [5, %d]\n", MT_MAX_LOG2);
            return 2;
        }
        if (const int rc = one_size(lgN)) return rc;
    }
    return 0;
}
