// owned_fake_hip.cpp - test infrastructure: csrc/owned.h and csrc/mcgroup_staging.h alone, under -fsanitize=address,undefined (no HIP library, no GPU).
// The few runtime functions the header calls are defined here on malloc and a counter: every creation adds to `live`, every
// release takes one off, and `fail_at` makes the k-th creation from now fail (nothing is made then).  A leak, a double free and
// a memset past an array's end are the sanitizer's to find; the counts are checked here.  Prints "ok <checks>" or a diagnostic
// and exits non-zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cuda_audio_amd/csrc/mcgroup_staging.h"
#include "../../cuda_audio_amd/csrc/owned.h"

static long live = 0, made = 0, freed = 0, syncs = 0, fail_at = -1;
static long checks = 0, bad = 0;

static bool refuse() { return fail_at >= 0 && fail_at-- == 0; }
static hipError_t create(void** p, size_t bytes) {
    *p = nullptr;
    if (refuse()) return hipErrorOutOfMemory;
    if (bytes && !(*p = std::malloc(bytes))) return hipErrorOutOfMemory;
    if (*p) live++, made++;
    return hipSuccess;
}
static hipError_t destroy(void* p) {
    if (p) live--, freed++;
    std::free(p);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return create(p, bytes); }
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned) { return create(p, bytes); }
hipError_t hipFree(void* p) { return destroy(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return create(p, bytes); }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
    if (refuse()) return hipErrorInvalidValue;
    *d = h;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) { return destroy(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) { return create(reinterpret_cast<void**>(ev), 1); }
hipError_t hipEventDestroy(hipEvent_t ev) { return destroy(ev); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return create(reinterpret_cast<void**>(s), 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return destroy(s); }
hipError_t hipMemset(void* p, int v, size_t bytes) {
    std::memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
    std::memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    syncs++;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) bad++, fprintf(stderr, "line %d: %s (live %ld)\n", __LINE__, #cond, live); \
    } while (0)

// A group made on first use: a failure at any of its creations leaves nothing alive and the slot empty, and the next try, with
// nothing failing, makes exactly the group
template <class G, class... A>
static void group_rows(A... args) {
    for (int k = 0; k < G::kCreations; k++) {
        std::unique_ptr<G> slot;
        fail_at = k;
        CHECK(make_group(slot, args...) != hipSuccess);
        CHECK(fail_at == -1);  // (the k-th creation exists: kCreations counts them all)
        CHECK(live == 0 && !slot);
        CHECK(make_group(slot, args...) == hipSuccess);
        CHECK(slot && live == G::kCreations);
        slot.reset();
        CHECK(live == 0);
    }
    std::unique_ptr<G> slot;
    fail_at = G::kCreations;  // one past the last: nothing fails
    CHECK(make_group(slot, args...) == hipSuccess && live == G::kCreations);
    fail_at = -1;
}

int main() {
    {  // scope exit, reset, size, zero over the whole array
        DevArray<double> a;
        CHECK(!a && a.size() == 0);
        CHECK(a.alloc(100) == hipSuccess && a && a.size() == 100 && live == 1);
        CHECK(a.zero(nullptr) == hipSuccess);
        a.reset();
        CHECK(live == 0 && !a && a.size() == 0);
        CHECK(a.alloc(7) == hipSuccess && a.alloc(9) == hipSuccess && live == 1 && a.size() == 9);  // (alloc lets the old array go)
        PinnedArray<float> h;
        CHECK(h.alloc(16, hipHostMallocMapped) == hipSuccess && h.dev() == h.get() && h.size() == 16);
        PinnedArray<float> plain;
        CHECK(plain.alloc(16, hipHostMallocDefault) == hipSuccess && plain && !plain.dev());
        Event ev;
        Stream st;
        CHECK(ev.create(hipEventDisableTiming) == hipSuccess && st.create(hipStreamNonBlocking) == hipSuccess && live == 5);
        CHECK(st.sync() == hipSuccess && Stream().sync() == hipSuccess);
        DevArray<float> page;
        CHECK(page.alloc_finegrained(8192) == hipSuccess && page.size() == 8192 && live == 6);
    }
    CHECK(live == 0);
    {  // moves
        DevArray<int> a;
        CHECK(a.alloc(10) == hipSuccess);
        int* const p = a;
        DevArray<int> b(std::move(a));
        CHECK(!a && a.size() == 0 && b == p && b.size() == 10 && live == 1);
        DevArray<int> c;
        CHECK(c.alloc(3) == hipSuccess && live == 2);
        c = std::move(b);  // (what c held is freed)
        CHECK(live == 1 && c == p && c.size() == 10 && !b);
        DevArray<int>& self = c;
        c = std::move(self);
        CHECK(live == 1 && c == p && c.size() == 10);
        PinnedArray<int> h, h2;
        CHECK(h.alloc(4, hipHostMallocMapped) == hipSuccess);
        h2 = std::move(h);
        PinnedArray<int>& hs = h2;
        h2 = std::move(hs);
        CHECK(!h && !h.dev() && h2 && h2.dev() && h2.size() == 4 && live == 2);
        Event e1, e2;
        Stream s1, s2;
        CHECK(e1.create(0) == hipSuccess && s1.create(0) == hipSuccess);
        e2 = std::move(e1);
        s2 = std::move(s1);
        Event& es = e2;
        Stream& ss = s2;
        e2 = std::move(es);
        s2 = std::move(ss);
        Event e3(std::move(e2));
        Stream s3(std::move(s2));
        CHECK(!e1 && !e2 && e3 && !s1 && !s2 && s3 && live == 4);
    }
    CHECK(live == 0);
    {  // adopt and release
        DevArray<float> a, b;
        CHECK(a.alloc(5) == hipSuccess);
        float* const p = a.release();
        CHECK(p && !a && a.size() == 0 && live == 1);  // (the caller's now)
        CHECK(b.alloc(2) == hipSuccess && live == 2);
        b.adopt(p, 5);  // (what b held is freed)
        CHECK(b == p && b.size() == 5 && live == 1);
        b.adopt(nullptr, 9);
        CHECK(!b && b.size() == 0 && live == 0);
    }
    CHECK(live == 0);
    {  // grow
        DevArray<float> a;
        Stream st;
        CHECK(st.create(0) == hipSuccess && a.alloc(64) == hipSuccess);
        float* const p = a;
        long m = made, f = freed, s = syncs;
        CHECK(a.grow(64, st) == hipSuccess && a.grow(1, st) == hipSuccess && a.grow(0, st) == hipSuccess);
        CHECK(made == m && freed == f && syncs == s && a == p && a.size() == 64);  // fits: no call
        CHECK(a.grow(65, st) == hipSuccess);
        CHECK(made == m + 1 && freed == f + 1 && syncs == s + 1 && a.size() == 65);  // the stream waited for, one free, one allocation
        fail_at = 0;
        CHECK(a.grow(1000, st) != hipSuccess);
        CHECK(!a && a.size() == 0 && live == 1);  // (the stream is what lives)
        CHECK(a.grow(10, st) == hipSuccess && a.size() == 10);
        fail_at = 0;
        CHECK(a.alloc(20) != hipSuccess && !a && a.size() == 0);
        PinnedArray<float> h;
        fail_at = 1;  // the mapping fails after the allocation: the allocation goes
        CHECK(h.alloc(8, hipHostMallocMapped) != hipSuccess && !h && !h.dev() && h.size() == 0 && live == 1);
    }
    CHECK(live == 0);
    // the three groups the engine makes on first use
    group_rows<PinnedStaging>((size_t)4096);
    group_rows<OsSide>();
    group_rows<KernelTiming>((size_t)128);
    CHECK(live == 0);
    {  // the group driver's staging: the capacity reads 0 after a failure at any creation, and a smaller batch grows again
        const int n = 3;
        for (int k = 0; k < n * RankStaging::kCreations; k++) {
            std::vector<RankStaging> ranks(n);
            uint64_t cap = 0;
            CHECK(ensure_staging(ranks, cap, 256) == hipSuccess && cap == 256 && live == n * RankStaging::kCreations);
            long m = made;
            CHECK(ensure_staging(ranks, cap, 100) == hipSuccess && cap == 256 && made == m);
            fail_at = k;
            CHECK(ensure_staging(ranks, cap, 512) != hipSuccess);
            CHECK(cap == 0);
            CHECK(ensure_staging(ranks, cap, 100) == hipSuccess && cap == 100);
            for (const RankStaging& r : ranks) CHECK(r.d_in && r.d_part && r.d_sum && r.d_out && r.d_in.size() >= 200 && r.d_out.size() >= 200);
        }
    }
    CHECK(live == 0 && made == freed);
    if (bad) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
