// owned.h - the owners of GPU resources: a device array, a pinned host array, an event, a stream, and the three groups of them
// the engine makes on first use.  Host only, plain C++17 over <hip/hip_runtime_api.h>: no kernel, so tests/stub/owned_fake_hip.cpp
// compiles it with g++ against a counting fake of the runtime.
//
// The types enforce two conditions: a resource is freed exactly once, and a size lives with its pointer.  Nothing else belongs
// here (no allocator parameter, no pool, no sharing, no logging).  Every owner is move-only; a raw pointer or handle next to one
// is a view of it and says so in its comment.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <memory>
#include <utility>

template <class T>
class DevArray {
   public:
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevArray& operator=(DevArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevArray() { reset(); }

    hipError_t alloc(size_t n) {
        reset();
        const hipError_t er = hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n);
        return settle(er, n);
    }
    // fine-grained device memory (the BAR page the CPU writes through); hipFree releases it like any other
    hipError_t alloc_finegrained(size_t n) {
        reset();
        const hipError_t er = hipExtMallocWithFlags(reinterpret_cast<void**>(&p_), sizeof(T) * n, hipDeviceMallocFinegrained);
        return settle(er, n);
    }
    // n elements fit: nothing.  Otherwise whatever `stream` still does with the old array finishes first, and the contents go
    hipError_t grow(size_t n, hipStream_t stream) {
        if (n <= n_) return hipSuccess;
        const hipError_t er = hipStreamSynchronize(stream);
        if (er != hipSuccess) return er;
        return alloc(n);
    }
    hipError_t zero(hipStream_t stream) { return n_ ? hipMemsetAsync(p_, 0, sizeof(T) * n_, stream) : hipSuccess; }
    void adopt(T* p, size_t n) {
        reset();
        p_ = p;
        n_ = p ? n : 0;
    }
    T* release() {
        n_ = 0;
        return std::exchange(p_, nullptr);
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    size_t size() const { return n_; }
    T* get() const { return p_; }  // where a cast follows; everywhere else the conversion reads as the pointer did
    operator T*() const { return p_; }

   private:
    hipError_t settle(hipError_t er, size_t n) {
        if (er != hipSuccess) p_ = nullptr;
        n_ = p_ ? n : 0;
        return er;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};

// pinned host memory; dev() is the device-side address of a mapped one (hipHostMallocMapped), null otherwise
template <class T>
class PinnedArray {
   public:
    PinnedArray() = default;
    PinnedArray(PinnedArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), d_(std::exchange(o.d_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    PinnedArray& operator=(PinnedArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            d_ = std::exchange(o.d_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~PinnedArray() { reset(); }

    hipError_t alloc(size_t n, unsigned flags) {
        reset();
        hipError_t er = hipHostMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n, flags);
        if (er != hipSuccess) {
            p_ = nullptr;
            return er;
        }
        n_ = n;
        if (flags & hipHostMallocMapped) er = hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), p_, 0);
        if (er != hipSuccess) reset();
        return er;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = d_ = nullptr;
        n_ = 0;
    }
    size_t size() const { return n_; }
    T* dev() const { return d_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }

   private:
    T *p_ = nullptr, *d_ = nullptr;
    size_t n_ = 0;
};

class Event {
   public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            ev_ = std::exchange(o.ev_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }

    hipError_t create(unsigned flags) {
        reset();
        const hipError_t er = hipEventCreateWithFlags(&ev_, flags);
        if (er != hipSuccess) ev_ = nullptr;
        return er;
    }
    void reset() {
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }
    operator hipEvent_t() const { return ev_; }

   private:
    hipEvent_t ev_ = nullptr;
};

class Stream {
   public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            reset();
            s_ = std::exchange(o.s_, nullptr);
        }
        return *this;
    }
    ~Stream() { reset(); }

    hipError_t create(unsigned flags) {
        reset();
        const hipError_t er = hipStreamCreateWithFlags(&s_, flags);
        if (er != hipSuccess) s_ = nullptr;
        return er;
    }
    // everything issued on it has finished (nothing to wait for when there is no stream)
    hipError_t sync() const { return s_ ? hipStreamSynchronize(s_) : hipSuccess; }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    operator hipStream_t() const { return s_; }

   private:
    hipStream_t s_ = nullptr;
};

// ---- resources made on first use.  A group is built in a local and moved into its slot only when every piece exists: a slot is
// empty or whole, and a creation that failed midway leaves nothing behind and nothing to trip over on the next try.
template <class G, class... A>
hipError_t make_group(std::unique_ptr<G>& slot, A... args) {
    auto g = std::make_unique<G>();
    const hipError_t er = g->create(args...);
    if (er == hipSuccess) slot = std::move(g);
    return er;
}

// host-buffer batches with pinned caller memory: three sets of input staging, the copy-in stream, an event pair per set
struct PinnedStaging {
    DevArray<float> d_in[3][2];
    Stream h2d;
    Event ev_h2d[3], ev_comp[3];
    hipError_t create(size_t frames) {
        hipError_t er = h2d.create(hipStreamNonBlocking);
        for (int b = 0; b < 3 && er == hipSuccess; b++) {
            for (int i = 0; i < 2 && er == hipSuccess; i++) er = d_in[b][i].alloc(frames);
            if (er == hipSuccess) er = ev_h2d[b].create(hipEventDisableTiming);
            if (er == hipSuccess) er = ev_comp[b].create(hipEventDisableTiming);
        }
        return er;
    }
    static constexpr int kCreations = 13;
};

// overlap-save batches: the side stream of the small launches beside the three passes, and its events
struct OsSide {
    Stream stream;
    Event ev[3];
    hipError_t create() {
        hipError_t er = stream.create(hipStreamNonBlocking);
        for (int i = 0; i < 3 && er == hipSuccess; i++) er = ev[i].create(hipEventDisableTiming);
        return er;
    }
    static constexpr int kCreations = 4;
};

// kernel timing: a pool of event pairs and the kernels' own time stamps
struct KernelTiming {
    static constexpr int kPool = 1024;
    Event ev[kPool][2];
    DevArray<unsigned long long> d_stamps;
    hipError_t create(size_t stamps) {
        hipError_t er = hipSuccess;
        for (int i = 0; i < kPool && er == hipSuccess; i++) {
            er = ev[i][0].create(hipEventDefault);
            if (er == hipSuccess) er = ev[i][1].create(hipEventDefault);
        }
        if (er == hipSuccess) er = d_stamps.alloc(stamps);
        if (er == hipSuccess) er = hipMemset(d_stamps, 0, sizeof(unsigned long long) * stamps);
        return er;
    }
    static constexpr int kCreations = 2 * kPool + 1;
};
