// dev_buf.h -- the owning handles of the host side.  Every HIP resource the library holds is held by one of them: DevBuf, a growable block
// of device memory; PinBuf, its twin in pinned host memory; Event; Stream, a stream the library created (never a caller's).  Each releases
// in its destructor, is never copied, moves without throwing (std::swap works) and hands out the raw HIP handle.  They are members and
// locals only -- none has static or namespace-scope storage: the HIP runtime may be gone when such a destructor runs at process exit, and
// the library keeps no HIP resource for the life of the process.  nfc::live::count: what the handles hold right now, per library (the test
// build hands it out: nfc_debug_live_resources).  The allocation counter and the trace switch are per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>

namespace nfc::live {
enum Kind : int { DEVICE = 0, PINNED = 1, EVENTS = 2, STREAMS = 3 };
inline std::atomic<uint64_t> &count(int kind) {
    static std::atomic<uint64_t> n[4];
    return n[kind];
}
}  // namespace nfc::live

namespace {

// (re)allocations of device buffers by the calling thread: a batch's share is nfc_stats.device_allocs -- a stream in its steady state
// must show 0 (an allocation in the middle of a stream costs milliseconds: VERDICT r4, the hovering stream's second batch)
inline uint64_t &devbuf_allocs() {
    static thread_local uint64_t n = 0;
    return n;
}
inline bool &devbuf_trace() {   // (test build: NFC_TRACE_ALLOC names every (re)allocation on stderr)
    static bool on = false;
    return on;
}

// an event or a stream with one owner: `h` is null or the owner's to release with FREE.  (Assignment swaps: what the target held goes
// with the source.)
template <class H, int KIND, hipError_t (*FREE)(H)>
struct Owner {
    H h = nullptr;
    Owner() = default;
    Owner(Owner &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owner &operator=(Owner &&o) noexcept { return std::swap(h, o.h), *this; }
    ~Owner() {
        if (h) (void)FREE(h), nfc::live::count(KIND)--;
    }
    operator H() const { return h; }

protected:
    hipError_t made(hipError_t r) {   // (of a create that found h null)
        if (r == hipSuccess) nfc::live::count(KIND)++;
        else h = nullptr;
        return r;
    }
};
// created on demand (a second create() is a no-op), gone with the handle
struct Event : Owner<hipEvent_t, nfc::live::EVENTS, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return h ? hipSuccess : made(hipEventCreateWithFlags(&h, flags)); }
};
struct Stream : Owner<hipStream_t, nfc::live::STREAMS, hipStreamDestroy> {   // (non-blocking, as every stream of the library's)
    hipError_t create() { return h ? hipSuccess : made(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); }
};

// what the two buffers share: the block, how it moves, its growth (by half at least, to a multiple of 256 bytes)
template <bool PIN>
struct Block {
    void *p = nullptr;
    size_t cap = 0;
    Block() = default;
    Block(Block &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Block &operator=(Block &&o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~Block() { release(); }
    void release() { adopt(nullptr, 0); }
    template <class T>
    T *as() const { return (T *)p; }

protected:
    size_t grown(size_t bytes) const { return (std::max(bytes, cap + cap / 2) + 255) & ~(size_t)255; }
    void adopt(void *fresh, size_t fresh_cap) {   // ... in the place of the block, which goes
        if (fresh) nfc::live::count(PIN ? nfc::live::PINNED : nfc::live::DEVICE)++;
        if (p) (void)(PIN ? hipHostFree(p) : hipFree(p)), nfc::live::count(PIN ? nfc::live::PINNED : nfc::live::DEVICE)--;
        p = fresh;
        cap = fresh_cap;
    }
};
struct DevBuf : Block<false> {
    hipError_t ensure(size_t bytes, bool keep = false, hipStream_t st = nullptr) {
        if (bytes <= cap) return hipSuccess;
        devbuf_allocs()++;
        if (devbuf_trace()) fprintf(stderr, "[nfc] device buffer %p: %zu -> %zu bytes asked for\n", (void *)this, cap, bytes);
        void *np = nullptr;
        hipError_t e = hipMalloc(&np, grown(bytes));
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        adopt(np, grown(bytes));
        return hipSuccess;
    }
};
// the pinned twin, made with the hipHostMalloc flags it was given: the same growth, nothing kept across it and nothing counted (a pinned
// buffer is staging)
struct PinBuf : Block<true> {
    unsigned flags = hipHostMallocDefault;
    PinBuf() = default;
    explicit PinBuf(unsigned host_malloc_flags) : flags(host_malloc_flags) {}
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        void *np = nullptr;
        const hipError_t e = hipHostMalloc(&np, grown(bytes), flags);
        if (e == hipSuccess) adopt(np, grown(bytes));
        return e;
    }
};

template <class H>
constexpr bool one_owner = !std::is_copy_constructible<H>::value && !std::is_copy_assignable<H>::value &&
                           std::is_nothrow_move_constructible<H>::value && std::is_nothrow_move_assignable<H>::value;
static_assert(one_owner<DevBuf> && one_owner<PinBuf> && one_owner<Event> && one_owner<Stream>, "handles move, without throwing, and are never copied");

}  // namespace
