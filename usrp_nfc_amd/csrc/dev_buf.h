// dev_buf.h -- growable buffers of the host side: DevBuf on the device, PinBuf in pinned host memory (nfc_amd.hip, nfc_multi.hip; the
// counter and the trace switch are per translation unit)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

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
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, bool keep = false, hipStream_t st = nullptr) {
        if (bytes <= cap) return hipSuccess;
        devbuf_allocs()++;
        if (devbuf_trace()) fprintf(stderr, "[nfc] device buffer %p: %zu -> %zu bytes asked for\n", (void *)this, cap, bytes);
        size_t ncap = std::max(bytes, cap + cap / 2);
        ncap = (ncap + 255) & ~(size_t)255;
        void *np = nullptr;
        hipError_t e = hipMalloc(&np, ncap);
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        if (p) (void)hipFree(p);
        p = np;
        cap = ncap;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

// the pinned twin: the same growth, nothing kept across it and nothing counted (a pinned buffer is staging)
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        size_t ncap = std::max(bytes, cap + cap / 2);
        ncap = (ncap + 255) & ~(size_t)255;
        void *np = nullptr;
        hipError_t e = hipHostMalloc(&np, ncap, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p) (void)hipHostFree(p);
        p = np;
        cap = ncap;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

}  // namespace
