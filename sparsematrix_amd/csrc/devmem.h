// devmem.h -- the one place that allocates and frees device memory for the library (but for
// multi.cpp's gather buffers, the C++ shim's operands and the growth of the AddMatMat
// workspace).  Two owners:
//   DevMem      what a matrix keeps: every buffer is recorded with its size, counted in `bytes`
//               (sm_info.device_bytes) and freed with the matrix; release() drops one early,
//               release_since() everything a dropped layout allocated.
//   DevScratch  what a call needs until it returns: freed at scope end.
// Both hand out raw typed pointers, so the launchers and the *Dev structs stay plain data.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

namespace smamd {

struct DevMem {
    struct Buf {
        void *p;
        int64_t bytes;
    };
    std::vector<Buf> bufs;
    int64_t bytes = 0;

    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { release_all(); }

    // `count` elements, at least one (an empty array still has an address).
    template <class T>
    hipError_t alloc(T **p, int64_t count) {
        const size_t n = (size_t)std::max<int64_t>(count, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void **)p, n);
        if (e != hipSuccess) return e;
        bufs.push_back(Buf{(void *)*p, (int64_t)n});
        bytes += (int64_t)n;
        return e;
    }

    // Frees the buffers, forgets them, takes their bytes off the count and nulls the pointers
    // (a null or unrecorded pointer is only nulled).
    template <class... T>
    void release(T *&...p) {
        (release_one((void *)p), ...);
        ((p = nullptr), ...);
    }

    // Undo for a layout that is tried and then dropped: release_since(mark()) frees every buffer
    // allocated after the mark (bufs is in allocation order) and takes its bytes off the count.
    // The caller resets the descriptor that held the pointers, and releases no buffer from before
    // the mark in between (that would shift it).
    size_t mark() const { return bufs.size(); }
    void release_since(size_t mark) {
        for (; bufs.size() > mark; bufs.pop_back()) {
            (void)hipFree(bufs.back().p);
            bytes -= bufs.back().bytes;
        }
    }

    // The caller makes the buffers' device current.
    void release_all() { release_since(0); }

private:
    void release_one(void *q) {
        if (!q) return;
        for (size_t i = 0; i < bufs.size(); ++i) {
            if (bufs[i].p != q) continue;
            (void)hipFree(q);
            bytes -= bufs[i].bytes;
            bufs.erase(bufs.begin() + (std::ptrdiff_t)i);
            return;
        }
    }
};

// Allocates for a host vector and copies it (an empty one: the one-element allocation, no copy).
template <class T>
hipError_t dev_upload(DevMem &mem, T **p, const std::vector<T> &h) {
    const hipError_t e = mem.alloc(p, (int64_t)h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// A codebook as the kernels index it: 256 floats, `table` in the first table_size, zero past
// them.  `table` null: only the zeros (the caller fills the table on the device).
inline hipError_t dev_upload_table(DevMem &mem, float **p, const float *table, int32_t table_size) {
    hipError_t e = mem.alloc(p, 256);
    if (e == hipSuccess) e = hipMemset(*p, 0, 256 * sizeof(float));
    if (e == hipSuccess && table && table_size > 0)
        e = hipMemcpy(*p, table, (size_t)table_size * sizeof(float), hipMemcpyHostToDevice);
    return e;
}

struct DevScratch {
    std::vector<void *> p;

    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() {
        for (void *q : p) (void)hipFree(q);
    }

    template <class T>
    hipError_t alloc(T **out, int64_t count) {
        *out = nullptr;
        const hipError_t e = hipMalloc((void **)out, (size_t)std::max<int64_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }

    // Early release of one buffer (the large builders drop what a later phase does not read).
    void release(void *q) {
        for (void *&x : p)
            if (x == q && q) {
                (void)hipFree(x);
                x = nullptr;
            }
    }
};

// The AddMatMat workspace is grown by sm_addmatmat and counted nowhere; the matrix frees it here.
inline void dev_free_uncounted(void *p) { (void)hipFree(p); }

}  // namespace smamd
