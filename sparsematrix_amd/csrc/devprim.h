// devprim.h -- what the device-side builders and constructors (builddev*.hip, transpose_dev.hip,
// refenc_dev.hip, kernels_prune / _dense / _sum.hip) share: the grid-stride launch shape, the error
// macros, the key width of a radix sort, and hipcub's sort and scan over DevScratch ("ask for the
// size, allocate, call again", once).  Device code; include from a .hip file only.
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "devmem.h"

namespace smamd {

// 256-thread workgroups for n items, at most 65536 of them: the rest by grid stride.
inline unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1 << 16)); }

#define GS_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// The two return conventions of the device-side code.  DEV_TRY: in a function that returns the
// C ABI's int and has a `hipError_t &err` -- a HIP error is -5 with err set.  DEV_TRY_RET: in a
// function that returns the hipError_t itself.
#define DEV_TRY(x)                 \
    do {                           \
        const hipError_t e_ = (x); \
        if (e_ != hipSuccess) {    \
            err = e_;              \
            return -5;             \
        }                          \
    } while (0)

#define DEV_TRY_RET(x)                   \
    do {                                 \
        const hipError_t e_ = (x);       \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// Bits that hold v, at least 1: the end_bit of a sort whose largest key is v.  (transpose_dev.hip
// keeps its own count with 0 bits for v == 0, where it skips the sort.)
inline int bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

// A stable radix sort of (k, v) into (ks, vs) over the low end_bit key bits; the temporary comes
// from `t`.  With release_tmp the call waits for the stream and frees the temporary before it
// returns: for the builders that hold several term-sized arrays across the sort.
template <class K, class V>
hipError_t dev_sort_pairs(DevScratch &t, const K *k, K *ks, const V *v, V *vs, int64_t n, int end_bit, hipStream_t s,
                          bool release_tmp = false) {
    size_t bytes = 0;
    DEV_TRY_RET(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k, ks, v, vs, (int)n, 0, end_bit, s));
    uint8_t *tmp = nullptr;
    DEV_TRY_RET(t.alloc(&tmp, (int64_t)bytes));
    DEV_TRY_RET(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k, ks, v, vs, (int)n, 0, end_bit, s));
    if (!release_tmp) return hipSuccess;
    DEV_TRY_RET(hipStreamSynchronize(s));
    t.release(tmp);
    return hipSuccess;
}

// out[i] = in[0] + ... + in[i - 1] for i < n; `in` any input iterator.
template <class In, class O>
hipError_t dev_excl_sum(DevScratch &t, In in, O *out, int64_t n, hipStream_t s) {
    size_t bytes = 0;
    DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, s));
    uint8_t *tmp = nullptr;
    DEV_TRY_RET(t.alloc(&tmp, (int64_t)bytes));
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, s);
}

// *out = max(*out, the largest v[i]); values >= 0, *out zeroed by the caller.  (A template so
// that every file that includes this header may hold it: launch max_i32_kernel<>.)
template <int NT = 256>
__global__ __launch_bounds__(NT) void max_i32_kernel(int64_t n, const int32_t *__restrict__ v, int32_t *__restrict__ out) {
    int32_t mx = 0;
    GS_LOOP(i, n) mx = max(mx, v[i]);
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, mx);
}

}  // namespace smamd
