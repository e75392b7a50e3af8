// prune_select.h -- what the magnitude selects of kernels_prune.hip (over a matrix's stored terms)
// and kernels_dense.hip (over a dense matrix's elements) share: the key, the launch constants, the
// radix select's state and its pick step.  Device code; include from a .hip file only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kPThreads = 256;
constexpr int kPWaves = kPThreads / 64;
constexpr int64_t kPMaxBlocks = 2048;   // 256 CUs x 8; the rest by grid stride
constexpr int kPCopies = 16, kPCopyStride = 257;
constexpr unsigned kPHistBlocks = 1024;   // each workgroup ends in 256 global atomics: fewer, longer ones
constexpr uint32_t kKeyMask = 0x7FFFFFFFu;
static_assert(kSddmmChunk == 2 * 4 * kPThreads, "a chunk is two steps of four terms per thread");

inline unsigned p_grid(int64_t items, int64_t per_block = kPThreads) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, kPMaxBlocks));
}

#define P_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// The global select's state: the cut key (its decided high bytes while the passes run), what is
// still to be taken among the terms that match it, and the four passes' bins.
struct PruneState {
    uint32_t K;
    uint32_t r;
    uint32_t hist[4][256];
};

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// The digit, from 255 down, at which the running count of `bins` reaches `rem` (1 <= rem <= the
// bins' sum), by all 256 threads: thread t looks at digit 255 - t.  The one thread that finds it
// returns true with `digit` and `before`, the count of the greater digits.  One barrier inside;
// `wsum` is kPWaves words of LDS.
__device__ __forceinline__ bool pick_digit(const uint32_t *bins, uint32_t rem, uint32_t *wsum, uint32_t &digit,
                                           uint32_t &before) {
    const int t = threadIdx.x, lane = t & 63;
    digit = 255u - (uint32_t)t;
    const uint32_t v = bins[digit];
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[t >> 6] = inc;
    __syncthreads();
    for (int w = 0; w < (t >> 6); ++w) inc += wsum[w];
    before = inc - v;
    return before < rem && rem <= inc;
}

// One workgroup.  Pass 0 starts from `k` (1 <= k < the number of keys), the later ones from the state.
__global__ __launch_bounds__(kPThreads) void prune_pick_kernel(int pass, uint32_t k, PruneState *st) {
    __shared__ uint32_t wsum[kPWaves];
    const uint32_t rem = pass ? st->r : k;   // read by all before the barrier, written after it
    uint32_t digit, before;
    if (pick_digit(st->hist[pass], rem, wsum, digit, before)) {
        st->K |= digit << (24 - 8 * pass);
        st->r = rem - before;
    }
}

inline uint32_t float_key(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b & kKeyMask;
}

}  // namespace
}  // namespace smamd
