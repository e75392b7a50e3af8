// kernels_prune.hip -- pruning a matrix's stored terms by magnitude: the selection behind
// sm_prune_mask and the compaction behind sm_create_masked (DESIGN.md "Pruning the terms").
//
// The key of a value is its bits without the sign, compared as an unsigned integer; every rule of
// include/sparsematrix.h is a statement about keys and CSR indices, so every kernel here works on
// integers and the mask is a function of the values alone.
//
//   hist / pick    SM_PRUNE_GLOBAL_TOPK: a radix select over the key's four bytes, most significant
//                  first.  hist counts, per workgroup in LDS (16 copies of the 256 bins, a copy per
//                  lane group, at a stride of 257 words so that the copies of one bin lie in
//                  different banks) and then into the state's 256 global bins, the digit of every
//                  term whose higher bytes equal the prefix found so far; pick (one workgroup) scans
//                  the bins from 255 down, finds the digit at which the running count reaches what
//                  is still to be taken, and leaves the longer prefix and the rest in the state: no
//                  host round trip between the passes.  After four passes: the cut key K and r, the
//                  number of terms with key == K to keep.
//   equals / flag  per chunk of kSddmmChunk terms the number of keys == K; after an exclusive scan
//                  of the chunk counts, flag keeps a term iff key > K, or key == K and its rank
//                  among the equal-keyed terms in CSR order (the chunk's base + a ballot prefix) is
//                  below r.  Thread t of a step owns four consecutive terms: one 16-byte load, one
//                  32-bit store of four mask bytes where `keep` is 4-byte aligned, byte stores
//                  otherwise and for the last nnz % 4 terms (the shape of quantize_assign_kernel).
//   threshold      keep iff key >= key(threshold), the same loads and stores.
//   row (wave)     SM_PRUNE_ROW_TOPK, rows of at most 64 terms: one wavefront per row, lane i holds
//                  term i, its rank is the number of lanes that beat it (key greater, or equal in a
//                  lower lane), found by a broadcast loop over the row's lanes.  A wavefront takes
//                  four consecutive rows at a time and, where all four hold at most 16 terms, ranks
//                  them side by side in its four groups of 16 lanes (one wavefront per 16-term row
//                  left 48 lanes idle and was latency-bound: 610 us against 374 on config 2's
//                  shape).  Longer rows are appended to a list (an integer atomic counter: the
//                  list's order does not reach the mask).
//   row (group)    one workgroup per listed row: the same four-pass radix select on one LDS
//                  histogram over the row's terms, then the same tie ranking by ballots, 256 terms
//                  a step.  No thread walks a row alone.
//   positions      an exclusive scan (hipCUB) of the mask over nnz + 1 positions: every kept term's
//                  new index, and the new nnz at the end;
//   row_ptr        new_rp[r] = pos[old_rp[r]];
//   scatter        one pass writes the kept terms' columns, value bits, source indices and ids.
//
// Integer atomics only (LDS and global counters: counts are exact, their order reaches nothing);
// every launch geometry is a function of nnz and n_rows alone; every kernel strides over its
// terms, chunks or rows with a capped grid.
#include <algorithm>
#include <cstring>

#include "devprim.h"
#include "prune_select.h"
#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kRowBundle = 4;           // rows a wavefront of the row kernel takes at a time

// The workgroup's sum of a per-thread count into *part, by all threads (one barrier).  Every
// workgroup owns one slot and the host adds them: thousands of atomics on one address from eight
// XCDs were most of the threshold kernel's 108 us.
__device__ __forceinline__ void store_kept(uint32_t mine, uint32_t *part) {
    __shared__ uint32_t wkept[kPWaves];
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0) wkept[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) *part = wkept[0] + wkept[1] + wkept[2] + wkept[3];
}

// Four mask bytes (one per bit 0..3 of `bits`) for the terms [e, e + 4), e a multiple of 4.
template <bool PACKED>
__device__ __forceinline__ void store_keep4(uint8_t *keep, int64_t e, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    if (PACKED) {
        *reinterpret_cast<uint32_t *>(keep + e) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
        keep[e] = (uint8_t)b0;
        keep[e + 1] = (uint8_t)b1;
        keep[e + 2] = (uint8_t)b2;
        keep[e + 3] = (uint8_t)b3;
    }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPThreads) void prune_hist_kernel(int64_t nnz, const uint32_t *__restrict__ val, int pass,
                                                               PruneState *st) {
    __shared__ uint32_t h[kPCopies * kPCopyStride];
    for (int i = threadIdx.x; i < kPCopies * kPCopyStride; i += kPThreads) h[i] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass ? ~((1u << (shift + 8)) - 1u) : 0u;
    const uint32_t prefix = st->K;   // the undecided bytes are zero
    uint32_t *my = h + (threadIdx.x & (kPCopies - 1)) * kPCopyStride;
    auto take = [&](uint32_t bits) {
        const uint32_t key = bits & kKeyMask;
        if ((key & himask) == prefix) atomicAdd(&my[(key >> shift) & 255u], 1u);
    };
    const int64_t n4 = nnz >> 2;
    const uint4 *val4 = reinterpret_cast<const uint4 *>(val);
    P_LOOP(i, n4) {
        const uint4 v = val4[i];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    P_LOOP(j, nnz - (n4 << 2)) take(val[(n4 << 2) + j]);
    __syncthreads();
    uint32_t c = 0;
    for (int k = 0; k < kPCopies; ++k) c += h[k * kPCopyStride + threadIdx.x];
    if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);
}

// The keys of a step's four terms of thread `t` ([e, e + 4), e a multiple of 4) and which exist.
__device__ __forceinline__ void load_keys4(const uint32_t *__restrict__ val, int64_t e, int64_t nnz, uint32_t key[4],
                                           bool live[4]) {
    if (e + 4 <= nnz) {
        const uint4 v = *reinterpret_cast<const uint4 *>(val + e);
        key[0] = v.x & kKeyMask, key[1] = v.y & kKeyMask, key[2] = v.z & kKeyMask, key[3] = v.w & kKeyMask;
        live[0] = live[1] = live[2] = live[3] = true;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            live[j] = e + j < nnz;
            key[j] = live[j] ? val[e + j] & kKeyMask : 0u;
        }
    }
}

__global__ __launch_bounds__(kPThreads) void prune_equals_kernel(int64_t nnz, int64_t n_chunks,
                                                                 const uint32_t *__restrict__ val,
                                                                 const PruneState *__restrict__ st,
                                                                 int32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kPWaves];
    const uint32_t K = st->K;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        uint32_t mine = 0;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            uint32_t key[4];
            bool live[4];
            load_keys4(val, c * kSddmmChunk + it * (4 * kPThreads) + 4 * (int64_t)threadIdx.x, nnz, key, live);
#pragma unroll
            for (int j = 0; j < 4; ++j) mine += live[j] && key[j] == K;
        }
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) cnt[c] = (int32_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        __syncthreads();
    }
}

// keep iff key > K, or key == K and the term's rank among the equal-keyed terms is below r.
// `st` null: K and r are the arguments (every term, or none: no select ran) and `base` is not read.
template <bool PACKED>
__global__ __launch_bounds__(kPThreads) void prune_flag_kernel(int64_t nnz, int64_t n_chunks,
                                                               const uint32_t *__restrict__ val,
                                                               const PruneState *__restrict__ st, uint32_t K_arg,
                                                               uint32_t r_arg, const int32_t *__restrict__ base,
                                                               uint8_t *__restrict__ keep) {
    __shared__ uint32_t wtot[2][kPWaves];
    const uint32_t K = st ? st->K : K_arg, r = st ? st->r : r_arg;
    const int wave = threadIdx.x >> 6;
    const uint64_t below_mask = lanes_below();
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        uint32_t running = st ? (uint32_t)base[c] : 0u;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int64_t e = c * kSddmmChunk + it * (4 * kPThreads) + 4 * (int64_t)threadIdx.x;
            uint32_t key[4];
            bool live[4], eq[4];
            load_keys4(val, e, nnz, key, live);
            uint32_t below = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                eq[j] = live[j] && key[j] == K;
                const uint64_t b = __ballot(eq[j]);
                below += __popcll(b & below_mask);
                total += __popcll(b);
            }
            if ((threadIdx.x & 63) == 0) wtot[it][wave] = total;
            __syncthreads();
            uint32_t rank = running + below;
            for (int w = 0; w < wave; ++w) rank += wtot[it][w];
            running += wtot[it][0] + wtot[it][1] + wtot[it][2] + wtot[it][3];
            uint32_t k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                k[j] = live[j] && (key[j] > K || (eq[j] && rank < r));
                rank += eq[j];
            }
            if (e + 4 <= nnz) {
                store_keep4<PACKED>(keep, e, k[0], k[1], k[2], k[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (live[j]) keep[e + j] = (uint8_t)k[j];
            }
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(kPThreads) void prune_threshold_kernel(int64_t nnz, const uint32_t *__restrict__ val,
                                                                    uint32_t tkey, uint8_t *__restrict__ keep,
                                                                    uint32_t *__restrict__ kept_parts) {
    uint32_t mine = 0;
    const int64_t n4 = nnz >> 2;
    const uint4 *val4 = reinterpret_cast<const uint4 *>(val);
    P_LOOP(i, n4) {
        const uint4 v = val4[i];
        const uint32_t a = (v.x & kKeyMask) >= tkey, b = (v.y & kKeyMask) >= tkey, c = (v.z & kKeyMask) >= tkey,
                       d = (v.w & kKeyMask) >= tkey;
        mine += a + b + c + d;
        store_keep4<PACKED>(keep, i << 2, a, b, c, d);
    }
    P_LOOP(j, nnz - (n4 << 2)) {
        const int64_t e = (n4 << 2) + j;
        const uint32_t a = (val[e] & kKeyMask) >= tkey;
        mine += a;
        keep[e] = (uint8_t)a;
    }
    store_kept(mine, kept_parts + blockIdx.x);
}

// ---------------------------------------------------------------------------
// Rows of 1..64 terms: a wavefront per row.  Longer rows go to `list`.
__global__ __launch_bounds__(kPThreads) void prune_row_wave_kernel(int64_t n_rows, const int32_t *__restrict__ rp,
                                                                   const uint32_t *__restrict__ val, int64_t count,
                                                                   uint8_t *__restrict__ keep,
                                                                   int32_t *__restrict__ list, int32_t *n_list,
                                                                   uint32_t *__restrict__ kept_parts) {
    const int lane = threadIdx.x & 63, grp = lane >> 4, sub = lane & 15;
    const int64_t n_waves = (int64_t)gridDim.x * kPWaves;
    uint32_t mine = 0;
    // A wavefront takes kRowBundle consecutive rows at a time, lane group g the row r0 + g.
    for (int64_t r0 = kRowBundle * ((int64_t)blockIdx.x * kPWaves + (threadIdx.x >> 6)); r0 < n_rows;
         r0 += kRowBundle * n_waves) {
        const int64_t rg = r0 + grp;
        const int32_t bg = rg < n_rows ? rp[rg] : 0;
        const int32_t leng = rg < n_rows ? rp[rg + 1] - bg : 0;
        if (__all(leng <= 16)) {   // the four rows side by side: 16 lanes each
            const bool live = sub < leng;
            const uint32_t key = live ? val[(int64_t)bg + sub] & kKeyMask : 0u;
            int32_t rank = 0;
#pragma unroll
            for (int32_t j = 0; j < 16; ++j) {
                const uint32_t kj = __shfl(key, j, 16);
                rank += j < leng && (kj > key || (kj == key && j < sub));
            }
            if (live) {
                const uint32_t k = (int64_t)rank < count;
                keep[(int64_t)bg + sub] = (uint8_t)k;
                mine += k;
            }
            continue;
        }
        for (int g = 0; g < kRowBundle; ++g) {   // one row after the other: 64 lanes each
            const int64_t b = __shfl(bg, 16 * g, 64);
            const int32_t len = __shfl(leng, 16 * g, 64);
            if (len <= 0) continue;
            if (len > 64) {
                if (lane == 0) list[atomicAdd(n_list, 1)] = (int32_t)(r0 + g);
                continue;
            }
            const bool live = lane < len;
            const uint32_t key = live ? val[b + lane] & kKeyMask : 0u;
            int32_t rank = 0;
            if ((int64_t)len > count)   // else every term of the row is kept
                for (int32_t j = 0; j < len; ++j) {
                    const uint32_t kj = __shfl(key, j, 64);
                    rank += kj > key || (kj == key && j < lane);
                }
            if (live) {
                const uint32_t k = (int64_t)rank < count;
                keep[b + lane] = (uint8_t)k;
                mine += k;
            }
        }
    }
    store_kept(mine, kept_parts + blockIdx.x);
}

// Rows of more than 64 terms: a workgroup per listed row.
__global__ __launch_bounds__(kPThreads) void prune_row_group_kernel(const int32_t *__restrict__ list,
                                                                    const int32_t *__restrict__ n_list,
                                                                    const int32_t *__restrict__ rp,
                                                                    const uint32_t *__restrict__ val, int64_t count,
                                                                    uint8_t *__restrict__ keep,
                                                                    uint32_t *__restrict__ kept_parts) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[kPWaves], wtot[2][kPWaves];
    __shared__ uint32_t sK, sRem;
    const int32_t n = *n_list;
    const int wave = threadIdx.x >> 6;
    uint32_t mine = 0;   // thread 0's is what this workgroup's rows keep
    const uint64_t below_mask = lanes_below();
    for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t row = list[i];
        const int64_t b = rp[row];
        const int32_t len = (int32_t)(rp[row + 1] - b);
        if ((int64_t)len <= count || count == 0) {   // the whole row, or nothing of it
            const uint8_t k = count != 0;
            for (int32_t e = threadIdx.x; e < len; e += kPThreads) keep[b + e] = k;
            if (k) mine += (uint32_t)len;
            continue;
        }
        uint32_t K = 0, rem = (uint32_t)count;   // 1 <= count < len
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t himask = pass ? ~((1u << (shift + 8)) - 1u) : 0u;
            hist[threadIdx.x] = 0u;
            __syncthreads();
            for (int32_t e = threadIdx.x; e < len; e += kPThreads) {
                const uint32_t key = val[b + e] & kKeyMask;
                if ((key & himask) == K) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            uint32_t digit, before;
            if (pick_digit(hist, rem, wsum, digit, before)) {
                sK = K | (digit << shift);
                sRem = rem - before;
            }
            __syncthreads();
            K = sK;
            rem = sRem;
        }
        uint32_t running = 0;
        int par = 0;
        for (int32_t e0 = 0; e0 < len; e0 += kPThreads, par ^= 1) {
            const int32_t e = e0 + (int32_t)threadIdx.x;
            const bool live = e < len;
            const uint32_t key = live ? val[b + e] & kKeyMask : 0u;
            const bool eq = live && key == K;
            const uint64_t bal = __ballot(eq);
            if ((threadIdx.x & 63) == 0) wtot[par][wave] = __popcll(bal);
            __syncthreads();
            uint32_t rank = running + __popcll(bal & below_mask);
            for (int w = 0; w < wave; ++w) rank += wtot[par][w];
            running += wtot[par][0] + wtot[par][1] + wtot[par][2] + wtot[par][3];
            if (live) keep[b + e] = (uint8_t)(key > K || (eq && rank < rem));
        }
        mine += (uint32_t)count;
        __syncthreads();   // sK, sRem and the LDS counts are the next row's
    }
    if (threadIdx.x == 0) kept_parts[blockIdx.x] = mine;
}

// ---------------------------------------------------------------------------
struct KeepFlag {   // the mask as 0 / 1 over nnz + 1 positions, the last one 0
    const uint8_t *keep;
    int64_t nnz;
    __host__ __device__ int32_t operator()(int64_t i) const { return i < nnz && keep[i] ? 1 : 0; }
};

__global__ __launch_bounds__(kPThreads) void prune_row_ptr_kernel(int64_t n, const int32_t *__restrict__ rp,
                                                                  const int32_t *__restrict__ pos,
                                                                  int32_t *__restrict__ new_rp) {
    P_LOOP(r, n) new_rp[r] = pos[rp[r]];
}

__global__ __launch_bounds__(kPThreads) void prune_scatter_kernel(int64_t nnz, const uint8_t *__restrict__ keep,
                                                                  const int32_t *__restrict__ pos,
                                                                  const int32_t *__restrict__ col,
                                                                  const uint32_t *__restrict__ val,
                                                                  const uint8_t *__restrict__ ids,
                                                                  int32_t *__restrict__ new_col,
                                                                  uint32_t *__restrict__ new_val,
                                                                  int32_t *__restrict__ src_term,
                                                                  uint8_t *__restrict__ new_ids) {
    P_LOOP(e, nnz) {
        if (!keep[e]) continue;
        const int64_t j = pos[e];
        new_col[j] = col[e];
        new_val[j] = val[e];
        src_term[j] = (int32_t)e;
        if (ids) new_ids[j] = ids[e];
    }
}

hipError_t prune_mask_body(const int32_t *rp, const float *fval, int64_t n_rows, int64_t nnz, sm_prune_mode mode,
                           int64_t count, float threshold, uint8_t *keep, int64_t *kept, hipStream_t s) {
    const uint32_t *val = reinterpret_cast<const uint32_t *>(fval);
    const bool packed = ((uintptr_t)keep & 3) == 0;
    const int64_t n_chunks = (nnz + kSddmmChunk - 1) / kSddmmChunk;
    DevScratch t;
    if (mode == SM_PRUNE_GLOBAL_TOPK) {
        const int64_t k = std::min(count, nnz);
        const PruneState *d_st = nullptr;
        int32_t *d_base = nullptr;
        uint32_t K_arg = 0, r_arg = (uint32_t)nnz;   // k == nnz: every key is >= 0, and all of them rank below nnz
        if (k == 0) K_arg = 0xFFFFFFFFu, r_arg = 0;   // above every key
        if (k > 0 && k < nnz) {
            PruneState *st = nullptr;
            int32_t *d_cnt = nullptr;
            DEV_TRY_RET(t.alloc(&st, 1));
            DEV_TRY_RET(t.alloc(&d_cnt, n_chunks));
            DEV_TRY_RET(t.alloc(&d_base, n_chunks));
            DEV_TRY_RET(hipMemsetAsync(st, 0, sizeof(PruneState), s));
            const unsigned grid = std::min(p_grid((nnz + 3) >> 2), kPHistBlocks);
            for (int pass = 0; pass < 4; ++pass) {
                hipLaunchKernelGGL(prune_hist_kernel, dim3(grid), dim3(kPThreads), 0, s, nnz, val, pass, st);
                hipLaunchKernelGGL(prune_pick_kernel, dim3(1), dim3(kPThreads), 0, s, pass, (uint32_t)k, st);
            }
            hipLaunchKernelGGL(prune_equals_kernel, dim3(p_grid(n_chunks, 1)), dim3(kPThreads), 0, s, nnz, n_chunks, val,
                               st, d_cnt);
            DEV_TRY_RET(hipGetLastError());
            DEV_TRY_RET(dev_excl_sum(t, d_cnt, d_base, n_chunks, s));
            d_st = st;
        }
        const unsigned grid = p_grid(n_chunks, 1);
        if (packed)
            hipLaunchKernelGGL(prune_flag_kernel<true>, dim3(grid), dim3(kPThreads), 0, s, nnz, n_chunks, val, d_st,
                               K_arg, r_arg, d_base, keep);
        else
            hipLaunchKernelGGL(prune_flag_kernel<false>, dim3(grid), dim3(kPThreads), 0, s, nnz, n_chunks, val, d_st,
                               K_arg, r_arg, d_base, keep);
        DEV_TRY_RET(hipGetLastError());
        DEV_TRY_RET(hipStreamSynchronize(s));
        if (kept) *kept = k;
        return hipSuccess;
    }
    // The other two modes count what they keep: one slot per workgroup, added here.
    uint32_t *d_parts = nullptr;
    unsigned n_parts = 0;
    if (mode == SM_PRUNE_THRESHOLD) {
        const unsigned grid = n_parts = p_grid((nnz + 3) >> 2);
        const uint32_t tkey = float_key(threshold);
        DEV_TRY_RET(t.alloc(&d_parts, n_parts));
        if (packed)
            hipLaunchKernelGGL(prune_threshold_kernel<true>, dim3(grid), dim3(kPThreads), 0, s, nnz, val, tkey, keep,
                               d_parts);
        else
            hipLaunchKernelGGL(prune_threshold_kernel<false>, dim3(grid), dim3(kPThreads), 0, s, nnz, val, tkey, keep,
                               d_parts);
    } else {
        int32_t *d_list = nullptr, *d_n = nullptr;
        const unsigned wave_grid = p_grid(n_rows, kRowBundle * kPWaves), group_grid = p_grid(n_rows, 1);
        n_parts = wave_grid + group_grid;
        DEV_TRY_RET(t.alloc(&d_parts, n_parts));
        DEV_TRY_RET(t.alloc(&d_list, n_rows));
        DEV_TRY_RET(t.alloc(&d_n, 1));
        DEV_TRY_RET(hipMemsetAsync(d_n, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(prune_row_wave_kernel, dim3(wave_grid), dim3(kPThreads), 0, s, n_rows, rp, val, count, keep,
                           d_list, d_n, d_parts);
        hipLaunchKernelGGL(prune_row_group_kernel, dim3(group_grid), dim3(kPThreads), 0, s, d_list, d_n, rp, val, count,
                           keep, d_parts + wave_grid);
    }
    DEV_TRY_RET(hipGetLastError());
    std::vector<uint32_t> h_parts(n_parts);
    DEV_TRY_RET(hipMemcpyAsync(h_parts.data(), d_parts, (size_t)n_parts * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DEV_TRY_RET(hipStreamSynchronize(s));
    if (kept) {
        int64_t sum = 0;
        for (const uint32_t v : h_parts) sum += v;
        *kept = sum;
    }
    return hipSuccess;
}

}  // namespace

hipError_t prune_mask_device(const int32_t *rp, const float *val, int64_t n_rows, int64_t nnz, sm_prune_mode mode,
                             int64_t count, float threshold, uint8_t *keep, int64_t *kept, hipStream_t s) {
    if (kept) *kept = 0;
    if (nnz <= 0) return hipSuccess;
    const hipError_t e = prune_mask_body(rp, val, n_rows, nnz, mode, count, threshold, keep, kept, s);
    if (e != hipSuccess) (void)hipGetLastError();   // clear HIP's sticky error: the caller reports `e`
    return e;
}

hipError_t prune_positions_device(int64_t nnz, const uint8_t *keep, int32_t *pos, int64_t *new_nnz, hipStream_t s) {
    hipError_t e = hipSuccess;
    int32_t last = 0;
    {
        DevScratch t;
        hipcub::CountingInputIterator<int64_t> idx(0);
        hipcub::TransformInputIterator<int32_t, KeepFlag, hipcub::CountingInputIterator<int64_t>> in(idx, KeepFlag{keep, nnz});
        e = dev_excl_sum(t, in, pos, nnz + 1, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&last, pos + nnz, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    *new_nnz = last;
    return e;
}

hipError_t launch_prune_compact(int64_t n_rows, int64_t nnz, const uint8_t *keep, const int32_t *pos,
                                const int32_t *rp, const int32_t *col, const float *val, const uint8_t *ids,
                                int32_t *new_rp, int32_t *new_col, float *new_val, int32_t *src_term, uint8_t *new_ids,
                                bool any_kept, hipStream_t s) {
    hipLaunchKernelGGL(prune_row_ptr_kernel, dim3(p_grid(n_rows + 1)), dim3(kPThreads), 0, s, n_rows + 1, rp, pos, new_rp);
    if (nnz > 0 && any_kept)
        hipLaunchKernelGGL(prune_scatter_kernel, dim3(p_grid(nnz)), dim3(kPThreads), 0, s, nnz, keep, pos, col,
                           reinterpret_cast<const uint32_t *>(val), ids, new_col,
                           reinterpret_cast<uint32_t *>(new_val), src_term, new_ids);
    return hipGetLastError();
}

}  // namespace smamd
