// kernels_dense.hip -- the pipeline's entrance and exit: the selection and compaction behind
// sm_create_from_dense_device, and the zero fill and scatter behind sm_to_dense_device (DESIGN.md
// "From and to dense weights").
//
// The dense matrix W (n_rows x n_cols, element (r, c) at w[r * ld + c]) stands for the full CSR in
// which every element is a stored term: term index i = r * n_cols + c.  The rule is
// sm_prune_mask's, on keys (the bits without the sign) and on i; every kernel works on integers.
// E = n_rows * n_cols <= 2^32 - 1, so a 32-bit bin or tie rank counts every element; element
// indices and offsets into w are 64-bit.  The padding columns [n_cols, ld) are never read: a
// kernel addresses w through DenseSrc, which maps i to r * ld + c.
//
//   hist / pick    SM_PRUNE_GLOBAL_TOPK: the four-pass radix select of kernels_prune.hip over the
//                  elements in i-order (pick is that file's kernel), 16-byte loads where every
//                  group of four elements from a multiple of four is contiguous and aligned.
//   equals / flag  the ties per chunk of kSddmmChunk elements, an exclusive scan, then the byte
//                  mask keep[i]: key > K, or key == K and the rank among the equal keys in i-order
//                  below r.  SM_PRUNE_THRESHOLD is the same flag kernel with K = key(threshold) - 1
//                  and r = 0; "keep every element" is K = 0 and r = E.
//   row (wave)     SM_PRUNE_ROW_TOPK, n_cols <= 64: lane c holds element c of its row and counts
//                  the lanes that beat it; four rows to a wavefront where n_cols <= 16.
//   row (group)    n_cols > 64: a workgroup per row, the same radix select on LDS bins, then the tie
//                  ranking by ballots, 256 elements a step.  No thread walks a row alone; the grid
//                  is capped and strides over the rows.
//   count / fill   the kept bytes per chunk, an exclusive scan over n_chunks + 1 (the new nnz at
//                  the end), then one pass in i-order: a kept element's new index is its chunk's
//                  base plus a ballot-prefix rank, and the element that starts row r (c == 0)
//                  writes row_ptr[r], kept or not.  The chunks follow i, not the rows, so
//                  2^20 x 1 and 1 x 2^20 run the same grids.
//   zero / scatter sm_to_dense_device: zeros over the live columns only, then one thread per term
//                  (its row by a binary search of row_ptr) where every row's columns strictly
//                  ascend, so that no two terms share an element.  Other matrices keep the
//                  row-serial scatter_dense_kernel: only its order makes the last stored term win.
//
// Integer atomics on LDS and global counters only; every launch geometry is a function of
// (n_rows, n_cols, the alignment class of w and ld) alone.
#include <algorithm>
#include <cstring>

#include "devprim.h"
#include "prune_select.h"
#include "sm_internal.h"

namespace smamd {
namespace {

// W as the runs of live elements the kernels walk in i-order: `seg` elements every `ld` (one run
// of E where ld == n_cols).
struct DenseSrc {
    const uint32_t *w;
    uint64_t E, seg, ld;
};

// The keys of elements [i, i + 4), i a multiple of 4, and which exist.  VEC: every such group is
// contiguous and 16-byte aligned (the host checks base, seg and ld).
template <bool VEC>
__device__ __forceinline__ void dense_keys4(const DenseSrc &d, uint64_t i, uint32_t key[4], bool live[4]) {
    uint64_t q = d.seg == d.E ? 0 : i / d.seg, c = i - q * d.seg;
    if (VEC && i + 4 <= d.E) {
        const uint4 v = *reinterpret_cast<const uint4 *>(d.w + q * d.ld + c);
        key[0] = v.x & kKeyMask, key[1] = v.y & kKeyMask, key[2] = v.z & kKeyMask, key[3] = v.w & kKeyMask;
        live[0] = live[1] = live[2] = live[3] = true;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        live[j] = i + j < d.E;
        key[j] = live[j] ? d.w[q * d.ld + c] & kKeyMask : 0u;
        if (++c == d.seg) c = 0, ++q;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPThreads) void dense_hist_kernel(DenseSrc d, int pass, PruneState *st) {
    __shared__ uint32_t h[kPCopies * kPCopyStride];
    for (int i = threadIdx.x; i < kPCopies * kPCopyStride; i += kPThreads) h[i] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass ? ~((1u << (shift + 8)) - 1u) : 0u;
    const uint32_t prefix = st->K;   // the undecided bytes are zero
    uint32_t *my = h + (threadIdx.x & (kPCopies - 1)) * kPCopyStride;
    const int64_t n4 = (int64_t)((d.E + 3) >> 2);
    P_LOOP(g, n4) {
        uint32_t key[4];
        bool live[4];
        dense_keys4<VEC>(d, (uint64_t)g << 2, key, live);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (live[j] && (key[j] & himask) == prefix) atomicAdd(&my[(key[j] >> shift) & 255u], 1u);
    }
    __syncthreads();
    uint32_t c = 0;
    for (int k = 0; k < kPCopies; ++k) c += h[k * kPCopyStride + threadIdx.x];
    if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);   // E <= 2^32 - 1: a bin holds every element
}

// The first element of thread `t`'s four in step `it` of chunk `c`.
__device__ __forceinline__ uint64_t chunk_elem(int64_t c, int it) {
    return (uint64_t)c * kSddmmChunk + (uint64_t)(it * (4 * kPThreads) + 4 * (int)threadIdx.x);
}

template <bool VEC>
__global__ __launch_bounds__(kPThreads) void dense_equals_kernel(DenseSrc d, int64_t n_chunks,
                                                                 const PruneState *__restrict__ st,
                                                                 uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kPWaves];
    const uint32_t K = st->K;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        uint32_t mine = 0;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            uint32_t key[4];
            bool live[4];
            dense_keys4<VEC>(d, chunk_elem(c, it), key, live);
#pragma unroll
            for (int j = 0; j < 4; ++j) mine += live[j] && key[j] == K;
        }
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) cnt[c] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// keep[i] for every i of every chunk (the mask holds whole chunks: zero past E).  `st` null: K and
// r are the arguments and `base` is not read.  The ties before a chunk can pass 2^31 but not
// E <= 2^32 - 1: the ranks are unsigned 32-bit.
template <bool VEC>
__global__ __launch_bounds__(kPThreads) void dense_flag_kernel(DenseSrc d, int64_t n_chunks,
                                                               const PruneState *__restrict__ st, uint32_t K_arg,
                                                               uint32_t r_arg, const uint32_t *__restrict__ base,
                                                               uint8_t *__restrict__ keep) {
    __shared__ uint32_t wtot[2][kPWaves];
    const uint32_t K = st ? st->K : K_arg, r = st ? st->r : r_arg;
    const int wave = threadIdx.x >> 6;
    const uint64_t below_mask = lanes_below();
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        uint32_t running = st ? base[c] : 0u;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const uint64_t i = chunk_elem(c, it);
            uint32_t key[4];
            bool live[4], eq[4];
            dense_keys4<VEC>(d, i, key, live);
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
            *reinterpret_cast<uint32_t *>(keep + i) = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
        }
        __syncthreads();   // wtot is the next chunk's
    }
}

// ---------------------------------------------------------------------------
// Rows of at most 64 elements, 1 <= count < n_cols: GROUP lanes per row (16 or 64), lane c its
// element c.
template <int GROUP>
__global__ __launch_bounds__(kPThreads) void dense_row_wave_kernel(const uint32_t *__restrict__ w, int64_t n_rows,
                                                                   int32_t n_cols, int64_t ld, int64_t count,
                                                                   uint8_t *__restrict__ keep) {
    constexpr int kRows = 64 / GROUP;
    const int lane = threadIdx.x & 63, grp = lane / GROUP, sub = lane % GROUP;
    const int64_t n_waves = (int64_t)gridDim.x * kPWaves;
    for (int64_t r0 = kRows * ((int64_t)blockIdx.x * kPWaves + (threadIdx.x >> 6)); r0 < n_rows; r0 += kRows * n_waves) {
        const int64_t r = r0 + grp;
        const bool live = r < n_rows && sub < n_cols;
        const uint32_t key = live ? w[r * ld + sub] & kKeyMask : 0u;
        int32_t rank = 0;
        for (int32_t j = 0; j < n_cols; ++j) {
            const uint32_t kj = __shfl(key, j, GROUP);
            rank += kj > key || (kj == key && j < sub);
        }
        if (live) keep[r * n_cols + sub] = (uint8_t)((int64_t)rank < count);
    }
}

// Longer rows, 1 <= count < n_cols: a workgroup per row.  The bins are kPCopies copies, as in the
// global select: a row of one binade puts every element of the first pass into one bin.
__global__ __launch_bounds__(kPThreads) void dense_row_group_kernel(const uint32_t *__restrict__ w, int64_t n_rows,
                                                                    int64_t n_cols, int64_t ld, uint32_t count,
                                                                    uint8_t *__restrict__ keep) {
    __shared__ uint32_t h[kPCopies * kPCopyStride];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[kPWaves], wtot[2][kPWaves];
    __shared__ uint32_t sK, sRem;
    const int wave = threadIdx.x >> 6;
    const uint64_t below_mask = lanes_below();
    uint32_t *my = h + (threadIdx.x & (kPCopies - 1)) * kPCopyStride;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint32_t *wr = w + row * ld;
        uint8_t *kr = keep + row * n_cols;
        uint32_t K = 0, rem = count;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t himask = pass ? ~((1u << (shift + 8)) - 1u) : 0u;
            for (int i = threadIdx.x; i < kPCopies * kPCopyStride; i += kPThreads) h[i] = 0u;
            __syncthreads();
            for (int64_t e = threadIdx.x; e < n_cols; e += kPThreads) {
                const uint32_t key = wr[e] & kKeyMask;
                if ((key & himask) == K) atomicAdd(&my[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            uint32_t c = 0;
            for (int k = 0; k < kPCopies; ++k) c += h[k * kPCopyStride + threadIdx.x];
            hist[threadIdx.x] = c;
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
        for (int64_t e0 = 0; e0 < n_cols; e0 += kPThreads, par ^= 1) {
            const int64_t e = e0 + threadIdx.x;
            const bool live = e < n_cols;
            const uint32_t key = live ? wr[e] & kKeyMask : 0u;
            const bool eq = live && key == K;
            const uint64_t bal = __ballot(eq);
            if ((threadIdx.x & 63) == 0) wtot[par][wave] = __popcll(bal);
            __syncthreads();
            uint32_t rank = running + __popcll(bal & below_mask);
            for (int w2 = 0; w2 < wave; ++w2) rank += wtot[par][w2];
            running += wtot[par][0] + wtot[par][1] + wtot[par][2] + wtot[par][3];
            if (live) kr[e] = (uint8_t)(key > K || (eq && rank < rem));
        }
        __syncthreads();   // sK, sRem and the LDS counts are the next row's
    }
}

// ---------------------------------------------------------------------------
// The kept bytes of every chunk: thread t the mask's bytes [8t, 8t + 8) of the chunk.
__global__ __launch_bounds__(kPThreads) void dense_count_kernel(const uint8_t *__restrict__ keep, int64_t n_chunks,
                                                                uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kPWaves];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint2 v = *reinterpret_cast<const uint2 *>(keep + c * kSddmmChunk + 8 * threadIdx.x);
        uint32_t mine = __popc(v.x) + __popc(v.y);   // the bytes are 0 or 1
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) cnt[c] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// The compaction, in i-order.  base[c]: the kept elements before chunk c (the checked new nnz
// < 2^31 bounds every position).  Element i = r * n_cols + c goes to col[pos] = c and
// val[pos] = its bits where kept; where c == 0 its position is row_ptr[r]; the last element's
// position, plus itself, is row_ptr[n_rows].
__global__ __launch_bounds__(kPThreads) void dense_fill_kernel(const uint32_t *__restrict__ w, uint64_t E,
                                                               int64_t n_rows, uint64_t n_cols, uint64_t ld,
                                                               int64_t n_chunks, const uint8_t *__restrict__ keep,
                                                               const uint32_t *__restrict__ base,
                                                               int32_t *__restrict__ rp, int32_t *__restrict__ col,
                                                               uint32_t *__restrict__ val) {
    __shared__ uint32_t wtot[2][kPWaves];
    const int wave = threadIdx.x >> 6;
    const uint64_t below_mask = lanes_below();
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        uint32_t running = base[ch];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const uint64_t i = chunk_elem(ch, it);
            const uint32_t bytes = *reinterpret_cast<const uint32_t *>(keep + i);
            uint32_t below = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t b = __ballot((bytes >> (8 * j)) & 1u);
                below += __popcll(b & below_mask);
                total += __popcll(b);
            }
            if ((threadIdx.x & 63) == 0) wtot[it][wave] = total;
            __syncthreads();
            uint32_t pos = running + below;
            for (int w2 = 0; w2 < wave; ++w2) pos += wtot[it][w2];
            running += wtot[it][0] + wtot[it][1] + wtot[it][2] + wtot[it][3];
            if (i < E) {
                uint64_t r = i / n_cols, c = i - r * n_cols;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i + j >= E) break;
                    const uint32_t k = (bytes >> (8 * j)) & 1u;
                    if (c == 0) rp[r] = (int32_t)pos;
                    if (k) {
                        col[pos] = (int32_t)c;
                        val[pos] = w[r * ld + c];
                    }
                    pos += k;
                    if (i + j + 1 == E) rp[n_rows] = (int32_t)pos;
                    if (++c == n_cols) c = 0, ++r;
                }
            }
        }
        __syncthreads();   // wtot is the next chunk's
    }
}

// ---------------------------------------------------------------------------
// Zeros over columns [0, width) of `rows` rows of `out`.  VEC: out and ld allow 16-byte stores at
// every row start; the last width % 4 columns of a row go one by one.
template <bool VEC>
__global__ __launch_bounds__(kPThreads) void dense_zero_kernel(float *__restrict__ out, int64_t rows, int64_t width,
                                                               int64_t ld) {
    if (VEC) {
        const int64_t per_row = (width + 3) >> 2, n4 = width >> 2;
        P_LOOP(t, rows * per_row) {
            const int64_t r = t / per_row, q = t - r * per_row;
            float *p = out + r * ld + 4 * q;
            if (q < n4) *reinterpret_cast<float4 *>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
            else
                for (int64_t c = 4 * q; c < width; ++c) out[r * ld + c] = 0.f;
        }
    } else {
        P_LOOP(t, rows * width) {
            const int64_t r = t / width;
            out[r * ld + (t - r * width)] = 0.f;
        }
    }
}

// One thread per term of a matrix whose rows all strictly ascend: no element is written twice.
__global__ __launch_bounds__(kPThreads) void dense_scatter_terms_kernel(int32_t n_rows, int64_t nnz,
                                                                        const int32_t *__restrict__ rp,
                                                                        const int32_t *__restrict__ col,
                                                                        const float *__restrict__ val,
                                                                        float *__restrict__ out, int64_t ld,
                                                                        bool b_layout) {
    P_LOOP(e, nnz) {
        int32_t lo = 0, hi = n_rows;   // the last row r with rp[r] <= e: rp[0] = 0 <= e < nnz = rp[n_rows]
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (rp[mid] <= (int32_t)e) lo = mid;
            else hi = mid;
        }
        const int64_t r = lo, c = col[e];
        out[b_layout ? r * ld + c : c * ld + r] = val[e];
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

hipError_t dense_mask_body(const float *fw, int64_t n_rows, int64_t n_cols, int64_t ld, sm_prune_mode mode,
                           int64_t count, float threshold, DevScratch &t, uint8_t **keep_out, uint32_t **base_out,
                           int64_t *kept, hipStream_t s) {
    const uint64_t E = (uint64_t)n_rows * (uint64_t)n_cols;
    const int64_t n_chunks = (int64_t)((E + kSddmmChunk - 1) / kSddmmChunk);
    const bool linear = ld == n_cols || n_rows == 1;
    DenseSrc d{reinterpret_cast<const uint32_t *>(fw), E, linear ? E : (uint64_t)n_cols, linear ? E : (uint64_t)ld};
    const bool vec = aligned16(fw) && (linear || (n_cols % 4 == 0 && ld % 4 == 0));
    uint8_t *keep = nullptr;
    uint32_t *cnt = nullptr, *base = nullptr;
    DEV_TRY_RET(t.alloc(&keep, n_chunks * kSddmmChunk));
    DEV_TRY_RET(t.alloc(&cnt, n_chunks + 1));
    DEV_TRY_RET(t.alloc(&base, n_chunks + 1));
    // The producers write the live elements only (the flag kernel: up to the next multiple of 4).
    DEV_TRY_RET(hipMemsetAsync(keep + (n_chunks - 1) * kSddmmChunk, 0, kSddmmChunk, s));
    DEV_TRY_RET(hipMemsetAsync(cnt + n_chunks, 0, sizeof(uint32_t), s));
    const unsigned chunk_grid = p_grid(n_chunks, 1);
    size_t scan_bytes = 0;
    uint8_t *scan_tmp = nullptr;
    DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, cnt, base, (int)(n_chunks + 1), s));
    DEV_TRY_RET(t.alloc(&scan_tmp, (int64_t)scan_bytes));

    bool row_select = mode == SM_PRUNE_ROW_TOPK && count < n_cols;
    if (row_select) {
        const uint32_t *w = d.w;
        if (n_cols <= 16)
            hipLaunchKernelGGL(dense_row_wave_kernel<16>, dim3(p_grid(n_rows, 4 * kPWaves)), dim3(kPThreads), 0, s, w,
                               n_rows, (int32_t)n_cols, ld, count, keep);
        else if (n_cols <= 64)
            hipLaunchKernelGGL(dense_row_wave_kernel<64>, dim3(p_grid(n_rows, kPWaves)), dim3(kPThreads), 0, s, w, n_rows,
                               (int32_t)n_cols, ld, count, keep);
        else
            hipLaunchKernelGGL(dense_row_group_kernel, dim3(p_grid(n_rows, 1)), dim3(kPThreads), 0, s, w, n_rows, n_cols,
                               ld, (uint32_t)count, keep);
    } else {
        // Every element (K = 0, r = E: every key is >= 0 and every rank below E), the threshold's
        // cut, or the global select's.
        const PruneState *d_st = nullptr;
        uint32_t K_arg = 0, r_arg = (uint32_t)E;
        const uint64_t k = mode == SM_PRUNE_GLOBAL_TOPK ? std::min<uint64_t>((uint64_t)count, E) : E;
        if (mode == SM_PRUNE_THRESHOLD && float_key(threshold) > 0) K_arg = float_key(threshold) - 1, r_arg = 0;
        if (mode == SM_PRUNE_GLOBAL_TOPK && k < E) {   // 1 <= k < E: the caller took k == 0
            PruneState *st = nullptr;
            DEV_TRY_RET(t.alloc(&st, 1));
            DEV_TRY_RET(hipMemsetAsync(st, 0, sizeof(PruneState), s));
            const unsigned grid = std::min(p_grid((int64_t)((E + 3) >> 2)), kPHistBlocks);
            for (int pass = 0; pass < 4; ++pass) {
                if (vec) hipLaunchKernelGGL(dense_hist_kernel<true>, dim3(grid), dim3(kPThreads), 0, s, d, pass, st);
                else hipLaunchKernelGGL(dense_hist_kernel<false>, dim3(grid), dim3(kPThreads), 0, s, d, pass, st);
                hipLaunchKernelGGL(prune_pick_kernel, dim3(1), dim3(kPThreads), 0, s, pass, (uint32_t)k, st);
            }
            if (vec) hipLaunchKernelGGL(dense_equals_kernel<true>, dim3(chunk_grid), dim3(kPThreads), 0, s, d, n_chunks, st, cnt);
            else hipLaunchKernelGGL(dense_equals_kernel<false>, dim3(chunk_grid), dim3(kPThreads), 0, s, d, n_chunks, st, cnt);
            DEV_TRY_RET(hipGetLastError());
            DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, base, (int)(n_chunks + 1), s));
            d_st = st;
        }
        if (vec)
            hipLaunchKernelGGL(dense_flag_kernel<true>, dim3(chunk_grid), dim3(kPThreads), 0, s, d, n_chunks, d_st, K_arg,
                               r_arg, base, keep);
        else
            hipLaunchKernelGGL(dense_flag_kernel<false>, dim3(chunk_grid), dim3(kPThreads), 0, s, d, n_chunks, d_st, K_arg,
                               r_arg, base, keep);
    }
    hipLaunchKernelGGL(dense_count_kernel, dim3(chunk_grid), dim3(kPThreads), 0, s, keep, n_chunks, cnt);
    DEV_TRY_RET(hipGetLastError());
    DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, base, (int)(n_chunks + 1), s));
    uint32_t total = 0;
    DEV_TRY_RET(hipMemcpyAsync(&total, base + n_chunks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DEV_TRY_RET(hipStreamSynchronize(s));
    *keep_out = keep;
    *base_out = base;
    *kept = (int64_t)total;
    return hipSuccess;
}

}  // namespace

hipError_t dense_mask_device(const float *w, int64_t n_rows, int64_t n_cols, int64_t ld, sm_prune_mode mode,
                             int64_t count, float threshold, DevScratch &t, uint8_t **keep, uint32_t **base,
                             int64_t *kept, hipStream_t s) {
    const hipError_t e = dense_mask_body(w, n_rows, n_cols, ld, mode, count, threshold, t, keep, base, kept, s);
    if (e != hipSuccess) (void)hipGetLastError();   // clear HIP's sticky error: the caller reports `e`
    return e;
}

hipError_t launch_dense_fill(const float *w, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t *keep,
                             const uint32_t *base, int32_t *rp, int32_t *col, float *val, hipStream_t s) {
    const uint64_t E = (uint64_t)n_rows * (uint64_t)n_cols;
    const int64_t n_chunks = (int64_t)((E + kSddmmChunk - 1) / kSddmmChunk);
    hipLaunchKernelGGL(dense_fill_kernel, dim3(p_grid(n_chunks, 1)), dim3(kPThreads), 0, s,
                       reinterpret_cast<const uint32_t *>(w), E, n_rows, (uint64_t)n_cols, (uint64_t)ld, n_chunks, keep,
                       base, rp, col, reinterpret_cast<uint32_t *>(val));
    return hipGetLastError();
}

hipError_t launch_dense_zero(float *out, int64_t rows, int64_t width, int64_t ld, hipStream_t s) {
    if (ld == width) width *= rows, ld = width, rows = 1;   // one run
    if (aligned16(out) && (rows == 1 || ld % 4 == 0))
        hipLaunchKernelGGL(dense_zero_kernel<true>, dim3(p_grid(rows * ((width + 3) >> 2))), dim3(kPThreads), 0, s, out,
                           rows, width, ld);
    else
        hipLaunchKernelGGL(dense_zero_kernel<false>, dim3(p_grid(rows * width)), dim3(kPThreads), 0, s, out, rows, width,
                           ld);
    return hipGetLastError();
}

hipError_t launch_scatter_terms(int32_t n_rows, int64_t nnz, const int32_t *rp, const int32_t *col, const float *val,
                                float *out, int64_t ld, bool b_layout, hipStream_t s) {
    hipLaunchKernelGGL(dense_scatter_terms_kernel, dim3(p_grid(nnz)), dim3(kPThreads), 0, s, n_rows, nnz, rp, col, val, out,
                       ld, b_layout);
    return hipGetLastError();
}

}  // namespace smamd
