// transpose_dev.hip -- the CSR of B^T from a device CSR of B (sm_create_transpose), without
// copying the terms to the host and back.
//
// The result is unique: row c of B^T holds the terms of column c of B by ascending source row,
// equal source rows in stored order -- a stable sort of the terms by column.  Values travel bit
// for bit (explicit zeros, NaN payloads, -0.0).
//
//   histogram  one integer atomicAdd per term into cnt[col]; an exclusive scan of the n_cols + 1
//              counts is B^T's row_ptr (integer sums: the same bytes every time);
//   pack       per term, in term order: its source row by a binary search of row_ptr (coalesced
//              over the terms, neighbours share their search path) packed with the value's bits in
//              one 8-byte word, and its column as the sort key;
//   sort       a stable hipcub::DeviceRadixSort::SortPairs of (column, word) over the key bits
//              n_cols - 1 needs (none for n_cols == 1: the packed order is the answer already);
//   unpack     t_col[j] = the word's row, t_val[j] = its value bits, coalesced.
//
// The sort carries (row, value) itself and not the term's index: the gathers row[idx[j]] and
// val[idx[j]] it would leave are random 4-byte reads over the whole matrix, dearer than 4 more
// bytes per term in every radix pass.
//
// Scratch: 24 bytes per term (keys 2 x 4, words 2 x 8: the sort's double buffers) + hipCUB's
// own temporary storage (digit histograms, a few KiB to MiB, independent of the term count at
// these sizes) + 4 (n_cols + 1) bytes of counts.  All of it is freed on every path.
// Deterministic: the counts are integer sums, the sort is stable, nothing else is reduced.
//
// transpose_ids_device: a CopyForm-built matrix's codebook ids (one byte per term) in the new
// order -- the same pack / sort / unpack with the widened id as the "value" (8 more bytes per
// term of scratch; such matrices are bounded by their dense index).  transpose_terms_device: the
// terms' own indices the same way (sm_build_opts.updatable: values given in the source's order).
#include <algorithm>
#include <vector>

#include "devprim.h"
#include "sm_internal.h"

namespace smamd {
namespace {

__global__ __launch_bounds__(256) void tr_count_kernel(int64_t nnz, const int32_t *__restrict__ col,
                                                       int32_t *__restrict__ cnt) {
    GS_LOOP(e, nnz) atomicAdd(&cnt[col[e]], 1);
}

// key = the term's column; word = source row << 32 | value bits.  The row of term e is the last
// r with row_ptr[r] <= e (row_ptr[n_rows] = nnz > e; empty rows are skipped by the rule).
__global__ __launch_bounds__(256) void tr_pack_kernel(int64_t nnz, int32_t n_rows, const int32_t *__restrict__ rp,
                                                      const int32_t *__restrict__ col, const float *__restrict__ val,
                                                      uint32_t *__restrict__ key,
                                                      unsigned long long *__restrict__ word) {
    GS_LOOP(e, nnz) {
        int32_t lo = 0, hi = n_rows;   // rp[lo] <= e < rp[hi]
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)rp[mid] <= e) lo = mid;
            else hi = mid;
        }
        key[e] = (uint32_t)col[e];
        word[e] = ((unsigned long long)(uint32_t)lo << 32) | __float_as_uint(val[e]);
    }
}

__global__ __launch_bounds__(256) void tr_unpack_kernel(int64_t nnz, const unsigned long long *__restrict__ word,
                                                        int32_t *__restrict__ t_col, float *__restrict__ t_val) {
    GS_LOOP(j, nnz) {
        const unsigned long long w = word[j];
        if (t_col) t_col[j] = (int32_t)(uint32_t)(w >> 32);
        t_val[j] = __uint_as_float((uint32_t)w);
    }
}

// Codebook ids ride through the same transposition as the bits of a 4-byte "value".
__global__ __launch_bounds__(256) void tr_widen_kernel(int64_t nnz, const uint8_t *__restrict__ ids,
                                                       uint32_t *__restrict__ wide) {
    GS_LOOP(e, nnz) wide[e] = ids[e];
}

__global__ __launch_bounds__(256) void tr_iota_kernel(int64_t nnz, uint32_t *__restrict__ idx) {
    GS_LOOP(e, nnz) idx[e] = (uint32_t)e;
}

__global__ __launch_bounds__(256) void tr_narrow_kernel(int64_t nnz, const uint32_t *__restrict__ wide,
                                                        uint8_t *__restrict__ ids) {
    GS_LOOP(j, nnz) ids[j] = (uint8_t)wide[j];
}

// Bits that hold v, 0 for v == 0 (one column: no sort); devprim.h's bits_for counts at least 1.
int key_bits(uint32_t v) {
    int b = 0;
    while (b < 32 && (v >> b) != 0) ++b;
    return b;
}

hipError_t transpose_body(const int32_t *rp, const int32_t *col, const float *val, int64_t n_rows, int64_t n_cols,
                          int64_t nnz, int32_t *t_rp, int32_t *t_col, float *t_val, hipStream_t s) {
    DevScratch t;
    if (t_rp) {   // (null with t_col: only the values' new order is wanted)
        int32_t *cnt = nullptr;
        DEV_TRY_RET(t.alloc(&cnt, n_cols + 1));
        DEV_TRY_RET(hipMemsetAsync(cnt, 0, (size_t)(n_cols + 1) * 4, s));
        if (nnz > 0) {
            hipLaunchKernelGGL(tr_count_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, col, cnt);
            DEV_TRY_RET(hipGetLastError());
        }
        DEV_TRY_RET(dev_excl_sum(t, cnt, t_rp, n_cols + 1, s));
    }
    if (nnz > 0) {
        uint32_t *key[2] = {nullptr, nullptr};
        unsigned long long *word[2] = {nullptr, nullptr};
        const int end_bit = key_bits((uint32_t)(n_cols - 1));
        DEV_TRY_RET(t.alloc(&key[0], nnz));
        DEV_TRY_RET(t.alloc(&word[0], nnz));
        hipLaunchKernelGGL(tr_pack_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, (int32_t)n_rows, rp, col, val,
                           key[0], word[0]);
        DEV_TRY_RET(hipGetLastError());
        const unsigned long long *sorted = word[0];   // one column: every key equal, stored order stays
        if (end_bit > 0) {
            DEV_TRY_RET(t.alloc(&key[1], nnz));
            DEV_TRY_RET(t.alloc(&word[1], nnz));
            hipcub::DoubleBuffer<uint32_t> dk(key[0], key[1]);
            hipcub::DoubleBuffer<unsigned long long> dw(word[0], word[1]);
            size_t bytes = 0;
            DEV_TRY_RET(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, dk, dw, (int)nnz, 0, end_bit, s));
            uint8_t *tmp = nullptr;
            DEV_TRY_RET(t.alloc(&tmp, (int64_t)bytes));
            DEV_TRY_RET(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, dk, dw, (int)nnz, 0, end_bit, s));
            sorted = dw.Current();
        }
        hipLaunchKernelGGL(tr_unpack_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, sorted, t_col, t_val);
        DEV_TRY_RET(hipGetLastError());
    }
    return hipStreamSynchronize(s);   // the scratch is freed on return
}

}  // namespace

hipError_t transpose_csr_device(const int32_t *rp, const int32_t *col, const float *val, int64_t n_rows,
                                int64_t n_cols, int64_t nnz, int32_t *t_rp, int32_t *t_col, float *t_val,
                                hipStream_t s) {
    const hipError_t e = transpose_body(rp, col, val, n_rows, n_cols, nnz, t_rp, t_col, t_val, s);
    if (e != hipSuccess) (void)hipGetLastError();   // clear HIP's sticky error: the caller reports `e`
    return e;
}

hipError_t transpose_ids_device(const int32_t *rp, const int32_t *col, const uint8_t *ids, int64_t n_rows,
                                int64_t n_cols, int64_t nnz, uint8_t *t_ids, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    {
        DevScratch t;
        uint32_t *wide = nullptr, *t_wide = nullptr;
        e = t.alloc(&wide, nnz);
        if (e == hipSuccess) e = t.alloc(&t_wide, nnz);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(tr_widen_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, ids, wide);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = transpose_body(rp, col, reinterpret_cast<const float *>(wide), n_rows, n_cols, nnz, nullptr, nullptr,
                               reinterpret_cast<float *>(t_wide), s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(tr_narrow_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, t_wide, t_ids);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

hipError_t transpose_terms_device(const int32_t *rp, const int32_t *col, int64_t n_rows, int64_t n_cols,
                                  int64_t nnz, int32_t *t_src, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    {
        DevScratch t;
        uint32_t *idx = nullptr;
        e = t.alloc(&idx, nnz);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(tr_iota_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, idx);
            e = hipGetLastError();
        }
        if (e == hipSuccess)   // the index rides as the bits of the 4-byte "value", straight into t_src
            e = transpose_body(rp, col, reinterpret_cast<const float *>(idx), n_rows, n_cols, nnz, nullptr, nullptr,
                               reinterpret_cast<float *>(t_src), s);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

}  // namespace smamd
