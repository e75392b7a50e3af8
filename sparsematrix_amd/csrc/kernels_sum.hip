// kernels_sum.hip -- the sum of two held matrices on the union of their patterns: the count and
// fill passes behind sm_create_sum (DESIGN.md "Sum of two matrices").
//
// Both operands' rows strictly ascend (the caller checks rows_ascend), so a column is found in a
// row by binary search and no thread walks a row: the structure is integers only, and the place
// of every term of C follows from two counts.
//
//   match    one thread per term i of A: its row r (the chunk's first and last row by two uniform
//            searches of the whole row pointer, then a search among those, as kernels_sddmm.hip
//            finds a term's row), the lower bound lb of colA[i] in B's row r, and one word
//            m[i] = lb where B stores the column there (its term index in B), ~lb where it does
//            not: the fill pass needs lb either way and reads it back instead of searching again.
//   scan     S = the exclusive scan (hipCUB) of [m[i] >= 0] over nnzA + 1 positions: S[i] is the
//            number of matched terms of A before i.
//   rows     len[r] = lenA[r] + lenB[r] - (S[rpA[r + 1]] - S[rpA[r]]) in unsigned 32 bits (the
//            lengths sum to at most nnzA + nnzB < 2^32); their exclusive scan (hipCUB) over
//            n_rows + 1 positions is C's row pointer, the last entry its nnz.
//   fill A   term i of A goes to rpC[r] + (i - rpA[r]) + (lb - rpB[r]) - (S[i] - S[rpA[r]]): the
//            terms of A before it in the row, plus the terms of B below its column that no earlier
//            term of A has matched.  It writes the column, the value under the header's rule (B's
//            value at m[i] where matched), terms_a = i and terms_b = m[i] or -1.
//   fill B   term j of B finds the lower bound k of colB[j] in A's row r.  A stores the column:
//            done, A's thread wrote it.  Else it goes to
//            rpC[r] + (j - rpB[r]) + k - (S[rpA[r] + k] - S[rpA[r]]) with terms_a = -1,
//            terms_b = j.
//
// A workgroup takes kSddmmChunk consecutive terms at a time, thread t the terms t, t + 256, ...
// of the chunk, one after the other (coalesced loads; the stores land in ascending places).  A form
// that ran a thread's eight searches side by side was slower on config 2's shape (102 to 130
// registers, 3 to 4 wavefronts per SIMD instead of 8; DESIGN.md has both figures) and is not kept.
// No atomics; every launch geometry is a function of (n_rows, nnzA, nnzB); the result is a function
// of the operands alone.  Products and the add are __fmul_rn / __fadd_rn: two separately rounded
// products and one add, never a fused multiply-add.
#include <algorithm>

#include "devprim.h"
#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kSumThreads = 256;
constexpr int kSumSteps = kSddmmChunk / kSumThreads;   // terms per thread and chunk
constexpr int64_t kSumMaxBlocks = 2048;                // 256 CUs x 8; the rest by grid stride

unsigned sum_grid(int64_t items, int64_t per_block) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, kSumMaxBlocks));
}

// kernels_sddmm.hip's row_of_term: the largest r in [lo, lo + len) with rp[r] <= e.
__device__ __forceinline__ int32_t sum_row_of_term(const int32_t *__restrict__ rp, int32_t lo, int32_t len, int32_t e) {
    for (; len > 1; len -= len >> 1) {
        const int32_t mid = lo + (len >> 1);
        if (rp[mid] <= e) lo = mid;
    }
    return lo;
}

// The first index in [lo, hi) whose column is not below c (hi if there is none).
__device__ __forceinline__ int32_t lower_bound_col(const int32_t *__restrict__ col, int32_t lo, int32_t hi, int32_t c) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The rows [r_lo, r_lo + n) that hold the terms [c0, c1) of a chunk (c0 < c1 <= nnz).
__device__ __forceinline__ void chunk_rows(const int32_t *__restrict__ rp, int32_t n_rows, int32_t c0, int32_t c1,
                                           int32_t &r_lo, int32_t &n) {
    r_lo = sum_row_of_term(rp, 0, n_rows, c0);
    n = sum_row_of_term(rp, r_lo, n_rows - r_lo, c1 - 1) - r_lo + 1;
}

__global__ __launch_bounds__(kSumThreads) void sum_match_kernel(int32_t n_rows, int64_t nnz_a, int64_t n_chunks,
                                                                const int32_t *__restrict__ rp_a,
                                                                const int32_t *__restrict__ col_a,
                                                                const int32_t *__restrict__ rp_b,
                                                                const int32_t *__restrict__ col_b,
                                                                int32_t *__restrict__ m) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t c0 = c * kSddmmChunk, c1 = min(nnz_a, c0 + kSddmmChunk);
        int32_t r_lo, n_seg;
        chunk_rows(rp_a, n_rows, (int32_t)c0, (int32_t)c1, r_lo, n_seg);
#pragma unroll 2
        for (int k = 0; k < kSumSteps; ++k) {
            const int64_t i = c0 + k * kSumThreads + threadIdx.x;
            if (i >= c1) break;
            const int32_t r = sum_row_of_term(rp_a, r_lo, n_seg, (int32_t)i);
            const int32_t cc = col_a[i];
            const int32_t b1 = rp_b[r + 1];
            const int32_t lb = lower_bound_col(col_b, rp_b[r], b1, cc);
            m[i] = lb < b1 && col_b[lb] == cc ? lb : ~lb;
        }
    }
}

struct MatchFlag {   // [m[i] >= 0] over nnz + 1 positions, the last one 0
    const int32_t *m;
    int64_t nnz;
    __host__ __device__ int32_t operator()(int64_t i) const { return i < nnz && m[i] >= 0 ? 1 : 0; }
};

__global__ __launch_bounds__(kSumThreads) void sum_rows_kernel(int64_t n_rows, const int32_t *__restrict__ rp_a,
                                                               const int32_t *__restrict__ rp_b,
                                                               const int32_t *__restrict__ S,
                                                               uint32_t *__restrict__ len) {
    for (int64_t r = (int64_t)blockIdx.x * kSumThreads + threadIdx.x; r <= n_rows; r += (int64_t)gridDim.x * kSumThreads) {
        uint32_t l = 0;
        if (r < n_rows) {
            const int32_t a0 = rp_a[r], a1 = rp_a[r + 1];
            l = (uint32_t)(a1 - a0) + (uint32_t)(rp_b[r + 1] - rp_b[r]) - (uint32_t)(S[a1] - S[a0]);
        }
        len[r] = l;
    }
}

// One side's contribution: absent (the value is not read), the value's bits, or fl(coef * value).
__device__ __forceinline__ bool contribution(bool stored, float coef, const uint32_t *__restrict__ val, int64_t e,
                                             uint32_t &bits) {
    if (!stored || coef == 0.0f) return false;
    bits = val[e];
    if (coef != 1.0f) bits = __float_as_uint(__fmul_rn(coef, __uint_as_float(bits)));
    return true;
}

__device__ __forceinline__ uint32_t sum_value(bool has_a, uint32_t pa, bool has_b, uint32_t pb) {
    if (has_a && has_b) return __float_as_uint(__fadd_rn(__uint_as_float(pa), __uint_as_float(pb)));
    return has_a ? pa : has_b ? pb : 0u;
}

__global__ __launch_bounds__(kSumThreads) void sum_fill_a_kernel(
    int32_t n_rows, int64_t nnz_a, int64_t n_chunks, const int32_t *__restrict__ rp_a, const int32_t *__restrict__ col_a,
    const uint32_t *__restrict__ val_a, float alpha, const int32_t *__restrict__ rp_b, const uint32_t *__restrict__ val_b,
    float beta, const int32_t *__restrict__ m, const int32_t *__restrict__ S, const int32_t *__restrict__ rp_c,
    int32_t *__restrict__ col_c, uint32_t *__restrict__ val_c, int32_t *__restrict__ terms_a,
    int32_t *__restrict__ terms_b) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t c0 = c * kSddmmChunk, c1 = min(nnz_a, c0 + kSddmmChunk);
        int32_t r_lo, n_seg;
        chunk_rows(rp_a, n_rows, (int32_t)c0, (int32_t)c1, r_lo, n_seg);
#pragma unroll 2
        for (int k = 0; k < kSumSteps; ++k) {
            const int64_t i = c0 + k * kSumThreads + threadIdx.x;
            if (i >= c1) break;
            const int32_t r = sum_row_of_term(rp_a, r_lo, n_seg, (int32_t)i);
            const int32_t mi = m[i];
            const bool matched = mi >= 0;
            const int32_t lb = matched ? mi : ~mi;
            const int32_t a0 = rp_a[r];
            const int64_t pos = (int64_t)rp_c[r] + ((int32_t)i - a0) + (lb - rp_b[r]) - (S[i] - S[a0]);
            uint32_t pa = 0, pb = 0;
            const bool has_a = contribution(true, alpha, val_a, i, pa);
            const bool has_b = contribution(matched, beta, val_b, mi, pb);
            col_c[pos] = col_a[i];
            val_c[pos] = sum_value(has_a, pa, has_b, pb);
            terms_a[pos] = (int32_t)i;
            terms_b[pos] = matched ? mi : -1;
        }
    }
}

__global__ __launch_bounds__(kSumThreads) void sum_fill_b_kernel(
    int32_t n_rows, int64_t nnz_b, int64_t n_chunks, const int32_t *__restrict__ rp_b, const int32_t *__restrict__ col_b,
    const uint32_t *__restrict__ val_b, float beta, const int32_t *__restrict__ rp_a, const int32_t *__restrict__ col_a,
    const int32_t *__restrict__ S, const int32_t *__restrict__ rp_c, int32_t *__restrict__ col_c,
    uint32_t *__restrict__ val_c, int32_t *__restrict__ terms_a, int32_t *__restrict__ terms_b) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t c0 = c * kSddmmChunk, c1 = min(nnz_b, c0 + kSddmmChunk);
        int32_t r_lo, n_seg;
        chunk_rows(rp_b, n_rows, (int32_t)c0, (int32_t)c1, r_lo, n_seg);
#pragma unroll 2
        for (int k = 0; k < kSumSteps; ++k) {
            const int64_t j = c0 + k * kSumThreads + threadIdx.x;
            if (j >= c1) break;
            const int32_t r = sum_row_of_term(rp_b, r_lo, n_seg, (int32_t)j);
            const int32_t cc = col_b[j];
            const int32_t a0 = rp_a[r], a1 = rp_a[r + 1];
            const int32_t ka = lower_bound_col(col_a, a0, a1, cc);
            if (ka < a1 && col_a[ka] == cc) continue;   // A's thread wrote this position
            const int64_t pos = (int64_t)rp_c[r] + ((int32_t)j - rp_b[r]) + (ka - a0) - (S[ka] - S[a0]);
            uint32_t pb = 0;
            const bool has_b = contribution(true, beta, val_b, j, pb);
            col_c[pos] = cc;
            val_c[pos] = sum_value(false, 0u, has_b, pb);
            terms_a[pos] = -1;
            terms_b[pos] = (int32_t)j;
        }
    }
}

int64_t sum_chunks(int64_t nnz) { return (nnz + kSddmmChunk - 1) / kSddmmChunk; }

hipError_t sum_count_body(int64_t n_rows, int64_t nnz_a, int64_t nnz_b, const int32_t *rp_a, const int32_t *col_a,
                          const int32_t *rp_b, const int32_t *col_b, DevScratch &t, int32_t **m, int32_t **S,
                          int32_t **rp_c, uint64_t *nnz_c, hipStream_t s) {
    uint32_t *d_len = nullptr, *d_rpc = nullptr;
    DEV_TRY_RET(t.alloc(m, nnz_a));
    DEV_TRY_RET(t.alloc(S, nnz_a + 1));
    DEV_TRY_RET(t.alloc(&d_len, n_rows + 1));
    DEV_TRY_RET(t.alloc(&d_rpc, n_rows + 1));
    *rp_c = reinterpret_cast<int32_t *>(d_rpc);
    if (nnz_a > 0 && nnz_b > 0) {
        const int64_t n_chunks = sum_chunks(nnz_a);
        hipLaunchKernelGGL(sum_match_kernel, dim3(sum_grid(n_chunks, 1)), dim3(kSumThreads), 0, s, (int32_t)n_rows, nnz_a,
                           n_chunks, rp_a, col_a, rp_b, col_b, *m);
        DEV_TRY_RET(hipGetLastError());
        hipcub::CountingInputIterator<int64_t> idx(0);
        hipcub::TransformInputIterator<int32_t, MatchFlag, hipcub::CountingInputIterator<int64_t>> in(idx, MatchFlag{*m, nnz_a});
        DEV_TRY_RET(dev_excl_sum(t, in, *S, nnz_a + 1, s));
    } else {   // nothing can match: m[i] = ~rpB[row] = ~0 for every term of A (B is empty where A is not)
        DEV_TRY_RET(hipMemsetAsync(*m, 0xFF, (size_t)std::max<int64_t>(nnz_a, 1) * sizeof(int32_t), s));
        DEV_TRY_RET(hipMemsetAsync(*S, 0, (size_t)(nnz_a + 1) * sizeof(int32_t), s));
    }
    hipLaunchKernelGGL(sum_rows_kernel, dim3(sum_grid(n_rows + 1, kSumThreads)), dim3(kSumThreads), 0, s, n_rows, rp_a, rp_b, *S, d_len);
    DEV_TRY_RET(hipGetLastError());
    DEV_TRY_RET(dev_excl_sum(t, d_len, d_rpc, n_rows + 1, s));
    uint32_t total = 0;
    DEV_TRY_RET(hipMemcpyAsync(&total, d_rpc + n_rows, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DEV_TRY_RET(hipStreamSynchronize(s));
    *nnz_c = total;
    return hipSuccess;
}

}  // namespace

hipError_t sum_count_device(int64_t n_rows, int64_t nnz_a, int64_t nnz_b, const int32_t *rp_a, const int32_t *col_a,
                            const int32_t *rp_b, const int32_t *col_b, DevScratch &t, int32_t **m, int32_t **S,
                            int32_t **rp_c, uint64_t *nnz_c, hipStream_t s) {
    *nnz_c = 0;
    const hipError_t e = sum_count_body(n_rows, nnz_a, nnz_b, rp_a, col_a, rp_b, col_b, t, m, S, rp_c, nnz_c, s);
    if (e != hipSuccess) (void)hipGetLastError();   // clear HIP's sticky error: the caller reports `e`
    return e;
}

hipError_t launch_sum_fill(int64_t n_rows, int64_t nnz_a, int64_t nnz_b, const int32_t *rp_a, const int32_t *col_a,
                           const float *val_a, float alpha, const int32_t *rp_b, const int32_t *col_b,
                           const float *val_b, float beta, const int32_t *m, const int32_t *S, const int32_t *rp_c,
                           int32_t *col_c, float *val_c, int32_t *terms_a, int32_t *terms_b, hipStream_t s) {
    const uint32_t *ua = reinterpret_cast<const uint32_t *>(val_a), *ub = reinterpret_cast<const uint32_t *>(val_b);
    uint32_t *uc = reinterpret_cast<uint32_t *>(val_c);
    if (nnz_a > 0) {
        const int64_t n_chunks = sum_chunks(nnz_a);
        hipLaunchKernelGGL(sum_fill_a_kernel, dim3(sum_grid(n_chunks, 1)), dim3(kSumThreads), 0, s, (int32_t)n_rows, nnz_a,
                           n_chunks, rp_a, col_a, ua, alpha, rp_b, ub, beta, m, S, rp_c, col_c, uc, terms_a, terms_b);
    }
    if (nnz_b > 0) {
        const int64_t n_chunks = sum_chunks(nnz_b);
        hipLaunchKernelGGL(sum_fill_b_kernel, dim3(sum_grid(n_chunks, 1)), dim3(kSumThreads), 0, s, (int32_t)n_rows, nnz_b,
                           n_chunks, rp_b, col_b, ub, beta, rp_a, col_a, S, rp_c, col_c, uc, terms_a, terms_b);
    }
    return hipGetLastError();
}

}  // namespace smamd
