// kernels_sddmm.hip -- sm_sddmm: one dot product per stored term of B,
//   out[e] = alpha * sum_j G[r_e, j] * X[c_e, j] + beta * out[e]      (CSR order),
// the gradient of Y = alpha * B * X with respect to B's stored values and the dual of the
// row-panel SpMM: the same X rows are gathered, G is read where the SpMM writes Y, and one
// float per term is written (DESIGN.md "SDDMM").
//
//   sddmm_term    one lane per term runs the j loop with separate round-to-nearest
//                 mul / add (the SM_ALGO_PARITY order); any placement, any size.  The
//                 term's row comes from a binary search of row_ptr on the term index:
//                 no thread walks a row, so a 238 K-term row costs what its terms cost.
//   sddmm_panel   G lanes per term, lane g holds G[r, 4g:4g+4] and X[c, 4g:4g+4]
//                 (range-checked 16-byte buffer loads, padded slots sent past the
//                 range), 8 terms' loads in flight; the lanes' partials are joined by a
//                 fixed __shfl_xor tree whose first steps transpose (8 terms in 7 + log2(G/8)
//                 shuffles), leaving one term's sum per lane, so a wavefront stores 64
//                 consecutive floats of `out` at once.
// Workgroups of both kernels take fixed runs of the term range (balanced by terms, not rows).
// Neither kernel uses atomics or state that outlives the launch.
#include "sm_internal.h"

namespace smamd {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSddmmThreads = 256;
constexpr int kSddmmRounds = kSddmmChunk / kSddmmThreads;   // 64-term rounds per wavefront
static_assert(kSddmmChunk % kSddmmThreads == 0, "whole rounds");
constexpr int kTermsPerLane = 4;                 // sddmm_term_kernel
constexpr int kTermBlock = 256 * kTermsPerLane;

// The row holding term e among the `len` rows from `lo` on: the largest r with rp[r] <= e
// (rp[lo] <= e is given, and rp[lo + len] > e); empty rows are skipped because the largest such
// r is taken.  The trip count depends on `len` alone: lanes that share `len` stay converged, and
// several searches can run side by side.
__device__ __forceinline__ int32_t row_of_term(const int32_t *__restrict__ rp, int32_t lo, int32_t len,
                                               int32_t e) {
    for (; len > 1; len -= len >> 1) {
        const int32_t mid = lo + (len >> 1);
        if (rp[mid] <= e) lo = mid;
    }
    return lo;
}

// out = alpha * s + beta * out with the library's beta rule and separate roundings.
__device__ __forceinline__ float finish_term(float s, float o, float alpha, float beta) {
    const float t = mul_rn(alpha, s);
    if (beta != 1.0f) o = mul_rn(beta, o);
    return add_rn(o, t);
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sddmm_term_kernel(int32_t n_rows, int32_t nnz, int32_t n_rhs,
                                                         const int32_t *__restrict__ rp,
                                                         const int32_t *__restrict__ col,
                                                         const float *__restrict__ Gm, int64_t ldg,
                                                         const float *__restrict__ X, int64_t ldx,
                                                         float *__restrict__ out, float alpha, float beta) {
    // The workgroup's kTermBlock consecutive terms lie in the rows [r_lo, r_hi] (two uniform
    // searches of the whole row_ptr); each lane then searches only those, for kTermsPerLane terms
    // a stride of 256 apart (coalesced col / out, independent searches and gathers in flight).
    const int64_t b0 = (int64_t)blockIdx.x * kTermBlock;
    const int32_t b1 = (int32_t)min((int64_t)nnz, b0 + kTermBlock);
    const int32_t r_lo = row_of_term(rp, 0, n_rows, (int32_t)b0);
    const int32_t r_hi = row_of_term(rp, 0, n_rows, b1 - 1);
    int32_t e[kTermsPerLane], r[kTermsPerLane], c[kTermsPerLane];
    bool live[kTermsPerLane];
#pragma unroll
    for (int i = 0; i < kTermsPerLane; ++i) {
        const int64_t e64 = b0 + i * 256 + threadIdx.x;   // 64 bits: nnz may be close to 2^31
        live[i] = e64 < b1;
        e[i] = live[i] ? (int32_t)e64 : b1 - 1;           // a valid term stands in for a missing one
        c[i] = col[e[i]];
        r[i] = r_lo;
    }
    for (int32_t len = r_hi - r_lo + 1; len > 1; len -= len >> 1) {   // row_of_term, side by side
#pragma unroll
        for (int i = 0; i < kTermsPerLane; ++i) {
            const int32_t mid = r[i] + (len >> 1);
            if (rp[mid] <= e[i]) r[i] = mid;
        }
    }
#pragma unroll
    for (int i = 0; i < kTermsPerLane; ++i) {
        if (!live[i]) continue;
        const float *gp = Gm + (int64_t)r[i] * ldg;
        const float *xp = X + (int64_t)c[i] * ldx;
        float s = mul_rn(gp[0], xp[0]);
        for (int32_t j = 1; j < n_rhs; ++j) s = add_rn(s, mul_rn(gp[j], xp[j]));
        out[e[i]] = finish_term(s, out[e[i]], alpha, beta);
    }
}

// ---------------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sddmm_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)bytes, 0x00020000);
}

// G lanes per term (a power of two up to 64); lane g owns the float4 slots g, g + G, ...
// of the j axis (T = ceil(n_rhs / 4G) of them, in that order; T > 1 only at G = 64).
// Summation order of one output: the lane's partial is one fused multiply-add per element, slot
// by slot (4T roundings), the G partials join in a fixed xor tree, lane distances G/2 ... 1
// (log2 G roundings), then alpha * s and the add onto beta * out.
// A group takes its G terms in S = G / U batches of U = min(G, 8): the batch's 2U loads are in
// flight together, its U partials per lane are joined by the transposing steps of the tree
// (distances G/2 ... S: each step halves the terms a lane still carries, the lane whose bit is
// set keeps the upper half), and the plain steps (S/2 ... 1) finish one value per lane.  Lane
// g = k * S + l then holds the sum of term k of every batch and keeps that of batch l: the
// group's G sums sit one per lane, a wavefront stores 64 consecutive floats of `out`.
// The chunk's piece of row_ptr is staged in LDS (a search there waits on the LDS counter only,
// so it overlaps the gathers in flight); a chunk spanning more than kSegRows rows (long runs
// of empty rows) searches row_ptr in memory instead.
// n_rhs % 4 == 0; G and X under 4 GiB (g_bytes, x_bytes).
// At most 4 waves per SIMD are planned for: with the default target of 8 the compiler keeps the
// kernel under 64 registers by waiting after every second term's loads.
template <int G>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void sddmm_panel_kernel(
    int32_t n_rows, int32_t nnz, int32_t n_rhs, const int32_t *__restrict__ rp,
    const int32_t *__restrict__ col, const float *__restrict__ Gm, int64_t ldg, uint32_t g_bytes,
    const float *__restrict__ X, int64_t ldx, uint32_t x_bytes, float *__restrict__ out, float alpha,
    float beta) {
    constexpr int U = G < 8 ? G : 8;   // terms whose loads are in flight together
    constexpr int S = G / U;           // batches per group and round
    constexpr int kLogS = __builtin_ctz(S);
    constexpr int kSegRows = kSddmmChunk + 256;
    constexpr uint32_t kOob = 0xFFFFFFF0u;
    __shared__ int32_t srp[kSegRows];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane & (G - 1);
    const int l = g & (S - 1), k = g >> kLogS;
    const int64_t c0 = (int64_t)blockIdx.x * kSddmmChunk;
    if (c0 >= nnz) return;   // whole workgroups
    const int32_t t1 = (int32_t)min((int64_t)nnz, c0 + kSddmmChunk);
    // The chunk's rows (workgroup-uniform).
    const int32_t r_lo = row_of_term(rp, 0, n_rows, (int32_t)c0);
    const int32_t r_hi = row_of_term(rp, 0, n_rows, t1 - 1);
    const int32_t n_seg = r_hi - r_lo + 1;
    const bool staged = n_seg <= kSegRows;
    if (staged)
        for (int32_t i = threadIdx.x; i < n_seg; i += kSddmmThreads) srp[i] = rp[r_lo + i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t g_src = sddmm_rsrc(Gm, g_bytes);
    const __amdgpu_buffer_rsrc_t x_src = sddmm_rsrc(X, x_bytes);
    const int tiles = G == 64 ? (n_rhs + 4 * G - 1) / (4 * G) : 1;

    for (int round = 0; round < kSddmmRounds; ++round) {
        // Term indices in 64 bits: the last round's may pass t1 (<= 2^31 - 1) before they are compared.
        const int64_t base = c0 + (round * (kSddmmThreads / 64) + wave) * 64;
        if (base >= t1) break;   // wavefront-uniform
        const int64_t e = base + lane;
        int32_t myc = 0, myr = 0;
        if (e < t1) {
            myc = col[e];
            myr = staged ? r_lo + row_of_term(srp, 0, n_seg, (int32_t)e)
                         : row_of_term(rp, r_lo, n_seg, (int32_t)e);
        }
        const int64_t gbase = e - g;   // first term of this lane's group
        float res = 0.0f;
#pragma unroll
        for (int b = 0; b < S; ++b) {
            float part[U];
#pragma unroll
            for (int u = 0; u < U; ++u) part[u] = 0.0f;
            for (int t = 0; t < tiles; ++t) {
                const int slot = g + G * t;
                const bool act = 4 * slot < n_rhs;
                u32x4 gv[U], xv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t r = __shfl(myr, b * U + u, G);
                    const int32_t c = __shfl(myc, b * U + u, G);
                    const bool live = act && gbase + b * U + u < t1;
                    const uint32_t go = live ? 4u * (uint32_t)((int64_t)r * ldg + 4 * slot) : kOob;
                    const uint32_t xo = live ? 4u * (uint32_t)((int64_t)c * ldx + 4 * slot) : kOob;
                    gv[u] = __builtin_amdgcn_raw_buffer_load_b128(g_src, go, 0, 0);
                    xv[u] = __builtin_amdgcn_raw_buffer_load_b128(x_src, xo, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float p = part[u];
                    p = __fmaf_rn(__uint_as_float(gv[u].x), __uint_as_float(xv[u].x), p);
                    p = __fmaf_rn(__uint_as_float(gv[u].y), __uint_as_float(xv[u].y), p);
                    p = __fmaf_rn(__uint_as_float(gv[u].z), __uint_as_float(xv[u].z), p);
                    p = __fmaf_rn(__uint_as_float(gv[u].w), __uint_as_float(xv[u].w), p);
                    part[u] = p;
                }
            }
#pragma unroll
            for (int off = G / 2, n = U / 2; n > 0; off >>= 1, n >>= 1) {   // transposing steps
                const bool up = (g & off) != 0;
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    const float send = up ? part[i] : part[i + n];
                    const float keep = up ? part[i + n] : part[i];
                    part[i] = add_rn(keep, __shfl_xor(send, off, G));
                }
            }
            float v = part[0];
#pragma unroll
            for (int off = S / 2; off > 0; off >>= 1) v = add_rn(v, __shfl_xor(v, off, G));
            if (b == l) res = v;
        }
        const int64_t eo = gbase + l * U + k;   // the term whose sum this lane holds
        if (eo < t1) out[eo] = finish_term(res, out[eo], alpha, beta);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
hipError_t launch_sddmm_term(int32_t n_rows, int32_t nnz, int32_t n_rhs, const int32_t *rp, const int32_t *col,
                             const float *G, int64_t ldg, const float *X, int64_t ldx, float *out, float alpha,
                             float beta, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(sddmm_term_kernel, dim3((unsigned)(((int64_t)nnz + kTermBlock - 1) / kTermBlock)), dim3(256), 0, s, n_rows,
                       nnz, n_rhs, rp, col, G, ldg, X, ldx, out, alpha, beta);
    return hipGetLastError();
}

bool sddmm_panel_ok(int64_t n_rows, int64_t n_cols, int32_t n_rhs, const float *G, int64_t ldg, const float *X,
                    int64_t ldx) {
    return n_rhs >= 4 && n_rhs % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)G % 16) == 0 &&
           ((uintptr_t)X % 16) == 0 && (uint64_t)n_rows * (uint64_t)ldg * 4u < 0xFFFFFFF0ull &&
           (uint64_t)n_cols * (uint64_t)ldx * 4u < 0xFFFFFFF0ull;
}

hipError_t launch_sddmm_panel(int32_t n_rows, int32_t n_cols, int32_t nnz, int32_t n_rhs, const int32_t *rp,
                              const int32_t *col, const float *G, int64_t ldg, const float *X, int64_t ldx,
                              float *out, float alpha, float beta, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    if (!sddmm_panel_ok(n_rows, n_cols, n_rhs, G, ldg, X, ldx)) return hipErrorInvalidValue;
    // The descriptors end with the last row's n_rhs-th element: the padding columns of the
    // last row need not exist.
    const uint32_t g_bytes = (uint32_t)((((int64_t)n_rows - 1) * ldg + n_rhs) * 4);
    const uint32_t x_bytes = (uint32_t)((((int64_t)n_cols - 1) * ldx + n_rhs) * 4);
    int lanes = 1;
    while (lanes < 64 && 4 * lanes < n_rhs) lanes <<= 1;
    const unsigned grid = (unsigned)(((int64_t)nnz + kSddmmChunk - 1) / kSddmmChunk);
#define SM_SDDMM(GG)                                                                                        \
    case GG:                                                                                                \
        hipLaunchKernelGGL(sddmm_panel_kernel<GG>, dim3(grid), dim3(kSddmmThreads), 0, s, n_rows, nnz, n_rhs, \
                           rp, col, G, ldg, g_bytes, X, ldx, x_bytes, out, alpha, beta);                    \
        break;
    switch (lanes) {
        SM_SDDMM(1) SM_SDDMM(2) SM_SDDMM(4) SM_SDDMM(8) SM_SDDMM(16) SM_SDDMM(32) SM_SDDMM(64)
        default: return hipErrorInvalidValue;
    }
#undef SM_SDDMM
    return hipGetLastError();
}

}  // namespace smamd
