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
//
// sm_sddmm_table runs the same two kernels with TABLE set: a workgroup takes one chunk of
// kSddmmChunk terms, keeps each term's dot (s before alpha) in LDS instead of storing it, and
// table_bin then sums them per codebook id -- thread t scans the chunk's ids and dots in ascending
// term order (every lane reads the same LDS address: a broadcast, no bank conflicts) and adds the
// dots whose id is t one at a time, from -0.0 -- into the chunk's row of partials.
// table_finish_kernel adds the rows in chunk order.  (DESIGN.md "Table gradient".)
#include "sm_internal.h"

namespace smamd {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSddmmThreads = 256;
constexpr int kSddmmRounds = kSddmmChunk / kSddmmThreads;   // 64-term rounds per wavefront
static_assert(kSddmmChunk % kSddmmThreads == 0, "whole rounds");
constexpr int kTermsPerLane = 4;                 // sddmm_term_kernel (sm_sddmm)
constexpr int kTermBlock = 256 * kTermsPerLane;
constexpr int kTableTermsPerLane = kSddmmChunk / 256;   // sddmm_term_kernel with TABLE: one chunk

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

// The per-id sums of one chunk (sm_sddmm_table step 2): sdot holds the dots of the chunk's n terms
// (written by this workgroup before the call), ids their codebook ids.  Thread t < table_size adds
// the dots with id t in ascending term order, each with its own rounding, from -0.0, and stores
// prow[t].  Ids are staged four to a word; the slots past n hold 255, which is no id (T <= 255).
struct TableLds {
    float dot[kSddmmChunk];
    uint32_t id4[kSddmmChunk / 4];
};
// The chunk's LDS: referenced (and so allocated) only by the TABLE instantiations.
__device__ __forceinline__ TableLds &table_lds() {
    __shared__ TableLds lds;
    return lds;
}
__device__ __forceinline__ void table_stage_ids(TableLds &lds, const uint8_t *__restrict__ ids, int64_t c0, int32_t n) {
    uint8_t *sid = reinterpret_cast<uint8_t *>(lds.id4);
    for (int32_t i = threadIdx.x; i < kSddmmChunk; i += 256) sid[i] = i < n ? ids[c0 + i] : (uint8_t)255;
}
__device__ __forceinline__ void table_bin(const TableLds &lds, int32_t n, int32_t table_size,
                                          float *__restrict__ prow) {
    __syncthreads();   // the dots and ids of the whole chunk are in LDS
    const uint32_t t = threadIdx.x;
    if ((int32_t)t >= table_size) return;
    float acc = -0.0f;
    const float4 *d4 = reinterpret_cast<const float4 *>(lds.dot);
    const int32_t n4 = (n + 3) >> 2;
    for (int32_t i = 0; i < n4; ++i) {
        const uint32_t w = lds.id4[i];
        const float4 d = d4[i];
        if ((w & 255u) == t) acc = add_rn(acc, d.x);
        if (((w >> 8) & 255u) == t) acc = add_rn(acc, d.y);
        if (((w >> 16) & 255u) == t) acc = add_rn(acc, d.z);
        if ((w >> 24) == t) acc = add_rn(acc, d.w);
    }
    prow[t] = acc;
}

// ---------------------------------------------------------------------------
// TABLE (sm_sddmm_table): the block is one chunk, `out` the chunk rows of the partials, and
// alpha / beta are not used (the finish kernel applies them).
template <int kTermsPerLane, bool TABLE>
__global__ __launch_bounds__(256) void sddmm_term_kernel(int32_t n_rows, int32_t nnz, int32_t n_rhs,
                                                         const int32_t *__restrict__ rp,
                                                         const int32_t *__restrict__ col,
                                                         const float *__restrict__ Gm, int64_t ldg,
                                                         const float *__restrict__ X, int64_t ldx,
                                                         float *__restrict__ out, float alpha, float beta,
                                                         const uint8_t *__restrict__ ids, int32_t table_size) {
    constexpr int kTermBlock = 256 * kTermsPerLane;
    // The workgroup's kTermBlock consecutive terms lie in the rows [r_lo, r_hi] (two uniform
    // searches of the whole row_ptr); each lane then searches only those, for kTermsPerLane terms
    // a stride of 256 apart (coalesced col / out, independent searches and gathers in flight).
    const int64_t b0 = (int64_t)blockIdx.x * kTermBlock;
    const int32_t b1 = (int32_t)min((int64_t)nnz, b0 + kTermBlock);
    if constexpr (TABLE) table_stage_ids(table_lds(), ids, b0, (int32_t)(b1 - b0));
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
        if constexpr (TABLE) table_lds().dot[e[i] - (int32_t)b0] = s;
        else out[e[i]] = finish_term(s, out[e[i]], alpha, beta);
    }
    if constexpr (TABLE)
        table_bin(table_lds(), (int32_t)(b1 - b0), table_size, out + (int64_t)blockIdx.x * kTablePartialStride);
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
// TABLE (sm_sddmm_table): `out` is the chunk rows of the partials; alpha / beta are not used.
template <int G, bool TABLE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void sddmm_panel_kernel(
    int32_t n_rows, int32_t nnz, int32_t n_rhs, const int32_t *__restrict__ rp,
    const int32_t *__restrict__ col, const float *__restrict__ Gm, int64_t ldg, uint32_t g_bytes,
    const float *__restrict__ X, int64_t ldx, uint32_t x_bytes, float *__restrict__ out, float alpha,
    float beta, const uint8_t *__restrict__ ids, int32_t table_size) {
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
    if constexpr (TABLE) table_stage_ids(table_lds(), ids, c0, (int32_t)(t1 - c0));
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
        if constexpr (TABLE) {
            if (eo < t1) table_lds().dot[eo - c0] = res;
        } else {
            if (eo < t1) out[eo] = finish_term(res, out[eo], alpha, beta);
        }
    }
    if constexpr (TABLE)
        table_bin(table_lds(), (int32_t)(t1 - c0), table_size, out + (int64_t)blockIdx.x * kTablePartialStride);
}

// sm_sddmm_table steps 3-4: S[t] = the chunks' partials in ascending k, one add each, from -0.0;
// out[t] = finish_term(S[t], out[t]).  The chain over k is serial by contract, so the kernel
// spends its parallelism on the loads: a workgroup owns kFinIds ids, all its threads stage
// kFinRows chunk rows of those ids into LDS (kFinLoads 16-byte loads each, the next step's already
// in flight), and one thread per id adds the staged column in row order.
constexpr int kFinIds = 16;
constexpr int kFinRows = 256;
constexpr int kFinLoads = kFinRows * (kFinIds / 4) / 256;   // float4 loads per thread and step
static_assert(kFinLoads * 256 == kFinRows * (kFinIds / 4) && kTablePartialStride % kFinIds == 0, "whole loads");
__global__ __launch_bounds__(256) void table_finish_kernel(int64_t n_chunks, int32_t table_size,
                                                           const float *__restrict__ partials,
                                                           float *__restrict__ out, float alpha, float beta) {
    __shared__ float tile[kFinRows][kFinIds];
    const int32_t id0 = blockIdx.x * kFinIds;
    const int32_t row = threadIdx.x >> 2, q = threadIdx.x & 3;
    const float4 *src = reinterpret_cast<const float4 *>(partials + id0 + 4 * q);
    // Rows past n_chunks are never added; ids past table_size (never written by the chunks) are
    // read but never stored.
    float4 next[kFinLoads];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < kFinLoads; ++i) {
            const int64_t k = k0 + row + 64 * i;
            next[i] = k < n_chunks ? src[k * (kTablePartialStride / 4)] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    float S = -0.0f;
    fetch(0);
    for (int64_t k0 = 0; k0 < n_chunks; k0 += kFinRows) {
#pragma unroll
        for (int i = 0; i < kFinLoads; ++i) *reinterpret_cast<float4 *>(&tile[row + 64 * i][4 * q]) = next[i];
        __syncthreads();
        fetch(k0 + kFinRows);
        const int32_t rows = (int32_t)min((int64_t)kFinRows, n_chunks - k0);
        if (threadIdx.x < kFinIds) {
#pragma unroll 8
            for (int32_t r = 0; r < rows; ++r) S = add_rn(S, tile[r][threadIdx.x]);
        }
        __syncthreads();
    }
    const int32_t t = id0 + (int32_t)threadIdx.x;
    if (threadIdx.x < kFinIds && t < table_size) out[t] = finish_term(S, out[t], alpha, beta);
}

}  // namespace

// ---------------------------------------------------------------------------
hipError_t launch_sddmm_term(int32_t n_rows, int32_t nnz, int32_t n_rhs, const int32_t *rp, const int32_t *col,
                             const float *G, int64_t ldg, const float *X, int64_t ldx, float *out, float alpha,
                             float beta, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL((sddmm_term_kernel<kTermsPerLane, false>),
                       dim3((unsigned)(((int64_t)nnz + kTermBlock - 1) / kTermBlock)), dim3(256), 0, s, n_rows, nnz,
                       n_rhs, rp, col, G, ldg, X, ldx, out, alpha, beta, (const uint8_t *)nullptr, 0);
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
        hipLaunchKernelGGL((sddmm_panel_kernel<GG, false>), dim3(grid), dim3(kSddmmThreads), 0, s, n_rows, \
                           nnz, n_rhs, rp, col, G, ldg, g_bytes, X, ldx, x_bytes, out, alpha, beta,          \
                           (const uint8_t *)nullptr, 0);                                                    \
        break;
    switch (lanes) {
        SM_SDDMM(1) SM_SDDMM(2) SM_SDDMM(4) SM_SDDMM(8) SM_SDDMM(16) SM_SDDMM(32) SM_SDDMM(64)
        default: return hipErrorInvalidValue;
    }
#undef SM_SDDMM
    return hipGetLastError();
}

hipError_t launch_sddmm_table(bool panel, int32_t n_rows, int32_t n_cols, int32_t nnz, int32_t n_rhs,
                              const int32_t *rp, const int32_t *col, const uint8_t *ids, int32_t table_size,
                              const float *G, int64_t ldg, const float *X, int64_t ldx, float *partials,
                              hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    // Development A/B (-DSM_DEV builds only, tools/table_bench.py --ab-nobin): SM_TABLE_NOBIN=1
    // runs the kernel with no id to scan for -- the dots still go to LDS, no thread sums them.
    if (const char *e = dev_env("SM_TABLE_NOBIN"))
        if (atoi(e)) table_size = 0;
    const unsigned grid = (unsigned)(((int64_t)nnz + kSddmmChunk - 1) / kSddmmChunk);
    if (!panel) {
        hipLaunchKernelGGL((sddmm_term_kernel<kTableTermsPerLane, true>), dim3(grid), dim3(256), 0, s, n_rows, nnz,
                           n_rhs, rp, col, G, ldg, X, ldx, partials, 1.0f, 0.0f, ids, table_size);
        return hipGetLastError();
    }
    if (!sddmm_panel_ok(n_rows, n_cols, n_rhs, G, ldg, X, ldx)) return hipErrorInvalidValue;
    const uint32_t g_bytes = (uint32_t)((((int64_t)n_rows - 1) * ldg + n_rhs) * 4);
    const uint32_t x_bytes = (uint32_t)((((int64_t)n_cols - 1) * ldx + n_rhs) * 4);
    int lanes = 1;
    while (lanes < 64 && 4 * lanes < n_rhs) lanes <<= 1;
#define SM_SDDMM_T(GG)                                                                                      \
    case GG:                                                                                                \
        hipLaunchKernelGGL((sddmm_panel_kernel<GG, true>), dim3(grid), dim3(kSddmmThreads), 0, s, n_rows,   \
                           nnz, n_rhs, rp, col, G, ldg, g_bytes, X, ldx, x_bytes, partials, 1.0f, 0.0f, ids, \
                           table_size);                                                                     \
        break;
    switch (lanes) {
        SM_SDDMM_T(1) SM_SDDMM_T(2) SM_SDDMM_T(4) SM_SDDMM_T(8) SM_SDDMM_T(16) SM_SDDMM_T(32) SM_SDDMM_T(64)
        default: return hipErrorInvalidValue;
    }
#undef SM_SDDMM_T
    return hipGetLastError();
}

hipError_t launch_table_finish(int64_t n_chunks, int32_t table_size, const float *partials, float *out,
                               float alpha, float beta, hipStream_t s) {
    if (table_size <= 0) return hipSuccess;
    hipLaunchKernelGGL(table_finish_kernel, dim3((unsigned)((table_size + kFinIds - 1) / kFinIds)), dim3(256), 0, s,
                       n_chunks, table_size, partials, out, alpha, beta);
    return hipGetLastError();
}

}  // namespace smamd
