// kernels_quantize.hip -- 1-D k-means (Lloyd) on a matrix's stored values: sm_quantize_assign,
// sm_quantize_update, sm_create_quantized, and the value expansion of
// sm_create_from_csr_ids_device (DESIGN.md "Quantising the values").
//
//   expand_ids     val[e] = table[ids[e]], a bit copy with the table in LDS; an id >= T raises
//                  the flag (the device table constructor's validation, folded into the pass).
//   minmax         the least and greatest stored value per workgroup (the host joins the few
//                  partials) and a flag for a NaN or Inf: the linear starting table.
//   assign         every workgroup stages the table into LDS sorted -- a rank sort over broadcast
//                  reads: entry t counts the entries before it, NaN entries take no place, equal
//                  entries (as floats: -0.0 == +0.0) sit side by side and all carry the lowest t of
//                  their run -- and every lane runs an 8-step binary search per term for the number
//                  of candidates <= v, on 16-byte loads of val.  The two bracketing candidates are
//                  compared by the header's rule.  Ids go out four to a 32-bit store where `ids`
//                  is 4-byte aligned, bytewise otherwise and for the last nnz % 4 terms.
//   chunk          one workgroup per chunk of kSddmmChunk terms, the shape of sm_sddmm_table's
//                  table_bin: values (widened to double once, while staging, so that no scanning lane
//                  converts), ids and the squared distances to the old entries go to LDS,
//                  thread t < T scans the chunk in ascending term order (every lane reads the same
//                  LDS address) and adds the values whose id is t, in double, one add each, from
//                  +0.0; thread 255 -- never an id -- adds the chunk's squares in the same loop.
//                  (A variant that formed the ids in this kernel instead of reading them, so that
//                  a Lloyd step read val once, was measured and dropped: 1131 us against 78 + 888
//                  for the two kernels on config 2's shape, DESIGN.md.)
//   finish         S[t], n[t] and the sse over the chunks in ascending order (the shape of
//                  table_finish_kernel: all threads stage chunk rows, one thread per id adds), then
//                  table[t] = (float)(S[t] / n[t]) where n[t] > 0.
// No atomics on data (only the error flags), no state that outlives a launch; every launch
// geometry is a function of nnz alone.
#include <algorithm>
#include <cmath>

#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kQThreads = 256;
constexpr int64_t kQMaxBlocks = 2048;   // 256 CUs x 8; the rest by grid stride
constexpr int kQSseSlot = 255;          // the partial slot of the chunk's sse: T <= 255, never an id

unsigned q_grid(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kQThreads - 1) / kQThreads, kQMaxBlocks));
}

#define Q_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---------------------------------------------------------------------------
template <bool PACKED>
__global__ __launch_bounds__(kQThreads) void expand_ids_kernel(int64_t nnz, const uint8_t *__restrict__ ids,
                                                               const uint32_t *__restrict__ table, int32_t T,
                                                               uint32_t *__restrict__ val, int32_t *flag) {
    __shared__ uint32_t stab[256];
    stab[threadIdx.x] = (int32_t)threadIdx.x < T ? table[threadIdx.x] : 0u;
    __syncthreads();
    const uint32_t uT = (uint32_t)T;
    bool bad = false;
    if (PACKED) {   // ids 4-byte aligned (val is the matrix's own allocation)
        const int64_t n4 = nnz >> 2;
        const uint32_t *id4 = reinterpret_cast<const uint32_t *>(ids);
        uint4 *val4 = reinterpret_cast<uint4 *>(val);
        Q_LOOP(i, n4) {
            const uint32_t w = id4[i];
            const uint32_t a = w & 255u, b = (w >> 8) & 255u, c = (w >> 16) & 255u, d = w >> 24;
            bad |= a >= uT || b >= uT || c >= uT || d >= uT;
            val4[i] = make_uint4(stab[a], stab[b], stab[c], stab[d]);
        }
        Q_LOOP(j, nnz - (n4 << 2)) {
            const int64_t e = (n4 << 2) + j;
            const uint32_t a = ids[e];
            bad |= a >= uT;
            val[e] = stab[a];
        }
    } else {
        Q_LOOP(e, nnz) {
            const uint32_t a = ids[e];
            bad |= a >= uT;
            val[e] = stab[a];
        }
    }
    if (bad) atomicOr(flag, 1);
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kQThreads) void quantize_minmax_kernel(int64_t nnz, const float *__restrict__ val,
                                                                    float *__restrict__ parts, int32_t *flag) {
    __shared__ float slo[kQThreads / 64], shi[kQThreads / 64];
    float lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    auto take = [&](float v) {
        bad |= (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;   // NaN or Inf
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    };
    const int64_t n4 = nnz >> 2;
    const float4 *val4 = reinterpret_cast<const float4 *>(val);
    Q_LOOP(i, n4) {
        const float4 v = val4[i];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    Q_LOOP(j, nnz - (n4 << 2)) take(val[(n4 << 2) + j]);
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        slo[threadIdx.x >> 6] = lo;
        shi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kQThreads / 64; ++w) {
            lo = fminf(lo, slo[w]);
            hi = fmaxf(hi, shi[w]);
        }
        parts[2 * blockIdx.x] = lo;
        parts[2 * blockIdx.x + 1] = hi;
    }
    if (bad) atomicOr(flag, 1);
}

// ---------------------------------------------------------------------------
// The candidates of a table, sorted (sm_quantize_assign step 1): sv[0, n) ascending with equal
// values side by side, NaN from n on (n <= 255, so sv[255] always is); sid[p] the lowest t among
// the entries equal to sv[p].
struct QTable {
    float raw[256];
    float sv[256];
    uint8_t sid[256];
};

// All 256 threads of the workgroup; ends with a barrier.
__device__ __forceinline__ void stage_candidates(QTable &q, const float *__restrict__ table, int32_t T) {
    const int32_t t = threadIdx.x;
    q.raw[t] = t < T ? table[t] : NAN;
    q.sv[t] = NAN;
    q.sid[t] = 0;
    __syncthreads();
    const float v = q.raw[t];
    if (v == v) {
        int32_t pos = 0, rep = t;
        for (int32_t u = 0; u < T; ++u) {
            const float w = q.raw[u];   // every lane the same address
            if (w < v || (w == v && u < t)) ++pos;
            if (w == v && u < rep) rep = u;
        }
        q.sv[pos] = v;
        q.sid[pos] = (uint8_t)rep;
    }
    __syncthreads();
}

// sm_quantize_assign steps 2-5 for one value.
__device__ __forceinline__ uint32_t nearest_id(const QTable &q, float v) {
    int32_t c = 0;   // the number of candidates <= v (a NaN slot or a NaN v compares false)
#pragma unroll
    for (int32_t step = 128; step > 0; step >>= 1)
        if (q.sv[c + step - 1] <= v) c += step;
    const float hi = q.sv[c];   // c <= 255; NaN: there is none
    const bool has_hi = hi == hi;
    const int32_t cl = c > 0 ? c - 1 : 0;
    const float lo = q.sv[cl];
    const uint32_t tl = q.sid[cl], th = q.sid[c];
    if (!(v == v)) return 0u;
    if (c == 0) return has_hi ? th : 0u;
    if (!has_hi) return tl;
    const float dl = __fsub_rn(v, lo), dh = __fsub_rn(hi, v);
    return (dh < dl || (dh == dl && th < tl)) ? th : tl;
}

__device__ __forceinline__ uint32_t nearest_id4(const QTable &q, float4 v) {
    return nearest_id(q, v.x) | (nearest_id(q, v.y) << 8) | (nearest_id(q, v.z) << 16) | (nearest_id(q, v.w) << 24);
}

template <bool PACKED>
__global__ __launch_bounds__(kQThreads) void quantize_assign_kernel(int64_t nnz, const float *__restrict__ val,
                                                                    const float *__restrict__ table, int32_t T,
                                                                    uint8_t *__restrict__ ids) {
    __shared__ QTable q;
    stage_candidates(q, table, T);
    const int64_t n4 = nnz >> 2;
    const float4 *val4 = reinterpret_cast<const float4 *>(val);
    Q_LOOP(i, n4) {
        const uint32_t w = nearest_id4(q, val4[i]);
        if (PACKED) {
            reinterpret_cast<uint32_t *>(ids)[i] = w;
        } else {
            uint8_t *p = ids + (i << 2);
            p[0] = (uint8_t)w;
            p[1] = (uint8_t)(w >> 8);
            p[2] = (uint8_t)(w >> 16);
            p[3] = (uint8_t)(w >> 24);
        }
    }
    Q_LOOP(j, nnz - (n4 << 2)) {
        const int64_t e = (n4 << 2) + j;
        ids[e] = (uint8_t)nearest_id(q, val[e]);
    }
}

// ---------------------------------------------------------------------------
// One chunk (sm_quantize_update steps 1 and 5).  `ids` is the caller's: any alignment, read bytewise.
struct alignas(16) QChunk {
    double sq[kSddmmChunk];              // (val - old[id])^2, +0.0 past the chunk's end
    double val[kSddmmChunk];             // widened once here, not by every scanning lane
    uint32_t id4[kSddmmChunk / 4];       // four ids to a word, 255 (no id) past the chunk's end
    float old[256];                      // the table on entry, 0 past T
};

__global__ __launch_bounds__(kQThreads) void quantize_chunk_kernel(int64_t nnz, const float *__restrict__ val,
                                                                   const float *__restrict__ table, int32_t T,
                                                                   const uint8_t *__restrict__ ids,
                                                                   double *__restrict__ psum,
                                                                   int32_t *__restrict__ pcnt, int32_t *flag) {
    __shared__ QChunk ch;
    const int32_t tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kSddmmChunk;   // a multiple of 4: val + c0 is 16-byte aligned
    const int32_t n = (int32_t)min((int64_t)kSddmmChunk, nnz - c0);
    ch.old[tid] = tid < T ? table[tid] : 0.0f;
    __syncthreads();
    uint8_t *sid = reinterpret_cast<uint8_t *>(ch.id4);
    bool bad = false;
    for (int32_t g = tid; g < kSddmmChunk / 4; g += kQThreads) {
        const int32_t i0 = 4 * g;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t id[4] = {255u, 255u, 255u, 255u};
        if (i0 + 4 <= n) {
            const float4 f = *reinterpret_cast<const float4 *>(val + c0 + i0);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) continue;
            if (i0 + 4 > n) v[k] = val[c0 + i0 + k];
            id[k] = ids[c0 + i0 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool live = i0 + k < n;
            if (live && id[k] >= (uint32_t)T) bad = true;
            const double d = __dsub_rn((double)v[k], (double)ch.old[id[k]]);
            ch.sq[i0 + k] = live ? __dmul_rn(d, d) : 0.0;
            ch.val[i0 + k] = (double)v[k];
            sid[i0 + k] = (uint8_t)id[k];
        }
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    const uint32_t t = (uint32_t)tid;
    const bool bins = (int32_t)t < T, sums = t == (uint32_t)kQSseSlot;
    if (!bins && !sums) return;
    double acc = 0.0;
    int32_t cnt = 0;
    const double2 *v2 = reinterpret_cast<const double2 *>(ch.val);
    const double2 *s2 = reinterpret_cast<const double2 *>(ch.sq);
    const int32_t n4 = (n + 3) >> 2;
    for (int32_t i = 0; i < n4; ++i) {
        if (bins) {
            const uint32_t w = ch.id4[i];
            const double2 a = v2[2 * i], b = v2[2 * i + 1];
            if ((w & 255u) == t) acc = __dadd_rn(acc, a.x), ++cnt;
            if (((w >> 8) & 255u) == t) acc = __dadd_rn(acc, a.y), ++cnt;
            if (((w >> 16) & 255u) == t) acc = __dadd_rn(acc, b.x), ++cnt;
            if ((w >> 24) == t) acc = __dadd_rn(acc, b.y), ++cnt;
        } else {   // the squares past the chunk's end are +0.0: adding them changes nothing
            const double2 a = s2[2 * i], b = s2[2 * i + 1];
            acc = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(acc, a.x), a.y), b.x), b.y);
        }
    }
    psum[(int64_t)blockIdx.x * kTablePartialStride + t] = acc;
    if (bins) pcnt[(int64_t)blockIdx.x * kTablePartialStride + t] = cnt;
}

// ---------------------------------------------------------------------------
// sm_quantize_update steps 2-5.  A workgroup owns kQFinIds ids (the last one also slot 255, the
// sse): all threads stage kQFinRows chunk rows of them into LDS, the next step's loads already in
// flight, and one thread per id adds the staged column in row order.  The counts are integers:
// every thread sums those it loaded, and the sums are joined at the end.
constexpr int kQFinIds = 16;
constexpr int kQFinRows = 256;
constexpr int kQFinLoads = kQFinRows * (kQFinIds / 2) / kQThreads;   // double2 loads per thread and step
static_assert(kQFinLoads * kQThreads == kQFinRows * (kQFinIds / 2) && kTablePartialStride % kQFinIds == 0, "whole loads");
__global__ __launch_bounds__(kQThreads) void quantize_finish_kernel(int64_t n_chunks, int32_t T,
                                                                    const double *__restrict__ psum,
                                                                    const int32_t *__restrict__ pcnt, float *table,
                                                                    int32_t *counts, double *sse) {
    __shared__ alignas(16) double tile[kQFinRows][kQFinIds];
    __shared__ int32_t cred[kQThreads / 8][kQFinIds];
    const int32_t id0 = blockIdx.x * kQFinIds;
    const bool has_sse = id0 <= kQSseSlot && kQSseSlot < id0 + kQFinIds;
    if (id0 >= T && !has_sse) return;   // the whole workgroup
    const int32_t row = threadIdx.x >> 3, q = threadIdx.x & 7;
    const double2 *ps = reinterpret_cast<const double2 *>(psum + id0 + 2 * q);
    const int2 *pc = reinterpret_cast<const int2 *>(pcnt + id0 + 2 * q);
    // Slots in [T, 255) were never written by the chunks: they are read, never stored.
    double2 next[kQFinLoads];
    int2 csum = make_int2(0, 0);
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < kQFinLoads; ++i) {
            const int64_t k = k0 + row + (kQThreads / 8) * i;
            next[i] = make_double2(0.0, 0.0);
            if (k < n_chunks) {
                next[i] = ps[k * (kTablePartialStride / 2)];
                const int2 c = pc[k * (kTablePartialStride / 2)];
                csum.x += c.x;
                csum.y += c.y;
            }
        }
    };
    double S = 0.0;
    fetch(0);
    for (int64_t k0 = 0; k0 < n_chunks; k0 += kQFinRows) {
#pragma unroll
        for (int i = 0; i < kQFinLoads; ++i)
            *reinterpret_cast<double2 *>(&tile[row + (kQThreads / 8) * i][2 * q]) = next[i];
        __syncthreads();
        fetch(k0 + kQFinRows);
        const int32_t rows = (int32_t)min((int64_t)kQFinRows, n_chunks - k0);
        if (threadIdx.x < kQFinIds) {
#pragma unroll 8
            for (int32_t r = 0; r < rows; ++r) S = __dadd_rn(S, tile[r][threadIdx.x]);
        }
        __syncthreads();
    }
    cred[row][2 * q] = csum.x;
    cred[row][2 * q + 1] = csum.y;
    __syncthreads();
    if (threadIdx.x >= kQFinIds) return;
    const int32_t t = id0 + (int32_t)threadIdx.x;
    if (t < T) {
        int32_t n = 0;
        for (int j = 0; j < kQThreads / 8; ++j) n += cred[j][threadIdx.x];
        if (n > 0) table[t] = (float)(S / (double)n);   // an empty cluster keeps its entry
        if (counts) counts[t] = n;
    } else if (t == kQSseSlot && sse) {
        *sse = S;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
hipError_t launch_expand_ids(int64_t nnz, const uint8_t *ids, const float *table, int32_t T, float *val,
                             int32_t *flag, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    const uint32_t *tb = reinterpret_cast<const uint32_t *>(table);
    uint32_t *vb = reinterpret_cast<uint32_t *>(val);
    if (((uintptr_t)ids & 3) == 0)
        hipLaunchKernelGGL(expand_ids_kernel<true>, dim3(q_grid((nnz + 3) >> 2)), dim3(kQThreads), 0, s, nnz, ids, tb, T,
                           vb, flag);
    else
        hipLaunchKernelGGL(expand_ids_kernel<false>, dim3(q_grid(nnz)), dim3(kQThreads), 0, s, nnz, ids, tb, T, vb, flag);
    return hipGetLastError();
}

int64_t quantize_minmax_blocks(int64_t nnz) { return nnz > 0 ? (int64_t)q_grid((nnz + 3) >> 2) : 0; }

hipError_t launch_quantize_minmax(int64_t nnz, const float *val, float *parts, int32_t *flag, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(quantize_minmax_kernel, dim3((unsigned)quantize_minmax_blocks(nnz)), dim3(kQThreads), 0, s, nnz,
                       val, parts, flag);
    return hipGetLastError();
}

hipError_t launch_quantize_assign(int64_t nnz, const float *val, const float *table, int32_t T, uint8_t *ids,
                                  hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    const unsigned grid = q_grid((nnz + 3) >> 2);
    if (((uintptr_t)ids & 3) == 0)
        hipLaunchKernelGGL(quantize_assign_kernel<true>, dim3(grid), dim3(kQThreads), 0, s, nnz, val, table, T, ids);
    else
        hipLaunchKernelGGL(quantize_assign_kernel<false>, dim3(grid), dim3(kQThreads), 0, s, nnz, val, table, T, ids);
    return hipGetLastError();
}

hipError_t launch_quantize_chunks(int64_t nnz, const float *val, const float *table, int32_t T, const uint8_t *ids,
                                  double *psum, int32_t *pcnt, int32_t *flag, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((nnz + kSddmmChunk - 1) / kSddmmChunk);
    hipLaunchKernelGGL(quantize_chunk_kernel, dim3(grid), dim3(kQThreads), 0, s, nnz, val, table, T, ids, psum, pcnt,
                       flag);
    return hipGetLastError();
}

hipError_t launch_quantize_finish(int64_t n_chunks, int32_t T, const double *psum, const int32_t *pcnt, float *table,
                                  int32_t *counts, double *sse, hipStream_t s) {
    hipLaunchKernelGGL(quantize_finish_kernel, dim3(kTablePartialStride / kQFinIds), dim3(kQThreads), 0, s, n_chunks, T,
                       psum, pcnt, table, counts, sse);
    return hipGetLastError();
}

}  // namespace smamd
