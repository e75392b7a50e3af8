// kernels_values.hip -- in-place updates of a matrix's stored values (sm_set_values,
// sm_axpy_values; DESIGN.md "Updating the values").
//
// Two steps, both pure streaming, the launch geometry a function of the sizes alone:
//
//   CSR step      val[e] = v[i]  or  val[e] = fl(val[e] + fl(a * d[i])),  i = e (own order) or
//                 i = src[e] (the order of the matrix this one was transposed from: a 4-byte
//                 gather).  Two separate roundings, never a fused multiply-add, so a matrix and
//                 its transposed companion hold the same bits per term after the same call.
//                 Only val[0, nnz) is written: the zero tail of kPadElems stays.
//   refresh step  one launch per layout that holds its own copy of the values.  Slot s reads
//                 t = map[s] (the CSR index of the term stored there, -1 for padding and dummy
//                 slots) and, if t >= 0, stores val[t]: the map read and the slot write are
//                 coalesced, the 4-byte gather hits the val array the CSR step just wrote.
//                 Slots with t < 0 are not written, so they keep the builder's padding bytes.
//                 A term -> slot scatter would dirty a whole line per 4-byte store instead.
//
// Plain slots (the exact / blocked / gather bands, the sliced ELLs): one float per slot, four
// slots per lane and step (16-byte map load, 16-byte store when all four are terms).  Entry slots
// (band2, gcb): a lane's 16-byte entry is {word, word, value, value}; one lane takes one entry,
// an 8-byte map load and one 8-byte store to words 2-3 (4 bytes when only one is a term).
// All offsets are 64-bit.  No LDS, no atomics, no scratch.
//
// Table matrices (sm_set_table, sm_axpy_table; DESIGN.md "Table matrices") need no maps: their
// layouts hold ids, so an update is the table step -- one workgroup writes the new entries into
// the authoritative table and every layout's table copy -- and one CSR pass val[e] = tab[ids[e]]
// (1 + 4 bytes per term, the table staged in LDS) for the kernels that read the CSR values.
#include <algorithm>

#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kValThreads = 256;
constexpr int64_t kValMaxBlocks = 2048;   // 256 CUs x 8; the rest by grid stride

unsigned val_grid(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kValThreads - 1) / kValThreads, kValMaxBlocks));
}

#define VAL_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__device__ __forceinline__ float step(float old, float a, float d, bool axpy) {
    return axpy ? __fadd_rn(old, __fmul_rn(a, d)) : d;
}

// Own order, `in` and val 16-byte aligned: four terms per lane and step; the tail one at a time.
template <bool AXPY>
__global__ __launch_bounds__(kValThreads) void values_own4_kernel(int64_t nnz, float a, const float *__restrict__ in,
                                                                  float *__restrict__ val) {
    const int64_t n4 = nnz >> 2;
    const float4 *in4 = reinterpret_cast<const float4 *>(in);
    float4 *val4 = reinterpret_cast<float4 *>(val);
    VAL_LOOP(i, n4) {
        const float4 d = in4[i];
        if (AXPY) {
            float4 o = val4[i];
            o.x = step(o.x, a, d.x, true);
            o.y = step(o.y, a, d.y, true);
            o.z = step(o.z, a, d.z, true);
            o.w = step(o.w, a, d.w, true);
            val4[i] = o;
        } else {
            val4[i] = d;
        }
    }
    VAL_LOOP(j, nnz - (n4 << 2)) {
        const int64_t e = (n4 << 2) + j;
        val[e] = step(val[e], a, in[e], AXPY);
    }
}

// Own order, any 4-byte aligned `in`.
template <bool AXPY>
__global__ __launch_bounds__(kValThreads) void values_own1_kernel(int64_t nnz, float a, const float *__restrict__ in,
                                                                  float *__restrict__ val) {
    VAL_LOOP(e, nnz) val[e] = step(val[e], a, in[e], AXPY);
}

// Source order: term e reads in[src[e]], 0 <= src[e] < nnz (a permutation built at creation).
template <bool AXPY>
__global__ __launch_bounds__(kValThreads) void values_src_kernel(int64_t nnz, float a, const float *__restrict__ in,
                                                                 const int32_t *__restrict__ src,
                                                                 float *__restrict__ val) {
    VAL_LOOP(e, nnz) val[e] = step(val[e], a, in[src[e]], AXPY);
}

// Plain slots: n_slots floats, map and slot 16-byte aligned (device allocations).
__global__ __launch_bounds__(kValThreads) void refresh_plain_kernel(int64_t n_slots, const int32_t *__restrict__ map,
                                                                    const float *__restrict__ val,
                                                                    float *__restrict__ slot) {
    const int64_t n4 = n_slots >> 2;
    const int4 *map4 = reinterpret_cast<const int4 *>(map);
    VAL_LOOP(i, n4) {
        const int4 t = map4[i];
        float *p = slot + (i << 2);
        if ((t.x | t.y | t.z | t.w) >= 0) {   // four terms: one 16-byte store
            *reinterpret_cast<float4 *>(p) = make_float4(val[t.x], val[t.y], val[t.z], val[t.w]);
        } else {
            if (t.x >= 0) p[0] = val[t.x];
            if (t.y >= 0) p[1] = val[t.y];
            if (t.z >= 0) p[2] = val[t.z];
            if (t.w >= 0) p[3] = val[t.w];
        }
    }
    VAL_LOOP(j, n_slots - (n4 << 2)) {
        const int64_t s = (n4 << 2) + j;
        const int32_t t = map[s];
        if (t >= 0) slot[s] = val[t];
    }
}

// Entry slots (band2, gcb): n_ent lane entries of four words, the values in words 2 and 3.
__global__ __launch_bounds__(kValThreads) void refresh_entry_kernel(int64_t n_ent, const int2 *__restrict__ map,
                                                                    const float *__restrict__ val,
                                                                    uint32_t *__restrict__ ent) {
    VAL_LOOP(i, n_ent) {
        const int2 t = map[i];
        float *p = reinterpret_cast<float *>(ent + (i << 2) + 2);
        if ((t.x | t.y) >= 0) {
            *reinterpret_cast<float2 *>(p) = make_float2(val[t.x], val[t.y]);
        } else {
            if (t.x >= 0) p[0] = val[t.x];
            if (t.y >= 0) p[1] = val[t.y];
        }
    }
}

// Table matrices (sm_set_table, sm_axpy_table).  One workgroup: thread t < table_size forms the
// new entry and stores it into the authoritative table and every layout's copy; the copies'
// entries past table_size (the 256-entry ones) are stored as 0, what the builders put there.
template <bool AXPY>
__global__ __launch_bounds__(kValThreads) void table_step_kernel(int32_t table_size, float a,
                                                                 const float *__restrict__ in, float *tab,
                                                                 TableDst dst) {
    const int32_t t = threadIdx.x;
    float v = 0.0f;
    if (t < table_size) {
        v = step(tab[t], a, in[t], AXPY);
        tab[t] = v;
    }
    for (int32_t i = 0; i < dst.count; ++i)
        if (t < dst.n[i]) dst.p[i][t] = v;
}

// val[e] = tab[ids[e]]: the table staged in LDS, four terms per lane and step (one 4-byte id
// load, one 16-byte store; ids and val are device allocations, so both are aligned), the tail
// one at a time.  Only val[0, nnz) is written.
__global__ __launch_bounds__(kValThreads) void values_from_table_kernel(int64_t nnz, const uint8_t *__restrict__ ids,
                                                                        const float *__restrict__ tab,
                                                                        float *__restrict__ val) {
    __shared__ float stab[256];
    stab[threadIdx.x] = tab[threadIdx.x];   // the authoritative table holds 256 floats
    __syncthreads();
    const int64_t n4 = nnz >> 2;
    const uint32_t *id4 = reinterpret_cast<const uint32_t *>(ids);
    float4 *val4 = reinterpret_cast<float4 *>(val);
    VAL_LOOP(i, n4) {
        const uint32_t w = id4[i];
        val4[i] = make_float4(stab[w & 255u], stab[(w >> 8) & 255u], stab[(w >> 16) & 255u], stab[w >> 24]);
    }
    VAL_LOOP(j, nnz - (n4 << 2)) {
        const int64_t e = (n4 << 2) + j;
        val[e] = stab[ids[e]];
    }
}

}  // namespace

hipError_t launch_table_step(int32_t table_size, bool axpy, float a, const float *in, float *tab,
                             const TableDst &dst, hipStream_t s) {
    if (table_size <= 0) return hipSuccess;
    static_assert(kValThreads == 256, "one thread per table slot");
    if (axpy) hipLaunchKernelGGL(table_step_kernel<true>, dim3(1), dim3(kValThreads), 0, s, table_size, a, in, tab, dst);
    else hipLaunchKernelGGL(table_step_kernel<false>, dim3(1), dim3(kValThreads), 0, s, table_size, a, in, tab, dst);
    return hipGetLastError();
}

hipError_t launch_values_from_table(int64_t nnz, const uint8_t *ids, const float *tab, float *val, hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(values_from_table_kernel, dim3(val_grid((nnz + 3) >> 2)), dim3(kValThreads), 0, s, nnz, ids,
                       tab, val);
    return hipGetLastError();
}

hipError_t launch_values_csr(int64_t nnz, bool axpy, float a, const float *in, const int32_t *src, float *val,
                             hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    if (src) {
        if (axpy)
            hipLaunchKernelGGL(values_src_kernel<true>, dim3(val_grid(nnz)), dim3(kValThreads), 0, s, nnz, a, in, src, val);
        else
            hipLaunchKernelGGL(values_src_kernel<false>, dim3(val_grid(nnz)), dim3(kValThreads), 0, s, nnz, a, in, src, val);
    } else if ((((uintptr_t)in | (uintptr_t)val) & 15) == 0) {
        const unsigned g = val_grid((nnz + 3) >> 2);
        if (axpy) hipLaunchKernelGGL(values_own4_kernel<true>, dim3(g), dim3(kValThreads), 0, s, nnz, a, in, val);
        else hipLaunchKernelGGL(values_own4_kernel<false>, dim3(g), dim3(kValThreads), 0, s, nnz, a, in, val);
    } else {
        if (axpy) hipLaunchKernelGGL(values_own1_kernel<true>, dim3(val_grid(nnz)), dim3(kValThreads), 0, s, nnz, a, in, val);
        else hipLaunchKernelGGL(values_own1_kernel<false>, dim3(val_grid(nnz)), dim3(kValThreads), 0, s, nnz, a, in, val);
    }
    return hipGetLastError();
}

hipError_t launch_refresh_plain(int64_t n_slots, const int32_t *map, const float *val, float *slot, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(refresh_plain_kernel, dim3(val_grid((n_slots + 3) >> 2)), dim3(kValThreads), 0, s, n_slots, map,
                       val, slot);
    return hipGetLastError();
}

hipError_t launch_refresh_entry(int64_t n_ent, const int32_t *map, const float *val, uint32_t *ent, hipStream_t s) {
    if (n_ent <= 0) return hipSuccess;
    hipLaunchKernelGGL(refresh_entry_kernel, dim3(val_grid(n_ent)), dim3(kValThreads), 0, s, n_ent,
                       reinterpret_cast<const int2 *>(map), val, ent);
    return hipGetLastError();
}

}  // namespace smamd
