// builddev_tiles.h -- the front and the middle that the two band builders on the device share
// (builddev_band2.hip: band2 / cband; builddev_gcb.hip: gcb).  Both cut a (row block, column
// slab) tile's terms, in (column, row) order, into bands, and both get there the same way:
//
//   keys    per term: its row (a search in row_ptr), key = block << cbits | column (a block's
//           columns ascending = its slabs in order, so the key order is the tile order), the row
//           in the block, and the check that the row's columns strictly ascend (the host builders
//           decline otherwise);
//   sort    one stable radix sort of (key, term) over the used bits: a tile is a contiguous run
//           ordered by (column, row) -- terms of one column stay in row order -- and every band
//           a contiguous sub-run of it;
//   gather  column, row in block and value bits (or codebook id) in sorted order;
//   tiles   every tile's first term, by a binary search of its first key;
//   cut     the builder's own: one workgroup per tile writes the band starts at the tile's term
//           offset + band index, and the tile's band count;
//   bands   an exclusive scan of the band counts (tile -> first band) and its total;
//   compact band starts by global band index, and each band's tile;
//   emit    the builder's own: one workgroup per band.
//
// run_tile_front is keys to tiles, BandScan and compact_bands the middle.  The LDS routines of
// cut and emit are here too: the block scan, the bitonic sort of a band's terms by (row,
// position) and the by-row segments of the sorted run, templates on the workgroup's threads.
// Device code; include from a .hip file only.
#pragma once
#include "band2_place.h"
#include "devprim.h"
#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kSortN = 2048;   // a band's terms at most, the bitonic width
constexpr int kPosBits = 11;   // sort key: row in block << kPosBits | position in the run
constexpr uint32_t kPosMask = (1u << kPosBits) - 1u;
constexpr uint32_t kPad = 0xFFFFFFFFu;
static_assert(kSortN == 1 << kPosBits, "a position in the run below kPosBits bits");

// One thread per term: key, row in block, term index; flag 1 = a row's columns not strictly
// ascending.
__global__ __launch_bounds__(256) void tile_keys_kernel(int64_t nnz, int64_t n_rows, const int32_t *__restrict__ rp,
                                                        const int32_t *__restrict__ col, int rows_log2, int cbits,
                                                        unsigned long long *__restrict__ key, int32_t *__restrict__ idx,
                                                        int32_t *__restrict__ rowl, int32_t *__restrict__ flag) {
    GS_LOOP(e, nnz) {
        int64_t lo = 0, hi = n_rows;   // the first r with rp[r] > e (rp[n_rows] = nnz > e)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)rp[mid] <= e) lo = mid + 1;
            else hi = mid;
        }
        const int64_t r = lo - 1;
        const int32_t c = col[e];
        if (e > (int64_t)rp[r] && c <= col[e - 1]) atomicOr(flag, 1);
        key[e] = ((unsigned long long)(r >> rows_log2) << cbits) | (unsigned)c;
        idx[e] = (int32_t)e;
        rowl[e] = (int32_t)(r & (((int64_t)1 << rows_log2) - 1));
    }
}

// Sorted order: column, row in block, and the value bits or (ids given) the codebook id.
__global__ __launch_bounds__(256) void tile_gather_kernel(int64_t n, const unsigned long long *__restrict__ skey,
                                                          const int32_t *__restrict__ sidx, const int32_t *__restrict__ rowl,
                                                          const float *__restrict__ val, const uint8_t *__restrict__ ids,
                                                          unsigned long long cmask, int32_t *__restrict__ scol,
                                                          int32_t *__restrict__ srl, uint32_t *__restrict__ sval) {
    GS_LOOP(i, n) {
        const int32_t e = sidx[i];
        scol[i] = (int32_t)(skey[i] & cmask);
        srl[i] = rowl[e];
        sval[i] = ids ? (uint32_t)ids[e] : __float_as_uint(val[e]);
    }
}

// Tile t = b * S + s starts at the first key >= (b << cbits) + the slab's first column.
__global__ __launch_bounds__(256) void tile_start_kernel(int64_t n_tiles, B2Slabs sl, int cbits, int64_t n,
                                                         const unsigned long long *__restrict__ skey,
                                                         int32_t *__restrict__ tts) {
    GS_LOOP(t, n_tiles + 1) {
        if (t == n_tiles) {
            tts[t] = (int32_t)n;
            continue;
        }
        const unsigned long long want = ((unsigned long long)(t / sl.ns) << cbits) + (unsigned long long)sl.lo(t % sl.ns);
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skey[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        tts[t] = (int32_t)lo;
    }
}

// Band starts by global band index, and each band's tile.
__global__ __launch_bounds__(256) void tile_compact_kernel(int64_t n_tiles, const int32_t *__restrict__ tts,
                                                           const int32_t *__restrict__ tbs,
                                                           const int32_t *__restrict__ bstart,
                                                           int32_t *__restrict__ gstart, int32_t *__restrict__ gtile) {
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t b0 = tbs[tile], nb = tbs[tile + 1] - b0;
        for (int32_t k = threadIdx.x; k < nb; k += blockDim.x) {
            gstart[b0 + k] = bstart[tts[tile] + k];
            gtile[b0 + k] = (int32_t)tile;
        }
    }
}

// ---- LDS routines of a cut or emit workgroup of NT threads --------------------------------------
// L is the kernel's LDS struct: key[kSortN] (uint32), crl[kSortN] and cpos[kSortN] (uint16) and
// wsum[NT / 64] (int32) at least.

// Exclusive block scan of one count per thread; the total in *tot.  Ends with a barrier.
template <int NT, class Lds>
__device__ __forceinline__ int block_scan(Lds &L, int v, int *tot) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) L.wsum[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const int s = L.wsum[k];
        before += k < w ? s : 0;
        all += s;
    }
    __syncthreads();   // wsum reused by the next scan
    *tot = all;
    return before + inc - v;
}

// Loads the run [a, a + n) (n <= kSortN) and sorts it by (row, position): position order = column
// order inside a row, the host builders' stable sort by row.
template <int NT, class Lds>
__device__ void band_sort(Lds &L, const int32_t *__restrict__ srl, int64_t a, int n) {
    const int t = threadIdx.x;
    for (int j = t; j < kSortN; j += NT) L.key[j] = j < n ? ((uint32_t)srl[a + j] << kPosBits) | (uint32_t)j : kPad;
    __syncthreads();
    for (int k = 2; k <= kSortN; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < kSortN / 2; p += NT) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int l = i | j;
                const uint32_t x = L.key[i], y = L.key[l];
                const bool up = (i & k) == 0;
                if ((x > y) == up) {
                    L.key[i] = y;
                    L.key[l] = x;
                }
            }
            __syncthreads();
        }
}

// The sorted run's entries of position < len, in (row, position) order, into L.crl / L.cpos, and
// their segments by row (the host builders' per-row runs inside the band).  Where a segment's
// record goes is the caller's: out.head(q, j, rl) for segment q, whose first kept entry is j and
// whose row is rl; out.entry(j, q) for every kept entry j, in segment q; out.end(nseg, len) once.
// Returns the segment count; ends with a barrier.  L.key is only read.
template <int NT, class Lds, class Out>
__device__ int band_segments(Lds &L, int len, const Out &out) {
    constexpr int E = kSortN / NT;   // entries per thread
    const int t = threadIdx.x;
    uint32_t k[E];
    int v = 0;
#pragma unroll
    for (int u = 0; u < E; ++u) {
        k[u] = L.key[t * E + u];
        v += k[u] != kPad && (int)(k[u] & kPosMask) < len;
    }
    int tot;
    int p = block_scan<NT>(L, v, &tot);
#pragma unroll
    for (int u = 0; u < E; ++u)
        if (k[u] != kPad && (int)(k[u] & kPosMask) < len) {
            L.crl[p] = (uint16_t)(k[u] >> kPosBits);
            L.cpos[p] = (uint16_t)(k[u] & kPosMask);
            ++p;
        }
    __syncthreads();
    // tot == len: every position < len is in the run exactly once.
    int h = 0;
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const int j = t * E + u;
        h += j < len && (j == 0 || L.crl[j] != L.crl[j - 1]);
    }
    int nseg;
    int q = block_scan<NT>(L, h, &nseg);
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const int j = t * E + u;
        if (j >= len) continue;
        if (j == 0 || L.crl[j] != L.crl[j - 1]) out.head(q++, j, L.crl[j]);
        out.entry(j, q - 1);
    }
    if (t == 0) out.end(nseg, len);
    __syncthreads();
    return nseg;
}

// ---- host side ------------------------------------------------------------------------------------

// A matrix's terms as the cut and emit kernels read them: sorted by (tile, column, row).
struct TileRun {
    int32_t *scol = nullptr, *srl = nullptr;   // column, row in block
    uint32_t *sval = nullptr;                  // value bits, or the codebook id
    int32_t *tts = nullptr;                    // tile -> first term; tts[ntile] = nnz
    int64_t ntile = 0;
    int32_t *flag = nullptr;                   // one zeroed word: emit reports a disagreement with cut there (2)
    bool unsorted = false;                     // a row's columns do not strictly ascend: nothing past the sort ran
};

// keys, sort, gather and tile starts of m's device CSR, in `tp`: block = row >> rows_log2, nblk
// of them, slabs `sl`; `ids` (or null) replaces the values.  What a later phase does not read is
// released as soon as it is read last, so the peak is key, skey, idx, sidx, rowl and the sort's
// temporary.  Any failure is returned as it is: the caller maps it (scratch out of memory included)
// to its own decline or error, and `unsorted` to its decline.
inline hipError_t run_tile_front(DevScratch &tp, const sm_matrix *m, const uint8_t *ids, int rows_log2, int64_t nblk,
                                 const B2Slabs &sl, TileRun &run, hipStream_t s) {
    const int64_t nnz = m->nnz;
    run.ntile = nblk * sl.ns;
    const int cbits = bits_for((uint64_t)(m->n_cols - 1));
    const int end_bit = cbits + bits_for((uint64_t)std::max<int64_t>(nblk - 1, 1));
    unsigned long long *key = nullptr, *skey = nullptr;
    int32_t *idx = nullptr, *sidx = nullptr, *rowl = nullptr;
    DEV_TRY_RET(tp.alloc(&key, nnz));
    DEV_TRY_RET(tp.alloc(&skey, nnz));
    DEV_TRY_RET(tp.alloc(&idx, nnz));
    DEV_TRY_RET(tp.alloc(&sidx, nnz));
    DEV_TRY_RET(tp.alloc(&rowl, nnz));
    DEV_TRY_RET(tp.alloc(&run.flag, 1));
    DEV_TRY_RET(hipMemsetAsync(run.flag, 0, 4, s));
    hipLaunchKernelGGL(tile_keys_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, m->n_rows, m->d_row_ptr, m->d_col,
                       rows_log2, cbits, key, idx, rowl, run.flag);
    DEV_TRY_RET(hipGetLastError());
    DEV_TRY_RET(dev_sort_pairs(tp, key, skey, idx, sidx, nnz, end_bit, s, true));
    int32_t fl = 0;
    DEV_TRY_RET(hipMemcpyAsync(&fl, run.flag, 4, hipMemcpyDeviceToHost, s));
    DEV_TRY_RET(hipStreamSynchronize(s));
    run.unsorted = fl != 0;
    if (run.unsorted) return hipSuccess;
    tp.release(key);
    tp.release(idx);
    DEV_TRY_RET(tp.alloc(&run.scol, nnz));
    DEV_TRY_RET(tp.alloc(&run.srl, nnz));
    DEV_TRY_RET(tp.alloc(&run.sval, nnz));
    DEV_TRY_RET(tp.alloc(&run.tts, run.ntile + 1));
    const unsigned long long cmask = ((unsigned long long)1 << cbits) - 1;
    hipLaunchKernelGGL(tile_gather_kernel, dim3(grid_of(nnz)), dim3(256), 0, s, nnz, skey, sidx, rowl, m->d_val, ids, cmask,
                       run.scol, run.srl, run.sval);
    hipLaunchKernelGGL(tile_start_kernel, dim3(grid_of(run.ntile + 1)), dim3(256), 0, s, run.ntile, sl, cbits, nnz, skey,
                       run.tts);
    DEV_TRY_RET(hipGetLastError());
    DEV_TRY_RET(hipStreamSynchronize(s));
    tp.release(skey);
    tp.release(sidx);
    tp.release(rowl);
    return hipSuccess;
}

// The scan of the tiles' band counts.  Its temporary is allocated once, ahead of the cut, so
// that a builder that cuts more than once (band2's geometries) allocates nothing in between.
struct BandScan {
    uint8_t *tmp = nullptr;
    size_t bytes = 0;
    int64_t n = 0;   // ntile + 1

    hipError_t prepare(DevScratch &tp, int64_t ntile) {
        n = ntile + 1;
        const int32_t *none = nullptr;
        DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, none, (int32_t *)nullptr, (int)n, (hipStream_t)0));
        return tp.alloc(&tmp, (int64_t)bytes);
    }
    // tbs[t] = the bands before tile t (nb[ntile] = 0 set by the caller); the total to the host.
    // Waits for the stream.
    hipError_t run(const int32_t *nb, int32_t *tbs, int32_t *n_bands, hipStream_t s) {
        DEV_TRY_RET(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, nb, tbs, (int)n, s));
        DEV_TRY_RET(hipMemcpyAsync(n_bands, tbs + n - 1, 4, hipMemcpyDeviceToHost, s));
        return hipStreamSynchronize(s);
    }
};

// gstart / gtile of the n_bands bands (in `tp`) from the cut's per-tile band starts.
inline hipError_t compact_bands(DevScratch &tp, const TileRun &run, const int32_t *tbs, const int32_t *bstart,
                                int32_t n_bands, int32_t **gstart, int32_t **gtile, hipStream_t s) {
    DEV_TRY_RET(tp.alloc(gstart, n_bands));
    DEV_TRY_RET(tp.alloc(gtile, n_bands));
    hipLaunchKernelGGL(tile_compact_kernel, dim3((unsigned)std::min<int64_t>(run.ntile, 1 << 16)), dim3(256), 0, s,
                       run.ntile, run.tts, tbs, bstart, *gstart, *gtile);
    return hipGetLastError();
}

}  // namespace
}  // namespace smamd
