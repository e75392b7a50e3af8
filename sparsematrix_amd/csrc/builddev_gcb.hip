// builddev_gcb.hip -- the gathered chunk bands (gcb.h) built on the device from a device CSR
// (config 5's host build took 15 s).  The same bytes gcb.cpp's gcb_build
// produces -- every band's start, its 4096 words and the tile -> band offsets -- without copying
// the terms to the host and back.  The sorted run of terms, the tile starts, the scan of the band
// counts and the LDS sort / scan / segment routines are builddev_tiles.h, shared with
// builddev_band2.hip; gcb's own:
//
//   cut     one workgroup per tile runs gcb.cpp's greedy: the longest next run within the window
//           and the capacity, shrunk by 31/32 until its by-row segments pack into 32 chunks.  One
//           wave replays the sequential packing with the segment list in its lanes (s_ registers
//           hold the packing state);
//   emit    one workgroup per band repeats the sort and the packing of its (now known) run and
//           writes the band's image -- headers, words, values, zero padding -- from LDS in one
//           coalesced pass.
#include <algorithm>

#include "builddev_tiles.h"
#include "gcb.h"
#include "sm_internal.h"

namespace smamd {
namespace {

constexpr int kCutThreads = 1024;
constexpr int kCap = kGcbChunks * kGcbChunkTerms;   // 2016 terms per band at most
static_assert(kCap <= kSortN && kSortN == 2 * kCutThreads, "one compare per thread per stage");

// LDS of one band's packing.
struct BandLds {
    uint32_t key[kSortN];          // (row << 11 | position), sorted; kPad beyond the run
    uint16_t crl[kSortN];          // kept entries in (row, position) order: row (< 2^15)
    uint16_t cpos[kSortN];         //   position in the run
    uint16_t cseg[kSortN];         //   segment
    int32_t seg_first[kSortN + 1]; // segment -> first kept entry
    uint16_t seg_rl[kSortN];
    uint8_t seg_chunk[kSortN];
    uint16_t seg_lane[kSortN];     // lane of the segment's first term
    int32_t cbase[kGcbChunks];
    int32_t wsum[kCutThreads / 64];
    int32_t nseg, ok, len;
};

// Where band_segments writes gcb's segment records.
struct GcbSegs {
    BandLds &L;
    __device__ void head(int q, int j, int rl) const {
        L.seg_first[q] = j;
        L.seg_rl[q] = (uint16_t)rl;
    }
    __device__ void entry(int j, int q) const { L.cseg[j] = (uint16_t)q; }
    __device__ void end(int nseg, int len) const { L.seg_first[nseg] = len; }
};

// Packs the sorted run's entries of position < len (gcb.cpp segments + pack): segments by row,
// a segment never split, a chunk's rows spanning < 4096, at most 32 chunks of 63 terms.  Sets
// L.ok; on success the segment -> (chunk, lane) map and the chunk bases.  All threads return
// after a barrier.
__device__ void band_pack(BandLds &L, int len) {
    const int t = threadIdx.x;
    const int nseg = band_segments<kCutThreads>(L, len, GcbSegs{L});
    if (t < 64) {
        const int lane = t;
        int fill = kGcbChunkTerms, chunks = 0, base = 0, my_base = 0;
        bool bad = false;
        for (int g0 = 0; g0 < nseg && !bad; g0 += 64) {
            const int g = g0 + lane;
            const int grl = g < nseg ? L.seg_rl[g] : 0;
            const int gn = g < nseg ? L.seg_first[g + 1] - L.seg_first[g] : 0;
            int my_c = 0, my_l = 0;
            const int m = min(64, nseg - g0);
            for (int u = 0; u < m; ++u) {
                const int r = __builtin_amdgcn_readlane(grl, u);
                const int n = __builtin_amdgcn_readlane(gn, u);
                if (n > kGcbChunkTerms) {   // a row's segment must fit one chunk
                    bad = true;
                    break;
                }
                if (fill + n > kGcbChunkTerms || r - base >= kGcbRowSpan) {
                    ++chunks;
                    fill = 0;
                    base = r;
                    if (chunks > kGcbChunks) {
                        bad = true;
                        break;
                    }
                    my_base = lane == chunks - 1 ? r : my_base;
                }
                my_c = lane == u ? chunks - 1 : my_c;
                my_l = lane == u ? fill + 1 : my_l;
                fill += n;
            }
            if (g < nseg) {
                L.seg_chunk[g] = (uint8_t)my_c;
                L.seg_lane[g] = (uint16_t)my_l;
            }
        }
        if (lane < kGcbChunks) L.cbase[lane] = my_base;
        if (lane == 0) {
            L.ok = bad ? 0 : 1;
            L.nseg = nseg;
        }
    }
    __syncthreads();
}

// One workgroup per tile: the band starts (gcb.cpp build_tile's loop), written at the tile's
// term offset + band index; the band count per tile.
__global__ __launch_bounds__(kCutThreads) void gk_cut_kernel(const int32_t *__restrict__ tts,
                                                             const int32_t *__restrict__ scol,
                                                             const int32_t *__restrict__ srl, int32_t window,
                                                             int32_t *__restrict__ bstart, int32_t *__restrict__ nbands) {
    __shared__ BandLds L;
    const int64_t tile = blockIdx.x;
    const int64_t t0 = tts[tile], t1 = tts[tile + 1];
    const int t = threadIdx.x;
    int32_t k = 0;
    for (int64_t a = t0; a < t1;) {
        const int64_t bmax = min(t1, a + (int64_t)kCap);
        const int32_t clo = scol[a];
        // b = the first term at or past clo + window (the run is sorted by column); at most
        // kCap < 2 * kCutThreads candidates
        const int in0 = a + t < bmax && scol[a + t] < clo + window;
        const int in1 = a + t + kCutThreads < bmax && scol[a + t + kCutThreads] < clo + window;
        const int n = __syncthreads_count(in0) + __syncthreads_count(in1);
        band_sort<kCutThreads>(L, srl, a, n);
        int len = n;
        for (;;) {
            band_pack(L, len);
            if (L.ok) break;
            len = max(1, len * 31 / 32);
            __syncthreads();   // every thread read L.ok before the next pack rewrites it
        }
        if (t == 0) bstart[t0 + k] = (int32_t)a;
        ++k;
        a += len;
        __syncthreads();
    }
    if (t == 0) nbands[tile] = k;
}

// One workgroup per band: its image (gcb.cpp build_tile's emission) through LDS.
__global__ __launch_bounds__(kCutThreads) void gk_emit_kernel(int64_t n_bands, const int32_t *__restrict__ tts,
                                                              const int32_t *__restrict__ gstart,
                                                              const int32_t *__restrict__ gtile,
                                                              const int32_t *__restrict__ scol,
                                                              const int32_t *__restrict__ srl,
                                                              const uint32_t *__restrict__ sval,
                                                              int32_t *__restrict__ band_clo, uint32_t *__restrict__ word,
                                                              int32_t *__restrict__ flag) {
    __shared__ BandLds L;
    __shared__ uint32_t img[kGcbBandWords];
    const int64_t g = blockIdx.x;
    const int t = threadIdx.x;
    const int32_t tile = gtile[g];
    const int64_t a = gstart[g];
    const int64_t b = g + 1 < n_bands && gtile[g + 1] == tile ? (int64_t)gstart[g + 1] : (int64_t)tts[tile + 1];
    const int n = (int)(b - a);
    if (n < 1 || n > kCap) {   // uniform: cut and emit disagree (a builder bug)
        if (t == 0) atomicOr(flag, 2);
        return;
    }
    for (int i = t; i < kGcbBandWords; i += kCutThreads) img[i] = 0u;
    band_sort<kCutThreads>(L, srl, a, n);
    band_pack(L, n);
    if (!L.ok) {
        if (t == 0) atomicOr(flag, 2);
        return;
    }
    const int32_t clo = scol[a];
    const int nseg = L.nseg;
    for (int q = t; q < nseg; q += kCutThreads)
        if (q == 0 || L.seg_chunk[q] != L.seg_chunk[q - 1]) {   // a chunk's first segment
            const int c = L.seg_chunk[q];
            img[(c >> 1) * 64 * 4 + (c & 1)] = (uint32_t)L.cbase[c];   // header: the chunk's base row
        }
    for (int j = t; j < n; j += kCutThreads) {
        const int q = L.cseg[j];
        const int c = L.seg_chunk[q];
        const int first = L.seg_first[q];
        const int lane = L.seg_lane[q] + (j - first);
        const int p = L.cpos[j];
        const int k = c & 1;
        const uint32_t w = (uint32_t)(scol[a + p] - clo) | ((uint32_t)((int)L.crl[j] - L.cbase[c]) << kGcbColBits) |
                           kGcbLive | (j > first ? kGcbCont : 0u);
        const int slot = ((c >> 1) * 64 + lane) * 4;
        img[slot + k] = w;
        img[slot + 2 + k] = sval[a + p];
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(word + g * kGcbBandWords);
    const uint4 *src = reinterpret_cast<const uint4 *>(img);
    for (int i = t; i < kGcbBandWords / 4; i += kCutThreads) dst[i] = src[i];
    if (t == 0) band_clo[g] = clo;
}

}  // namespace

// Every HIP failure is an error (-5), scratch out of memory included: unlike devbuild_band2,
// which declines to the host builder on that one.
int devbuild_gcb(sm_matrix *m, int rows_log2, int32_t n_slabs, int32_t window, GcbHost &meta, hipStream_t s,
                 hipError_t &err) {
    err = hipSuccess;
    meta = GcbHost();
    const int64_t n_rows = m->n_rows, n_cols = m->n_cols, nnz = m->nnz;
    // gcb_build's limits
    if (rows_log2 < 6 || rows_log2 > 15 || window < 64 || window > kGcbMaxWindow) return 1;
    if (n_rows <= 0 || n_cols <= 0 || n_slabs < 1 || n_cols >= ((int64_t)1 << 30) || nnz <= 0) return 1;
    const int32_t br = (int32_t)std::min<int64_t>((int64_t)1 << rows_log2, n_rows);
    const int64_t nblk = (n_rows + br - 1) / br;
    const B2Slabs sl = b2_slabs(n_cols, n_slabs, 1000);   // even slabs of whole 256-column pieces
    const int64_t ntile = nblk * sl.ns;
    if (ntile >= ((int64_t)1 << 30)) return 1;
    DevScratch tp;
    TileRun run;
    DEV_TRY(run_tile_front(tp, m, nullptr, rows_log2, nblk, sl, run, s));
    if (run.unsorted) return 1;   // a row's columns not strictly ascending (gcb_build declines)
    // cut
    int32_t *bstart = nullptr, *nb = nullptr, *mx = nullptr;
    DEV_TRY(tp.alloc(&bstart, nnz));
    DEV_TRY(tp.alloc(&nb, ntile + 1));
    DEV_TRY(tp.alloc(&mx, 1));
    DEV_TRY(hipMemsetAsync(nb + ntile, 0, 4, s));
    DEV_TRY(hipMemsetAsync(mx, 0, 4, s));
    hipLaunchKernelGGL(gk_cut_kernel, dim3((unsigned)ntile), dim3(kCutThreads), 0, s, run.tts, run.scol, run.srl, window,
                       bstart, nb);
    DEV_TRY(hipGetLastError());
    DEV_TRY(m->mem.alloc(&m->plan.gcb.d_tile_band, ntile + 1));
    int32_t *tbs = m->plan.gcb.d_tile_band;
    BandScan scan;
    DEV_TRY(scan.prepare(tp, ntile));
    hipLaunchKernelGGL(max_i32_kernel<>, dim3(grid_of(ntile)), dim3(256), 0, s, ntile, nb, mx);
    DEV_TRY(hipGetLastError());
    int32_t n_bands = 0, max_bands = 0;
    DEV_TRY(hipMemcpyAsync(&max_bands, mx, 4, hipMemcpyDeviceToHost, s));
    DEV_TRY(scan.run(nb, tbs, &n_bands, s));
    // gcb_build's output limits: a tile's bands under 4 GiB of 32-bit byte offsets.
    if ((int64_t)max_bands * kGcbBandWords * 4 >= ((int64_t)1 << 32) || n_bands <= 0 || n_bands >= INT32_MAX) return 1;
    int32_t *gstart = nullptr, *gtile = nullptr;
    DEV_TRY(compact_bands(tp, run, tbs, bstart, n_bands, &gstart, &gtile, s));
    GcbDev &d = m->plan.gcb;
    DEV_TRY(m->mem.alloc(&d.d_band_clo, n_bands));
    DEV_TRY(m->mem.alloc(&d.d_ent, (int64_t)n_bands * kGcbBandWords));
    hipLaunchKernelGGL(gk_emit_kernel, dim3((unsigned)n_bands), dim3(kCutThreads), 0, s, (int64_t)n_bands, run.tts,
                       gstart, gtile, run.scol, run.srl, run.sval, d.d_band_clo, d.d_ent, run.flag);
    DEV_TRY(hipGetLastError());
    int32_t fl = 0;
    DEV_TRY(hipMemcpyAsync(&fl, run.flag, 4, hipMemcpyDeviceToHost, s));
    DEV_TRY(hipStreamSynchronize(s));
    if (fl) {   // the emission's packing disagreed with the cut's: a builder bug, not a decline
        err = hipErrorUnknown;
        return -6;
    }
    meta.rows_log2 = rows_log2;
    meta.window = window;
    meta.block_rows = br;
    meta.n_blocks = (int32_t)nblk;
    meta.n_slabs = (int32_t)sl.ns;
    meta.slab_cols = (int32_t)sl.sc;
    meta.max_bands_per_tile = max_bands;
    meta.n_bands = n_bands;
    meta.real_terms = nnz;
    return 0;
}

}  // namespace smamd
