// builddev_band2.hip -- the balanced bands (xband.h Band2Host: band2's 8-byte entries, cband's
// codebook words) built on the device from a device CSR: the bytes band2.cpp's band2_build
// produces, as layouts.cpp's build_band2 chooses them, without copying the terms to the host
// and the layout back.  The placement heuristics are band2_place.h, the code the host runs.
// The sorted run of terms, the tile starts, the scan of the band counts and the LDS sort / scan /
// segment routines are builddev_tiles.h, shared with builddev_gcb.hip; band2's own:
//
//   cut     one workgroup per tile replays build_tile's loop: the band's last column from the
//           window and the term capacity (a look-up in the sorted run), the cut inside a row
//           segment too long for one chunk, the 31/32 shrink until the by-row segments pack
//           into the band's chunks, the by-row split of a one-column band (the by-row pieces of
//           a hub column are contiguous sub-runs too).  One thread replays the packing;
//   choose  on the host, from the band count alone (every term lands in a band): dma3 bands
//           first, wide ones where those would be under 70 % full, else declined;
//   emit    one wave per band repeats the sort and the segments of its run, balances its chunks
//           (a lane per candidate, the least score by a wave minimum, its first lane by a
//           ballot), places each chunk's lanes with one lane per chunk, and writes the image
//           from LDS in one coalesced pass.  (One thread per band for the balance took 1.3 s on
//           config 2, against 0.38 s on the host and 0.12 s this way: profiles/band_devbuild.txt.)
#include <algorithm>
#include <vector>

#include "band2_place.h"
#include "builddev_tiles.h"
#include "sm_internal.h"
#include "xband.h"

namespace smamd {
namespace {

constexpr int kNT = 256;                 // threads of a cut workgroup
constexpr int kET = 64;                  // threads of an emit workgroup: one wave
constexpr int kMaxChunks = 32;           // of 64 terms: kSortN
constexpr int kRowsLog2 = 14;            // both kernel geometries: 16K-row blocks
static_assert(kB2Wide.block_rows == 1 << kRowsLog2 && kB2Dma3Cb.block_rows == 1 << kRowsLog2 &&
                  kB2Dma3B2.block_rows == 1 << kRowsLog2,
              "row keys: rows in block below kRowsLog2 bits");
static_assert(kRowsLog2 + kPosBits <= 31, "sort key: row in block | position, below the pad");

// LDS of one band's packing.
struct BandLds {
    uint32_t key[kSortN];        // (row << 11 | position), sorted; kPad beyond the run
    uint16_t crl[kSortN];        // kept entries in (row, position) order: row in block
    uint16_t cpos[kSortN];       //   position in the run
    B2Seg segs[kSortN + 1];      // segments by row: s = first kept entry (segs[nseg].s = the entries)
    int32_t wsum[kNT / 64];
    int32_t cut, chunks, len, ok;
};

// The first index in [lo, hi) with v[index] >= x (hi when none); v ascending.
__device__ __forceinline__ int64_t lower_bound_dev(const int32_t *__restrict__ v, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Where band_segments writes band2's segment records.
struct B2Segs {
    BandLds &L;
    __device__ void head(int q, int j, int rl) const {
        L.segs[q].rl = rl;
        L.segs[q].s = j;
    }
    __device__ void entry(int, int) const {}
    __device__ void end(int nseg, int len) const { L.segs[nseg].s = len; }
};

// band_segments into L.segs, with every segment's length.  Ends with a barrier.
template <int NT>
__device__ int b2_segments(BandLds &L, int len) {
    const int nseg = band_segments<NT>(L, len, B2Segs{L});
    for (int g = threadIdx.x; g < nseg; g += NT) L.segs[g].n = L.segs[g + 1].s - L.segs[g].s;
    __syncthreads();
    return nseg;
}

// One workgroup per tile (grid stride): the band starts (band2.cpp build_tile's loop), written
// at the tile's term offset + band index; the band count per tile.
__global__ __launch_bounds__(kNT) void b2_cut_kernel(int64_t n_tiles, B2Slabs sl, const int32_t *__restrict__ tts,
                                                     const int32_t *__restrict__ scol, const int32_t *__restrict__ srl,
                                                     B2Geom geom, int cb, int32_t *__restrict__ bstart,
                                                     int32_t *__restrict__ nbands) {
    __shared__ BandLds L;
    const int t = threadIdx.x;
    const B2Pack pk = b2_pack(cb != 0, geom);
    const int nchunks = geom.chunks();
    const int64_t cap_terms = (int64_t)nchunks * 64;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t t0 = tts[tile], t1 = tts[tile + 1];
        const int64_t c1 = sl.lo(tile % sl.ns + 1);
        int32_t nb = 0;
        for (int64_t a = t0; a < t1;) {
            // The band starts at the next term's column (no band starts on an empty column; a
            // column split by rows continues with its next row).
            const int64_t clo = scol[a], clo_al = clo & ~(int64_t)3;
            const int64_t lim = min(c1, clo_al + (int64_t)geom.window);
            // Largest chi <= lim with at most nchunks * 64 of the tile's terms in [clo, chi):
            // those terms start at the column's first term (before a when the column is split).
            const int64_t first = lower_bound_dev(scol, t0, a, clo);
            const int64_t q = first + cap_terms;
            int64_t chi = q >= t1 ? lim : min(lim, (int64_t)scol[q]);
            chi = max(chi, clo + 1);
            // More than kSortN terms only in a one-column band, already in row order: the
            // first kSortN are all a band can take.
            int len = (int)min(lower_bound_dev(scol, a, t1, chi) - a, (int64_t)kSortN);
            band_sort<kNT>(L, srl, a, len);
            for (;;) {   // pack; shrink chi until the band fits
                const bool single = chi == clo + 1;
                if (t == 0) L.cut = INT32_MAX;
                const int nseg = b2_segments<kNT>(L, len);
                // A row's segment longer than a chunk (band2: the rank field) cuts the band at
                // that row's first column past it.
                for (int g = t; g < nseg; g += kNT)
                    if (L.segs[g].n > pk.max_seg) atomicMin(&L.cut, scol[a + L.cpos[L.segs[g].s + pk.max_seg]]);
                __syncthreads();
                const int32_t cut = L.cut;
                if (cut != INT32_MAX) {
                    chi = cut;
                    len = (int)(lower_bound_dev(scol, a, a + len, chi) - a);
                    __syncthreads();   // every thread read L.cut before it is reset
                    continue;
                }
                if (t == 0) {
                    int chunks = 0, fill = pk.cap, used = 0;
                    int32_t base = 0;
                    for (int g = 0; g < nseg; ++g) {
                        const int32_t rl = L.segs[g].rl, n = L.segs[g].n;
                        if (b2_opens(pk, fill, base, rl, n)) {
                            if (single && chunks == nchunks) break;   // split: the rest goes to the next band
                            if (++chunks > nchunks) break;
                            fill = 0;
                            base = rl;
                        }
                        fill += n;
                        used += n;
                    }
                    L.chunks = chunks;
                    L.len = used;
                }
                __syncthreads();
                const int chunks = L.chunks, used = L.len;
                __syncthreads();   // read before the next round rewrites them
                if (chunks > nchunks) {
                    chi = clo + max((int64_t)1, (chi - clo) * 31 / 32);
                    len = (int)(lower_bound_dev(scol, a, a + len, chi) - a);
                    continue;
                }
                len = used;
                break;
            }
            if (t == 0) bstart[t0 + nb] = (int32_t)a;
            ++nb;
            a += max(len, 1);   // a band holds its first term at least
        }
        if (t == 0) nbands[tile] = nb;
    }
}

// Bank counts of the two chunks of a pair (b2_balance_chunks' A and B).
struct BalanceLds {
    int32_t cx[2][32], cy[2][32];
};

__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// b2_chunk_stats of chunk `segs` (n <= 64 segments, one per lane) into W.cx[w] / W.cy[w] and the
// two smallest / largest rows (rows of a chunk are distinct).  One wave; ends with a barrier.
__device__ void chunk_stats_wave(BalanceLds &W, int w, const B2Seg *segs, int n, const int32_t *col, int32_t clo_al,
                                 int32_t &mn, int32_t &mn2, int32_t &mx, int32_t &mx2) {
    const int lane = threadIdx.x;
    if (lane < 32) W.cx[w][lane] = W.cy[w][lane] = 0;
    __syncthreads();
    int32_t rl = 0;
    if (lane < n) {
        const B2Seg g = segs[lane];
        rl = g.rl;
        for (int32_t j = 0; j < g.n; j++) atomicAdd(&W.cx[w][(col[g.s + j] - clo_al) & 31], 1);
        atomicAdd(&W.cy[w][g.rl & 31], 1);
    }
    const int32_t lo = lane < n ? rl : INT32_MAX, hi = lane < n ? rl : INT32_MIN;
    mn = wave_min(lo);
    mn2 = wave_min(lo == mn ? INT32_MAX : lo);
    mx = wave_max(hi);
    mx2 = wave_max(hi == mx ? INT32_MIN : hi);
    __syncthreads();
}

// b2_balance_chunks (band2_place.h) with one wave: the candidates of chunk b sit one per lane
// (lane = the segment's index in b, so the first lane of least score is the host's first least
// k), every hot single of chunk a is scored by all lanes at once, and the least score and its
// first lane come from a wave minimum and a ballot.  The same swaps in the same order; pinned to
// the host function by the layout digests (tests/test_gpu_devbuild_band2.py).  The workgroup is
// this one wave (kET), so __syncthreads orders its LDS accesses.
__device__ void balance_chunks_wave(B2Seg *segs, const int32_t *cstart, int nc, const int32_t *col, int32_t clo_al,
                                    int32_t span, BalanceLds &W) {
    constexpr int hot = 3;
    const int lane = threadIdx.x;
    for (int a = 0; a + 1 < nc; a++) {
        B2Seg *sa = segs + cstart[a], *sb = segs + cstart[a + 1];
        const int na = cstart[a + 1] - cstart[a], nb = cstart[a + 2] - cstart[a + 1];
        for (int it = 0; it < 16; it++) {
            int32_t Amn, Amn2, Amx, Amx2, Bmn, Bmn2, Bmx, Bmx2;
            chunk_stats_wave(W, 0, sa, na, col, clo_al, Amn, Amn2, Amx, Amx2);
            chunk_stats_wave(W, 1, sb, nb, col, clo_al, Bmn, Bmn2, Bmx, Bmx2);
            // this lane's candidate: segment `lane` of b when it is a single term
            const B2Seg t = lane < nb ? sb[lane] : B2Seg{0, 0, 0};
            const bool cand = lane < nb && t.n == 1;
            int32_t crl = 0, clo = INT32_MAX, chi = INT32_MIN, cxt = 0, cyt = 0, cpx = 0, cpy = 0;
            if (cand) {
                cxt = (col[t.s] - clo_al) & 31;
                cyt = t.rl & 31;
                const int32_t bmn = t.rl == Bmn ? Bmn2 : Bmn, bmx = t.rl == Bmx ? Bmx2 : Bmx;
                crl = t.rl;
                clo = b2_win_lo(bmn, bmx, span);
                chi = b2_win_hi(bmn, bmx, span);
                if (bmn != INT32_MAX && bmx - bmn >= span) clo = INT32_MAX;   // (never)
                cpx = W.cx[0][cxt] - W.cx[1][cxt];
                cpy = W.cy[0][cyt] - W.cy[1][cyt];
            }
            const unsigned long long cmask = __ballot(cand);
            const int nt = __popcll(cmask);
            const int32_t minpx = wave_min(cand ? cpx : INT32_MAX), minpy = wave_min(cand ? cpy : INT32_MAX);
            int best_i = -1, best_j = -1, best = 0;
            for (int i = 0; i < na; i++) {   // uniform across the wave
                const B2Seg s_ = sa[i];
                if (s_.n != 1) continue;
                const int xs = (col[s_.s] - clo_al) & 31, ys = s_.rl & 31;
                const int32_t acx = W.cx[0][xs], acy = W.cy[0][ys];
                if (acx < hot && acy < hot) continue;
                const int32_t amn = s_.rl == Amn ? Amn2 : Amn, amx = s_.rl == Amx ? Amx2 : Amx;
                if (amn != INT32_MAX && amx - amn >= span) continue;   // (never)
                const int32_t alo = b2_win_lo(amn, amx, span), ahi = b2_win_hi(amn, amx, span), srl = s_.rl;
                const int qx = W.cx[1][xs] - acx + 2, qy = W.cy[1][ys] - acy + 2;
                if (nt == 0 || 2 * b2_min(0, minpx + qx) + 2 * b2_min(0, minpy + qy) >= best) continue;
                const int d = 2 * (cpx + qx) * (int)(xs != cxt) + 2 * (cpy + qy) * (int)(ys != cyt);
                const bool ok = cand && crl >= alo && crl <= ahi && srl >= clo && srl <= chi;
                const int32_t dv = ok ? d : INT32_MAX;
                const int32_t mn = wave_min(dv);
                if (mn >= best) continue;
                best = mn;
                best_i = i;
                best_j = __ffsll((long long)__ballot(dv == mn)) - 1;
            }
            if (best_i < 0) break;
            __syncthreads();
            if (lane == 0) {
                const B2Seg tmp = sa[best_i];
                sa[best_i] = sb[best_j];
                sb[best_j] = tmp;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (lane < nc) {   // b2_emit_chunk: segments in row order, the first is the base
        B2Seg *s = segs + cstart[lane];
        const int n = cstart[lane + 1] - cstart[lane];
        for (int i = 1; i < n; i++) {
            const B2Seg g = s[i];
            int j = i;
            for (; j > 0 && s[j - 1].rl > g.rl; j--) s[j] = s[j - 1];
            s[j] = g;
        }
    }
    __syncthreads();
}

// One wave per band (grid stride): its image (build_tile's emission) through LDS.  flag 2:
// the band's run does not pack as the cut said (a builder bug).
__global__ __launch_bounds__(kET) void b2_emit_kernel(int64_t n_bands, const int32_t *__restrict__ tts,
                                                      const int32_t *__restrict__ gstart,
                                                      const int32_t *__restrict__ gtile,
                                                      const int32_t *__restrict__ scol, const int32_t *__restrict__ srl,
                                                      const uint32_t *__restrict__ sv, B2Geom geom, int cb,
                                                      int32_t *__restrict__ band_clo, uint32_t *__restrict__ ent,
                                                      int32_t *__restrict__ flag) {
    __shared__ BandLds L;
    __shared__ __attribute__((aligned(16))) uint32_t img[128 * kMaxChunks];
    __shared__ uint32_t lv[kSortN];          // the entries' value bits, or (cband) their ids as bytes
    __shared__ int32_t cstart[kMaxChunks + 1];
    __shared__ BalanceLds W;
    const int t = threadIdx.x;
    const B2Pack pk = b2_pack(cb != 0, geom);
    const int nchunks = geom.chunks();
    const int band_words = (cb ? 64 : 128) * nchunks;
    int32_t *lcol = reinterpret_cast<int32_t *>(L.key);   // the entries' columns, once the keys are read
    for (int64_t g = blockIdx.x; g < n_bands; g += gridDim.x) {
        const int32_t tile = gtile[g];
        const int64_t a = gstart[g];
        const int64_t b = g + 1 < n_bands && gtile[g + 1] == tile ? (int64_t)gstart[g + 1] : (int64_t)tts[tile + 1];
        const int n = (int)(b - a);
        if (b - a < 1 || b - a > kSortN) {   // uniform
            if (t == 0) atomicOr(flag, 2);
            continue;
        }
        for (int i = t; i < band_words; i += kET) img[i] = 0u;   // dummies: word 0, value 0
        band_sort<kET>(L, srl, a, n);
        const int nseg = b2_segments<kET>(L, n);
        const int32_t clo_al = scol[a] & ~3;
        for (int j = t; j < n; j += kET) {
            const int p = L.cpos[j];
            lcol[j] = scol[a + p];
            if (cb) reinterpret_cast<uint8_t *>(lv)[j] = (uint8_t)sv[a + p];
            else lv[j] = sv[a + p];
        }
        if (t == 0) {   // segments into chunks in row order
            int c = -1, fill = pk.cap;
            int32_t base = 0;
            bool bad = false;
            for (int q = 0; q < nseg && !bad; ++q) {
                const int32_t rl = L.segs[q].rl, sn = L.segs[q].n;
                if (sn > pk.max_seg) bad = true;
                if (b2_opens(pk, fill, base, rl, sn)) {
                    if (++c >= nchunks) {
                        bad = true;
                        break;
                    }
                    fill = 0;
                    base = rl;
                    cstart[c] = q;
                }
                fill += sn;
            }
            if (!bad) cstart[c + 1] = nseg;
            L.chunks = c + 1;
            L.ok = bad ? 0 : 1;
        }
        __syncthreads();
        const int nc = L.chunks;
        if (!L.ok) {   // uniform
            if (t == 0) atomicOr(flag, 2);
            __syncthreads();
            continue;
        }
        balance_chunks_wave(L.segs, cstart, nc, lcol, clo_al, pk.span, W);
        if (t < nc)
            b2_emit_chunk(img, nullptr, t, L.segs + cstart[t], cstart[t + 1] - cstart[t], lcol,
                          reinterpret_cast<const float *>(lv), cb ? reinterpret_cast<const uint8_t *>(lv) : nullptr,
                          clo_al, geom);
        __syncthreads();
        uint4 *dst = reinterpret_cast<uint4 *>(ent + g * (int64_t)band_words);
        const uint4 *src = reinterpret_cast<const uint4 *>(img);
        for (int i = t; i < band_words / 4; i += kET) dst[i] = src[i];
        if (t == 0) band_clo[g] = clo_al;
        __syncthreads();   // the image and the keys are rewritten by the next band
    }
}

// A step that allocates scratch: out of memory declines to the host builder (the error is
// cleared).  devbuild_gcb reports the same condition as an error; the two are not unified here.
#define B2_SCRATCH(x)                                    \
    do {                                                 \
        const hipError_t e_ = (x);                       \
        if (e_ == hipErrorOutOfMemory) {                 \
            (void)hipGetLastError();                     \
            return 1;                                    \
        }                                                \
        if (e_ != hipSuccess) {                          \
            err = e_;                                    \
            return -5;                                   \
        }                                                \
    } while (0)

// band2_build's checks of a geometry.
bool geom_ok(const B2Geom &g, bool cb) {
    if ((!cb && g.cpw != 2) || g.cpw < 1 || g.cpw > 8 || g.window > (1 << g.col_bits) ||
        (cb && g.window > (1 << g.cb_col)) ||
        g.block_rows > ((int64_t)1 << (32 - g.col_bits - kB2RankBits)) || g.block_rows > ((int64_t)1 << (31 - kCbIdBits)))
        return false;
    // this builder's own: the kernels' 16K-row blocks, a band's terms within the bitonic width
    return g.block_rows == 1 << kRowsLog2 && g.chunks() <= kMaxChunks && g.chunks() * 64 <= kSortN;
}

}  // namespace

int devbuild_band2(sm_matrix *m, int32_t kind, int32_t geo_opt, int32_t n_slabs, bool forced, int32_t slab0_permille,
                   Band2Host &meta, std::vector<float> &table, hipStream_t s, hipError_t &err) {
    err = hipSuccess;
    meta = Band2Host();
    table.clear();
    const int64_t n_rows = m->n_rows, n_cols = m->n_cols, nnz = m->nnz;
    if (band2_dev_knobs_set()) return 1;   // the development knobs are the host builder's
    // band2_build's limits
    if (n_rows <= 0 || n_cols <= 0 || n_slabs < 1 || n_cols >= ((int64_t)1 << 30) || nnz <= 0) return 1;
    const int32_t br = (int32_t)std::min<int64_t>((int64_t)1 << kRowsLog2, n_rows);
    const int64_t nblk = (n_rows + br - 1) / br;
    const B2Slabs sl = b2_slabs(n_cols, n_slabs, slab0_permille);
    const int64_t ntile = nblk * sl.ns;
    if (ntile >= ((int64_t)1 << 30)) return 1;
    DevScratch tp;
    // Codebook words where the values allow (first-occurrence ids, the host's order), else --
    // or for kind band2 -- 8-byte entries.
    uint8_t *ids = nullptr;
    bool cb = false;
    if (kind == kXbCband) {
        B2_SCRATCH(tp.alloc(&ids, nnz));
        const int rc = devbuild_codebook(m->d_val, nnz, table, ids, s, err);
        if (rc < 0) {
            if (err != hipErrorOutOfMemory) return rc;
            (void)hipGetLastError();
            err = hipSuccess;
            return 1;
        }
        cb = rc == 0;
        if (!cb) {
            tp.release(ids);
            ids = nullptr;
            table.clear();
        }
    }
    TileRun run;
    B2_SCRATCH(run_tile_front(tp, m, ids, kRowsLog2, nblk, sl, run, s));
    if (run.unsorted) return 1;   // a row's columns not strictly ascending (band2_build declines)
    if (ids) tp.release(ids);
    // cut: build_band2's sequence of geometries -- dma3 unless the wide one is asked for, wide
    // where the dma3 bands would be mostly padding
    int32_t *bstart = nullptr, *nb = nullptr, *tbs = nullptr;
    B2_SCRATCH(tp.alloc(&bstart, nnz));
    B2_SCRATCH(tp.alloc(&nb, ntile + 1));
    B2_SCRATCH(tp.alloc(&tbs, ntile + 1));
    BandScan scan;
    B2_SCRATCH(scan.prepare(tp, ntile));
    B2Geom g = geo_opt != 6 ? (cb ? kB2Dma3Cb : kB2Dma3B2) : kB2Wide;
    int32_t n_bands = 0;
    for (;;) {
        if (!geom_ok(g, cb)) return 1;
        DEV_TRY(hipMemsetAsync(nb + ntile, 0, 4, s));
        hipLaunchKernelGGL(b2_cut_kernel, dim3((unsigned)std::min<int64_t>(ntile, 1 << 16)), dim3(kNT), 0, s, ntile, sl,
                           run.tts, run.scol, run.srl, g, cb ? 1 : 0, bstart, nb);
        DEV_TRY(hipGetLastError());
        DEV_TRY(scan.run(nb, tbs, &n_bands, s));
        // band2_build: 32-bit entry offsets; build_band2: bands at least 70 % full unless forced
        // (every term lands in a band: real_terms = nnz)
        const bool ok = (int64_t)n_bands * 4096 < ((int64_t)1 << 31) &&
                        (forced || n_bands == 0 || (double)nnz >= 0.7 * (double)n_bands * g.chunks() * 64);
        if (ok) break;
        if (g.nch == 0) return 1;   // wide did not fit either
        g = kB2Wide;
    }
    if (n_bands <= 0) return 1;
    const int64_t band_words = (int64_t)(cb ? 64 : 128) * g.chunks();
    int32_t *gstart = nullptr, *gtile = nullptr;
    B2_SCRATCH(compact_bands(tp, run, tbs, bstart, n_bands, &gstart, &gtile, s));
    // the layout's arrays: build_band2's allocations
    Band2Dev &d = m->plan.b2;
    DEV_TRY(m->mem.alloc(&d.d_tile_band, ntile + 1));
    DEV_TRY(m->mem.alloc(&d.d_band_clo, std::max<int64_t>(1, n_bands)));
    DEV_TRY(m->mem.alloc(&d.d_ent, std::max<int64_t>(1, n_bands * band_words)));
    DEV_TRY(hipMemcpyAsync(d.d_tile_band, tbs, (size_t)(ntile + 1) * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(b2_emit_kernel, dim3((unsigned)std::min<int64_t>(n_bands, 1 << 20)), dim3(kET), 0, s,
                       (int64_t)n_bands, run.tts, gstart, gtile, run.scol, run.srl, run.sval, g, cb ? 1 : 0, d.d_band_clo,
                       d.d_ent, run.flag);
    DEV_TRY(hipGetLastError());
    int32_t fl = 0;
    DEV_TRY(hipMemcpyAsync(&fl, run.flag, 4, hipMemcpyDeviceToHost, s));
    DEV_TRY(hipStreamSynchronize(s));
    if (fl) {   // the emission's packing disagreed with the cut's: a builder bug, not a decline
        err = hipErrorUnknown;
        return -6;
    }
    meta.codebook = cb;
    meta.geom = g;
    meta.block_rows = br;
    meta.n_blocks = (int32_t)nblk;
    meta.n_slabs = (int32_t)sl.ns;
    meta.slab_cols = (int32_t)sl.sc;
    meta.slab0_cols = (int32_t)sl.s0;
    meta.n_bands = n_bands;
    meta.real_terms = nnz;
    return 0;
}

}  // namespace smamd
