// band2.cpp -- host-side builder of the balanced-band layout used by
// spmv_band2_kernel (kernels_band2.hip).  Layout: xband.h (Band2Host).
//
// Per tile (block b of rows, slab s of columns) the builder walks the slab's
// columns left to right and closes a band [clo, chi) as soon as either
//   * its window from clo rounded down to 4 columns would pass geom.window columns,
//   * its terms, packed row by row into 64-entry chunks without splitting a row's
//     segment (the row's run of terms inside the band), would need more than
//     kB2Chunks chunks, or
//   * a row would have more than 14 terms in it (the 4-bit rank field),
// so every band is one fixed-size slot of 32 chunks: the kernel's wave w applies
// chunks 2w and 2w+1 and loads them with one 16-byte load per lane.  Columns
// without terms never open a band.  Inside a band the terms are listed by row,
// each row's segment in ascending column order, so across the tile's bands (which
// ascend in column) every row's terms are added in the reference's order
// (sparse-matrix.cc:164-190, kernel.cc:780-796: per output, ascending column).
#include <algorithm>
#include <cstdlib>
#include <thread>

#include "band2_place.h"
#include "xband.h"

namespace smamd {

namespace {

struct TileOut {
    std::vector<int32_t> clo;
    std::vector<uint32_t> ent;
    std::vector<int32_t> term;   // want_term: 2 per lane entry (Band2Host::term)
    int64_t terms = 0;
    bool ok = true;
};

void build_tile(const int32_t *rp, const int32_t *col, const float *val, const uint8_t *ids,
                int64_t r0, int64_t r1, int64_t c0, int64_t c1, B2Geom geom, bool want_term, TileOut &out) {
#ifdef SM_DEV
    static const bool kBalance = !(getenv("SM_B2_BAL") && atoi(getenv("SM_B2_BAL")) == 0);   // A/B
#else
    constexpr bool kBalance = true;
#endif
    const int64_t nr = r1 - r0;
    const bool cb = ids != nullptr;
    // Chunk capacity, longest segment and row span of one chunk (band2_place.h).
    const B2Pack pack = b2_pack(cb, geom);
    const int cap = pack.cap;
    const int32_t max_seg = pack.max_seg, span = pack.span;
    const int nchunks = geom.chunks();   // band2's default: kB2Chunks (32)
    const size_t band_words = (size_t)(cb ? 64 : 128) * nchunks;
    auto opens = [&](int fill, int32_t base, const B2Seg &g) { return b2_opens(pack, fill, base, g.rl, g.n); };
#ifdef SM_DEV
    static const bool tab4_off = getenv("SM_B2_TAB4") && atoi(getenv("SM_B2_TAB4")) == 0;   // A/B
#else
    constexpr bool tab4_off = false;
#endif
    std::vector<int32_t> cur((size_t)nr), end((size_t)nr);
    std::vector<int32_t> hist((size_t)(c1 - c0) + 1, 0);
    for (int64_t r = r0; r < r1; r++) {
        const int32_t *a = col + rp[r], *z = col + rp[r + 1];
        cur[r - r0] = (int32_t)(std::lower_bound(a, z, (int32_t)c0) - col);
        end[r - r0] = (int32_t)(std::lower_bound(a, z, (int32_t)c1) - col);
        for (int32_t e = cur[r - r0]; e < end[r - r0]; e++) hist[(size_t)(col[e] - c0)]++;
    }
    // hist -> prefix counts H[i] = terms in columns [c0, c0 + i)
    std::vector<int64_t> H((size_t)(c1 - c0) + 1, 0);
    for (int64_t i = 0; i < c1 - c0; i++) H[(size_t)i + 1] = H[(size_t)i] + hist[(size_t)i];
    auto count = [&](int64_t a, int64_t b) { return H[(size_t)(b - c0)] - H[(size_t)(a - c0)]; };
    int64_t clo = c0;
    std::vector<B2Seg> segs;
    std::vector<int32_t> cstart((size_t)nchunks + 1);   // chunk c: segs[cstart[c] .. cstart[c + 1])
    while (clo < c1 && count(clo, c1) > 0) {
        while (hist[(size_t)(clo - c0)] == 0) clo++;   // no band starts on an empty column
        const int64_t clo_al = clo & ~(int64_t)3;
#ifdef SM_DEV_B2_WINDOW   // development A/B: narrower bands (fewer terms per band)
        const int64_t lim = std::min<int64_t>(c1, clo_al + std::min<int32_t>(geom.window, SM_DEV_B2_WINDOW));
#else
        const int64_t lim = std::min<int64_t>(c1, clo_al + geom.window);
#endif
        // Largest chi <= lim with at most 32 * 64 terms (binary search on H).
        int64_t lo = clo + 1, hi = lim;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (count(clo, mid) <= (int64_t)nchunks * 64) lo = mid; else hi = mid - 1;
        }
        int64_t chi = lo;
        // A single column whose terms in this block need more than kB2Chunks chunks (a
        // hub or dense column: > 2048 terms, or rows too far apart for one chunk's row
        // span) is split by rows over several one-column bands: a band takes the rows
        // that fill its 32 chunks, the next band the same column from the next row on.
        // Each row still has one term in that column, so every row's terms stay in
        // ascending column order across the bands.
        bool split = false;
        for (;;) {   // pack; shrink chi until the band fits
            segs.clear();
            bool retry = false;
            int chunks = 0, fill = cap;
            int32_t base = 0;
            const bool single = chi == clo + 1;
            split = false;
            for (int64_t r = 0; r < nr && !retry; r++) {
                const int32_t s = cur[(size_t)r];
                int32_t n = 0;
                while (s + n < end[(size_t)r] && col[s + n] < chi) n++;
                if (n == 0) continue;
                if (n > max_seg) {   // band2: ranks 0..13 + dummy 15; cband: one chunk
                    chi = col[s + max_seg];
                    retry = true;
                    break;
                }
                const B2Seg g{(int32_t)r, s, n};
                if (opens(fill, base, g)) {
                    if (single && chunks == nchunks) { split = true; break; }   // rest: next band
                    chunks++; fill = 0; base = g.rl;
                }
                fill += n;
                segs.push_back(g);
            }
            if (retry) continue;
            if (chunks > nchunks) {
                chi = clo + std::max<int64_t>(1, (chi - clo) * 31 / 32);
                continue;
            }
            break;
        }
        // Emit: segments into chunks in row order.
        const size_t base = out.ent.size();
        out.ent.resize(base + band_words, 0u);   // dummies: word 0 (= dummy ^ dummy), value 0
        const size_t tbase = out.term.size();
        if (want_term) out.term.resize(tbase + band_words / 2, -1);
        out.clo.push_back((int32_t)clo_al);
        int c = -1, fill = cap;
        int32_t cbase = 0;
        for (size_t q = 0; q < segs.size(); q++) {
            const B2Seg &g = segs[q];
            if (opens(fill, cbase, g)) { c++; fill = 0; cbase = g.rl; cstart[(size_t)c] = (int32_t)q; }
            fill += g.n;
            cur[(size_t)g.rl] += g.n;
            out.terms += g.n;
        }
        cstart[(size_t)c + 1] = (int32_t)segs.size();
        if (kBalance) b2_balance_chunks(segs.data(), cstart.data(), c + 1, col, (int32_t)clo_al, span);
        for (int k = 0; k <= c; k++)
            b2_emit_chunk(out.ent.data() + base, want_term ? out.term.data() + tbase : nullptr, k,
                          segs.data() + cstart[(size_t)k], cstart[(size_t)k + 1] - cstart[(size_t)k], col, val, ids,
                          (int32_t)clo_al, geom, tab4_off);
        if (!split) clo = chi;   // split: the column's remaining rows go to the next band
    }
    for (int64_t r = 0; r < nr; r++)
        if (cur[(size_t)r] != end[(size_t)r]) out.ok = false;   // unsorted columns
}

}  // namespace

bool band2_build(const int32_t *rp, const int32_t *col, const float *val, int64_t n_rows,
                 int64_t n_cols, int32_t n_slabs, Band2Host &out, const uint8_t *ids, B2Geom geom,
                 int32_t slab0_permille, bool want_term) {
    out = Band2Host();
    want_term = want_term && !ids;   // codebook words hold ids, not values
    out.codebook = ids != nullptr;
    out.geom = geom;
    if ((!ids && geom.cpw != 2) || geom.cpw < 1 || geom.cpw > 8 ||
        geom.window > (1 << geom.col_bits) || (ids && geom.window > (1 << geom.cb_col)) ||
        geom.block_rows > ((int64_t)1 << (32 - geom.col_bits - kB2RankBits)) ||
        geom.block_rows > ((int64_t)1 << (31 - kCbIdBits)))
        return false;
    const int64_t band_words = (int64_t)(ids ? 64 : 128) * geom.chunks();
    if (n_rows <= 0 || n_cols <= 0 || n_slabs < 1 || n_cols >= ((int64_t)1 << 30)) return false;   // x < 4 GiB: 32-bit buffer offsets
    for (int64_t r = 0; r < n_rows; r++)   // strictly ascending columns per row
        for (int32_t e = rp[r] + 1; e < rp[r + 1]; e++)
            if (col[e] <= col[e - 1]) return false;
    const int32_t br = (int32_t)std::min<int64_t>(geom.block_rows, n_rows);
    const int64_t nblk = (n_rows + br - 1) / br;
    // Slabs of whole 256-column pieces; slab 0 may be narrower (band2_place.h b2_slabs).
    const B2Slabs slabs = b2_slabs(n_cols, n_slabs, slab0_permille);
    const int64_t sc = slabs.sc, ns = slabs.ns, s0 = slabs.s0;
    auto slab_lo = [&](int64_t s) { return slabs.lo(s); };
    const int64_t ntile = nblk * ns;
    if (ntile >= ((int64_t)1 << 30)) return false;
    std::vector<TileOut> tiles((size_t)ntile);
    const int nthr = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; t++)
        th.emplace_back([&, t] {
            for (int64_t i = t; i < ntile; i += nthr) {
                const int64_t b = i / ns, s = i % ns;
                build_tile(rp, col, val, ids, b * br, std::min<int64_t>(n_rows, (b + 1) * br), slab_lo(s),
                           slab_lo(s + 1), geom, want_term, tiles[(size_t)i]);
            }
        });
    for (auto &x : th) x.join();
    out.block_rows = br;
    out.n_blocks = (int32_t)nblk;
    out.n_slabs = (int32_t)ns;
    out.slab_cols = (int32_t)sc;
    out.slab0_cols = (int32_t)s0;
    out.tile_band_start.resize((size_t)ntile + 1);
    int64_t nb = 0;
    for (int64_t i = 0; i < ntile; i++) {
        if (!tiles[(size_t)i].ok) return false;
        out.tile_band_start[(size_t)i] = (int32_t)nb;
        const int64_t k = (int64_t)tiles[(size_t)i].clo.size();
        out.max_bands_per_tile = std::max<int32_t>(out.max_bands_per_tile, (int32_t)k);
        nb += k;
        out.real_terms += tiles[(size_t)i].terms;
    }
    out.tile_band_start[(size_t)ntile] = (int32_t)nb;
    if (nb * 4096 >= ((int64_t)1 << 31)) return false;   // 32-bit entry offsets (x 4 bytes per dword)
    out.n_bands = nb;
    out.band_clo.reserve((size_t)nb);
    out.ent.reserve((size_t)(nb * band_words));
    for (auto &t : tiles) {
        out.band_clo.insert(out.band_clo.end(), t.clo.begin(), t.clo.end());
        out.ent.insert(out.ent.end(), t.ent.begin(), t.ent.end());
        out.term.insert(out.term.end(), t.term.begin(), t.term.end());
        std::vector<uint32_t>().swap(t.ent);
        std::vector<int32_t>().swap(t.term);
    }
    return true;
}

bool band2_dev_knobs_set() {
#ifdef SM_DEV_B2_WINDOW
    return true;
#elif defined(SM_DEV)
    return getenv("SM_B2_BAL") != nullptr || getenv("SM_B2_TAB4") != nullptr;
#else
    return false;
#endif
}

bool codebook_ids(const float *val, int64_t n, std::vector<float> &table, std::vector<uint8_t> &ids) {
    // Open-addressing set of at most 255 bit patterns (512 slots).
    constexpr uint32_t kSlots = 512;
    uint32_t key[kSlots];
    int16_t id[kSlots];
    for (uint32_t i = 0; i < kSlots; i++) id[i] = -1;
    table.clear();
    ids.assign((size_t)n, 0);
    for (int64_t e = 0; e < n; e++) {
        uint32_t b;
        __builtin_memcpy(&b, &val[e], 4);
        uint32_t h = (b * 2654435761u) >> 23;   // 9 bits
        while (id[h] >= 0 && key[h] != b) h = (h + 1) & (kSlots - 1);
        if (id[h] < 0) {
            if (table.size() >= kCbDummyId) return false;
            key[h] = b;
            id[h] = (int16_t)table.size();
            table.push_back(val[e]);
        }
        ids[(size_t)e] = (uint8_t)id[h];
    }
    return true;
}

}  // namespace smamd
