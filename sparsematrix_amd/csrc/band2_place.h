// band2_place.h -- the placement heuristics of the balanced-band layout (xband.h Band2Host), one
// source for the host builder (band2.cpp) and the device builder (builddev_band2.hip): the "a new
// chunk opens" rule, the cross-chunk balance of a band's single terms, and a chunk's lane
// placement with its word encoders.  Integer-only, deterministic and order-sensitive: plain
// arrays, no allocation, so the same code runs in a kernel.  A band's segments are one array in
// chunk order; chunk c holds segs[cstart[c] .. cstart[c + 1]), at most 64 of them.
#pragma once

#include <cstdint>

#include "xband.h"

#ifdef __HIP__
#define SM_B2_HD __host__ __device__
#else
#define SM_B2_HD
#endif

namespace smamd {

// A row's run of terms inside one chunk: row in block, first term index, count.  The terms are
// col[s .. s + n) (val / ids alike): CSR indices on the host, indices into the band's staged
// copy on the device.
struct B2Seg {
    int32_t rl, s, n;
};

// Chunk capacity, longest segment and row span of one chunk.
struct B2Pack {
    int cap;
    int32_t max_seg, span;
};
SM_B2_HD inline B2Pack b2_pack(bool cb, const B2Geom &geom) {
    return B2Pack{cb ? kCbChunkTerms : 64, cb ? kCbChunkTerms : (int32_t)kB2DummyRank - 1,
                  cb ? geom.cb_row_span() : INT32_MAX};
}

// The column slabs of a band2 layout: whole 256-column pieces; slab 0 may be narrower
// (slab0_permille of an even share), the others split the rest evenly.  Slab s = [lo(s), lo(s + 1)).
struct B2Slabs {
    int64_t n_cols, sc, ns, s0;   // columns per slab s >= 1, slabs, columns of slab 0
    SM_B2_HD int64_t lo(int64_t s) const {
        if (s == 0) return 0;
        const int64_t v = s0 + (s - 1) * sc;
        return v < n_cols ? v : n_cols;
    }
};
inline B2Slabs b2_slabs(int64_t n_cols, int32_t n_slabs, int32_t slab0_permille) {
    int64_t sc = ((n_cols + n_slabs - 1) / n_slabs + 255) & ~(int64_t)255;
    int64_t ns = (n_cols + sc - 1) / sc;
    int64_t s0 = sc;
    if (ns > 1 && slab0_permille > 0 && slab0_permille < 1000) {
        s0 = (sc * slab0_permille / 1000 + 255) & ~(int64_t)255;
        if (s0 < 256) s0 = 256;
        if (s0 < sc) {
            sc = ((n_cols - s0 + ns - 2) / (ns - 1) + 255) & ~(int64_t)255;
            ns = 1 + (n_cols - s0 + sc - 1) / sc;
        } else {
            s0 = sc;
        }
    }
    return B2Slabs{n_cols, sc, ns, s0};
}

// A new chunk opens when the segment does not fit the current one (terms or rows).
SM_B2_HD inline bool b2_opens(const B2Pack &p, int fill, int32_t base, int32_t rl, int32_t n) {
    return fill + n > p.cap || rl - base >= p.span;
}

SM_B2_HD inline int b2_min(int a, int b) { return a < b ? a : b; }
SM_B2_HD inline int b2_max(int a, int b) { return a > b ? a : b; }

// Lanes inside a chunk: segments of 2+ terms take consecutive lanes first (the
// kernel passes a running sum up the lanes), then the single terms go to the two
// half-waves so that each half's LDS reads spread over the 32 banks: a ds_read_b32
// is served per 32-lane half, one LDS cycle per distinct address on its busiest bank,
// and every lane reads x[column - clo] (bank = column - clo mod 32) and the
// accumulator of its row (bank = row mod 32).  Each single goes to the half where its
// two banks are least used so far (ties: the emptier half), singles with the most
// contended banks first; lane order inside a half does not matter.  Which rows share
// a chunk and the per-row term order are unchanged (only lanes move).  cband
// (ids != nullptr): lane 0 is the header (the chunk's base row), terms take lanes
// 1..63 and carry their id, row - base and a continuation flag instead of value bits
// and rank.  band_term (8-byte entries, may be null): the band's slot -> term map.
// segs: chunk c's nseg (<= 64) segments in row order.  tab4_off: development A/B (host only).
SM_B2_HD inline void b2_emit_chunk(uint32_t *band_ent, int32_t *band_term, int c, const B2Seg *segs, int nseg,
                                   const int32_t *col, const float *val, const uint8_t *ids, int32_t clo_al,
                                   const B2Geom &geom, bool tab4_off = false) {
    bool used[64] = {false};
    const int cpw = ids != nullptr ? geom.cpw : 2;
    const int wave = c / cpw, k = c % cpw;
    const bool cb = ids != nullptr;
    const uint32_t cb_colmask = (1u << geom.cb_col) - 1u, cb_dummy = geom.cb_dummy_word();
    const int cb_off_shift = geom.cb_off_shift();
    const bool tab_banks = cb && geom.tab_copies == 1;   // one table copy: bank = id mod 32
    // Four table copies (dma3): lane l reads copy l mod 4, bank = 4 (id mod 8) + l mod 4 --
    // the lane's class (l mod 4) matters, so singles are placed by (half, class).
    const bool tab4 = cb && geom.tab_copies == 4 && !tab4_off;
    auto tbank = [&](uint32_t id, int lane) -> int {
        return tab_banks ? (int)(id & 31) : tab4 ? (int)((4 * (id & 7) + (uint32_t)(lane & 3)) & 31) : 0;
    };
    const int32_t base = nseg == 0 ? 0 : segs[0].rl;   // segments come in row order
    int next = 0;
    // Bank use per half: x reads (column bank), accumulator reads (row bank) and, with
    // one table copy, the table reads (id bank).
    uint8_t xb[2][32] = {}, yb[2][32] = {}, tb[2][32] = {};
    // A segment's lanes read one accumulator (a broadcast): its row counts once per half.
    auto note = [&](int lane, uint32_t cbits, int32_t rl, bool same_row_before, uint32_t id) {
        const int h = lane >> 5;
        xb[h][cbits & 31]++;
        if (!(same_row_before && ((lane - 1) >> 5) == h)) yb[h][rl & 31]++;
        tb[h][tbank(id, lane)]++;
    };
    if (cb) {
        const uint32_t h = ((uint32_t)base & cb_colmask) | cb_dummy |
                           ((((uint32_t)base >> geom.cb_col) & geom.cb_off_mask()) << cb_off_shift);
        band_ent[(size_t)(wave * 64) * cpw + k] = h ^ cb_dummy;
        used[0] = true;
        next = 1;
        note(0, h & cb_colmask, base + (int32_t)((h >> cb_off_shift) & geom.cb_off_mask()), false, kCbDummyId);
    }
    auto put = [&](const B2Seg &g, int32_t j, int lane) {
        const uint32_t cbits = (uint32_t)(col[g.s + j] - clo_al);
        if (cb) {
            const uint32_t w = cbits | ((uint32_t)ids[g.s + j] << geom.cb_col) |
                               ((uint32_t)(g.rl - base) << cb_off_shift) | ((j > 0 ? 1u : 0u) << kCbContBit);
            band_ent[(size_t)(wave * 64 + lane) * cpw + k] = w ^ cb_dummy;
        } else {
            uint32_t *e = band_ent + ((size_t)(wave * 64 + lane)) * 4;
            e[k] = (cbits | ((uint32_t)j << geom.col_bits) | ((uint32_t)g.rl << (geom.col_bits + kB2RankBits))) ^
                   geom.dummy_word();
            float v = val[g.s + j];
            uint32_t vb;
            __builtin_memcpy(&vb, &v, 4);
            e[2 + k] = vb;
            if (band_term) band_term[(size_t)(wave * 64 + lane) * 2 + k] = g.s + j;
        }
        used[lane] = true;
        note(lane, cbits, g.rl, j > 0, cb ? ids[g.s + j] : 0u);
    };
    for (int q = 0; q < nseg; q++)
        if (segs[q].n > 1)
            for (int32_t j = 0; j < segs[q].n; j++) put(segs[q], j, next++);
    // Singles: greedy, most contended banks first (pairwise swaps afterwards measured
    // 2.65 / 2.44 vs 2.70 / 2.48 cycles per half-wave read, tools/band2_banks.cpp: not kept).
    // Fixed arrays (a chunk holds <= 64 segments): no allocation per chunk.
    const B2Seg *single[64];
    int ns = 0;
    for (int q = 0; q < nseg; q++)
        if (segs[q].n == 1) single[ns++] = &segs[q];
    if (ns == 0) return;
    uint8_t xcnt[32] = {}, ycnt[32] = {}, tcnt[32] = {};
    uint8_t sx[64], sy[64], st[64], half[64];
    for (int i = 0; i < ns; i++) {
        sx[i] = (uint8_t)((col[single[i]->s] - clo_al) & 31);
        sy[i] = (uint8_t)(single[i]->rl & 31);
        st[i] = tab_banks ? (uint8_t)(ids[single[i]->s] & 31) : 0;
        xcnt[sx[i]]++;
        ycnt[sy[i]]++;
        tcnt[st[i]]++;
    }
    // Most contended first, ties in segment order: a stable counting sort on the weight.
    int order[64];
    {
        int w[64], cnt[3 * 64 + 2] = {};
        int wmax = 0;
        for (int i = 0; i < ns; i++) {
            w[i] = xcnt[sx[i]] + ycnt[sy[i]] + (tab_banks ? tcnt[st[i]] : 0);
            cnt[w[i]]++;
            wmax = b2_max(wmax, w[i]);
        }
        int at = 0;
        for (int v = wmax; v >= 0; v--) {   // start offsets, heaviest first
            const int n = cnt[v];
            cnt[v] = at;
            at += n;
        }
        for (int i = 0; i < ns; i++) order[cnt[w[i]]++] = i;
    }
    int free_in[2] = {0, 0};
    for (int l = 0; l < 64; l++)
        if (!used[l]) free_in[l >> 5]++;
    if (tab4) {
        // (half, lane class) per single: x and accumulator banks by half as below, the
        // table bank by half and class; then a free lane of that class in that half.
        int free_hc[2][4] = {};
        for (int l = 0; l < 64; l++)
            if (!used[l]) free_hc[l >> 5][l & 3]++;
        uint8_t cls[64];
        for (int oi = 0; oi < ns; oi++) {
            const int i = order[oi];
            const uint32_t id = ids[single[i]->s];
            int best = -1, bcls = 0, bcost = 1 << 30;
            for (int h = 0; h < 2; h++)
                for (int q = 0; q < 4; q++) {
                    if (free_hc[h][q] == 0) continue;
                    const int a = xb[h][sx[i]] + 1, b = yb[h][sy[i]] + 1;
                    const int t = tb[h][tbank(id, q)] + 1;
                    const int cost = 64 * (a * a + b * b + t * t) - free_hc[h][q];
                    if (cost < bcost) { bcost = cost; best = h; bcls = q; }
                }
            half[i] = (uint8_t)best;
            cls[i] = (uint8_t)bcls;
            free_hc[best][bcls]--;
            xb[best][sx[i]]++;
            yb[best][sy[i]]++;
            tb[best][tbank(id, bcls)]++;
        }
        for (int i = 0; i < ns; i++) {
            int lane = 32 * half[i] + cls[i];
            while (used[lane]) lane += 4;   // a free lane of the class exists (counted above)
            put(*single[i], 0, lane);
        }
        return;
    }
    for (int oi = 0; oi < ns; oi++) {
        const int i = order[oi];
        int best = -1, bcost = 1 << 30;
        for (int h = 0; h < 2; h++) {
            if (free_in[h] == 0) continue;
            const int a = xb[h][sx[i]] + 1, b = yb[h][sy[i]] + 1;
            const int t = tab_banks ? tb[h][st[i]] + 1 : 0;
            const int cost = 64 * (a * a + b * b + t * t) - free_in[h];
            if (cost < bcost) { bcost = cost; best = h; }
        }
        half[i] = (uint8_t)best;
        free_in[best]--;
        xb[best][sx[i]]++;
        yb[best][sy[i]]++;
        tb[best][st[i]]++;
    }
    int lane_next[2] = {31, 63};
    for (int i = 0; i < ns; i++) {
        const int h = half[i];
        int &lane = lane_next[h];
        while (used[lane]) lane--;
        put(*single[i], 0, lane);
    }
}

// Bank counts and the two smallest / largest rows of one chunk (b2_balance_chunks).
struct B2ChunkStats {
    uint8_t cx[32], cy[32];
    int32_t mn, mn2, mx, mx2;
};
SM_B2_HD inline void b2_chunk_stats(B2ChunkStats &h, const B2Seg *segs, int nseg, const int32_t *col,
                                    int32_t clo_al) {
    for (int i = 0; i < 32; i++) h.cx[i] = h.cy[i] = 0;
    h.mn = h.mn2 = INT32_MAX;
    h.mx = h.mx2 = INT32_MIN;
    for (int q = 0; q < nseg; q++) {
        const B2Seg &g = segs[q];
        for (int32_t j = 0; j < g.n; j++) h.cx[(col[g.s + j] - clo_al) & 31]++;
        h.cy[g.rl & 31]++;
        if (g.rl < h.mn) { h.mn2 = h.mn; h.mn = g.rl; } else if (g.rl < h.mn2) h.mn2 = g.rl;
        if (g.rl > h.mx) { h.mx2 = h.mx; h.mx = g.rl; } else if (g.rl > h.mx2) h.mx2 = g.rl;
    }
}

// The rows a chunk whose other rows span [mn, mx] (none: mn = INT32_MAX) can take within `span`.
SM_B2_HD inline int32_t b2_win_lo(int32_t mn, int32_t mx, int32_t span) {
    if (mn == INT32_MAX) return INT32_MIN;
    const int64_t v = (int64_t)mx - span + 1;
    return (int32_t)(v < INT32_MIN ? (int64_t)INT32_MIN : v);
}
SM_B2_HD inline int32_t b2_win_hi(int32_t mn, int32_t mx, int32_t span) {
    if (mn == INT32_MAX) return INT32_MAX;
    const int64_t v = (int64_t)mn + span - 1;
    return (int32_t)(v > INT32_MAX ? (int64_t)INT32_MAX : v);
}

// Cross-chunk balance (codebook bands): a band's chunks are cut in row order, so each single
// term could also sit in a neighbouring chunk whose rows stay within the row span.  Swapping
// singles between neighbours so each chunk's x banks (column mod 32) and accumulator banks
// (row mod 32) repeat less gives b2_emit_chunk's half / lane-class placement a better start:
// the per-half read costs it reaches fall with the chunk-level sums of squared bank counts.
// Rows move between chunks only (each row is still one segment of one chunk), so the sums
// are unchanged.  Singles whose banks repeat at least `hot` times are the candidates.
// Chunk sizes (cstart) do not change; each chunk ends sorted by row (rows are distinct).
SM_B2_HD inline void b2_balance_chunks(B2Seg *segs, const int32_t *cstart, int nc, const int32_t *col,
                                       int32_t clo_al, int32_t span) {
    constexpr int hot = 3;
    // Per iteration, b's singles are tabulated once (structure of arrays: index, row, banks,
    // b's span without it, the a/b bank-count differences of its banks); for every hot single
    // of a, one pass scores them all (ineligible: INT32_MAX) and the first least score wins:
    // the first (i, j) of least d < 0.
    // Row windows: a chunk whose other rows span [mn, mx] (empty: mn = INT32_MAX) takes a row r
    // iff max(mx, r) - min(mn, r) < span, i.e. r in [mx - span + 1, mn + span - 1] when mx - mn
    // < span (always: a subset of a chunk's rows), any r when empty.
    // (64-bit: band2's span is INT32_MAX, no row limit -- the window then clamps to the int32 range)
    auto win_lo = [&](int32_t mn, int32_t mx) { return b2_win_lo(mn, mx, span); };
    auto win_hi = [&](int32_t mn, int32_t mx) { return b2_win_hi(mn, mx, span); };
    B2ChunkStats A, B;
    int32_t cj[64], crl[64], clo[64], chi[64], cxt[64], cyt[64], cpx[64], cpy[64], dv[64];
    for (int a = 0; a + 1 < nc; a++) {
        const int b = a + 1;
        B2Seg *sa = segs + cstart[a], *sb = segs + cstart[b];
        const int na = cstart[a + 1] - cstart[a], nb = cstart[b + 1] - cstart[b];
        b2_chunk_stats(A, sa, na, col, clo_al);
        b2_chunk_stats(B, sb, nb, col, clo_al);
        for (int it = 0; it < 16; it++) {
            int nt = 0;
            for (int j = 0; j < nb; j++) {
                const B2Seg &t = sb[j];
                if (t.n != 1) continue;
                const int xt = (col[t.s] - clo_al) & 31, yt = t.rl & 31;
                const int32_t bmn = t.rl == B.mn ? B.mn2 : B.mn, bmx = t.rl == B.mx ? B.mx2 : B.mx;
                cj[nt] = j;
                crl[nt] = t.rl;
                clo[nt] = win_lo(bmn, bmx);
                chi[nt] = win_hi(bmn, bmx);
                if (bmn != INT32_MAX && bmx - bmn >= span) clo[nt] = INT32_MAX;   // (never: see above)
                cxt[nt] = xt;
                cyt[nt] = yt;
                cpx[nt] = A.cx[xt] - B.cx[xt];
                cpy[nt] = A.cy[yt] - B.cy[yt];
                nt++;
            }
            int minpx = INT32_MAX, minpy = INT32_MAX;   // lower bound of any single's best d
            for (int k = 0; k < nt; k++) {
                minpx = b2_min(minpx, cpx[k]);
                minpy = b2_min(minpy, cpy[k]);
            }
            int best_i = -1, best_j = -1, best = 0;
            for (int i = 0; i < na; i++) {
                const B2Seg &s_ = sa[i];
                if (s_.n != 1) continue;
                const int xs = (col[s_.s] - clo_al) & 31, ys = s_.rl & 31;
                if (A.cx[xs] < hot && A.cy[ys] < hot) continue;
                const int32_t amn = s_.rl == A.mn ? A.mn2 : A.mn, amx = s_.rl == A.mx ? A.mx2 : A.mx;
                if (amn != INT32_MAX && amx - amn >= span) continue;   // (never: see above)
                const int32_t alo = win_lo(amn, amx), ahi = win_hi(amn, amx), srl = s_.rl;
                // d = 2 (A.cx[xt] - A.cx[xs] + 1) + 2 (B.cx[xs] - B.cx[xt] + 1) if xs != xt, + the same in y
                const int qx = B.cx[xs] - A.cx[xs] + 2, qy = B.cy[ys] - A.cy[ys] + 2;
                if (nt == 0 || 2 * b2_min(0, minpx + qx) + 2 * b2_min(0, minpy + qy) >= best) continue;
                for (int k = 0; k < nt; k++) {   // branch-free: vectorises
                    const int d = 2 * (cpx[k] + qx) * (int)(xs != cxt[k]) + 2 * (cpy[k] + qy) * (int)(ys != cyt[k]);
                    const int ok = (int)(crl[k] >= alo) & (int)(crl[k] <= ahi) & (int)(srl >= clo[k]) & (int)(srl <= chi[k]);
                    dv[k] = ok ? d : INT32_MAX;
                }
                int mn = INT32_MAX;
                for (int k = 0; k < nt; k++) mn = b2_min(mn, dv[k]);
                if (mn >= best) continue;
                int k = 0;
                while (dv[k] != mn) k++;
                best = mn;
                best_i = i;
                best_j = cj[k];
            }
            if (best_i < 0) break;
            const B2Seg tmp = sa[best_i];
            sa[best_i] = sb[best_j];
            sb[best_j] = tmp;
            b2_chunk_stats(A, sa, na, col, clo_al);
            b2_chunk_stats(B, sb, nb, col, clo_al);
        }
    }
    for (int c = 0; c < nc; c++) {   // b2_emit_chunk: segments in row order, the first is the base
        B2Seg *s = segs + cstart[c];
        const int n = cstart[c + 1] - cstart[c];
        for (int i = 1; i < n; i++) {
            const B2Seg g = s[i];
            int j = i;
            for (; j > 0 && s[j - 1].rl > g.rl; j--) s[j] = s[j - 1];
            s[j] = g;
        }
    }
}

}  // namespace smamd
