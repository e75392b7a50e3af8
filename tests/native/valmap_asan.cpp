// Host-only check of the slot -> term maps the layout builders emit for updatable matrices
// (band2.cpp, xband.cpp, sell.cpp, ccsell.cpp, gcb.cpp; want_term), built with AddressSanitizer
// by tests/test_values_map_builder.py.  For every builder and shape:
//   * every term appears in exactly one slot;
//   * a slot's stored bits equal val[map[slot]];
//   * every -1 slot holds the builder's padding (zero bits);
//   * the core property of sm_set_values: writing val2[map[s]] into the layout built from val1
//     gives, byte for byte, the layout built from val2 (every array of the layout compared);
//   * without want_term the map is empty and the layout's bytes are the same.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ccsell.h"
#include "gcb.h"
#include "sell.h"
#include "xband.h"

using namespace smamd;

namespace {

struct Csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int32_t> rp, col;
    std::vector<float> val1, val2;   // any bit patterns: NaNs with payloads, -0.0, denormals, inf
};

float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

void fill_values(Csr &m, std::mt19937 &rng) {
    const size_t nnz = m.col.size();
    m.val1.resize(nnz);
    m.val2.resize(nnz);
    const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00001u,
                                0xffc12345u, 0x7f800001u, 0x00000001u, 0x807fffffu};
    for (size_t e = 0; e < nnz; e++) {
        m.val1[e] = from_bits((uint32_t)rng());
        m.val2[e] = e % 5 == 0 ? from_bits(special[(e / 5) % 9]) : from_bits((uint32_t)rng());
    }
}

// per_row distinct sorted columns per row (rows with r % empty_every == 0 stay empty when > 0).
Csr random_csr(int64_t n_rows, int64_t n_cols, int per_row, unsigned seed, int empty_every = 0) {
    std::mt19937 rng(seed);
    Csr m;
    m.n_rows = n_rows;
    m.n_cols = n_cols;
    m.rp.assign(1, 0);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c;
        if (!(empty_every > 0 && r % empty_every == 0))
            for (int j = 0; j < per_row; j++) c.push_back((int32_t)(rng() % (uint64_t)n_cols));
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        m.col.insert(m.col.end(), c.begin(), c.end());
        m.rp.push_back((int32_t)m.col.size());
    }
    fill_values(m, rng);
    return m;
}

// The same draw with every row's columns kept as repeats where they collide (`repeated`: ascending,
// not strictly) or reversed (`descending`): the builders' rule for a row's columns.
Csr messy_csr(int64_t n_rows, int64_t n_cols, int per_row, unsigned seed, bool descending) {
    std::mt19937 rng(seed);
    Csr m;
    m.n_rows = n_rows;
    m.n_cols = n_cols;
    m.rp.assign(1, 0);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c;
        for (int j = 0; j < per_row; j++) c.push_back((int32_t)(rng() % (uint64_t)n_cols));
        std::sort(c.begin(), c.end());
        if (descending) {
            c.erase(std::unique(c.begin(), c.end()), c.end());
            std::reverse(c.begin(), c.end());
        } else if (r % 3 == 0 && c.size() > 2) {
            c[1] = c[0];                        // a column twice ...
            c[c.size() - 2] = c[c.size() - 1];  // ... and the last one (three times when per_row == 3)
        }
        m.col.insert(m.col.end(), c.begin(), c.end());
        m.rp.push_back((int32_t)m.col.size());
    }
    fill_values(m, rng);
    return m;
}

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// `word(s)`: the 4-byte value word of slot s in the layout's own storage.
template <class W>
int check_map(const char *what, const Csr &m, const std::vector<int32_t> &map, size_t want_slots, W &&word) {
    const size_t nnz = m.col.size();
    if (map.size() != want_slots) { printf("FAIL %s: map has %zu slots, layout %zu\n", what, map.size(), want_slots); return 1; }
    std::vector<uint8_t> seen(nnz, 0);
    for (size_t s = 0; s < map.size(); s++) {
        const int32_t t = map[s];
        uint32_t got;
        memcpy(&got, word(s), 4);
        if (t < 0) {
            if (t != -1) { printf("FAIL %s: slot %zu map %d\n", what, s, t); return 1; }
            if (got != 0) { printf("FAIL %s: padding slot %zu holds %08x\n", what, s, got); return 1; }
            continue;
        }
        if ((size_t)t >= nnz || seen[(size_t)t]++) { printf("FAIL %s: term %d out of range or twice\n", what, t); return 1; }
        if (memcmp(&got, &m.val1[(size_t)t], 4) != 0) { printf("FAIL %s: slot %zu != val[%d]\n", what, s, t); return 1; }
    }
    for (size_t e = 0; e < nnz; e++)
        if (!seen[e]) { printf("FAIL %s: term %zu in no slot\n", what, e); return 1; }
    return 0;
}

template <class W>
void apply(const Csr &m, const std::vector<int32_t> &map, W &&word) {
    for (size_t s = 0; s < map.size(); s++)
        if (map[s] >= 0) memcpy(word(s), &m.val2[(size_t)map[s]], 4);
}

// ---- band2 -------------------------------------------------------------------------------
bool same_band2(const Band2Host &a, const Band2Host &b) {
    return a.n_bands == b.n_bands && a.n_blocks == b.n_blocks && a.n_slabs == b.n_slabs && a.slab_cols == b.slab_cols &&
           a.slab0_cols == b.slab0_cols && same(a.tile_band_start, b.tile_band_start) && same(a.band_clo, b.band_clo) &&
           same(a.ent, b.ent);
}

int check_band2(const Csr &m, int slabs, B2Geom geom) {
    Band2Host h1, h2, h0;
    const bool ok1 = band2_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, slabs, h1, nullptr, geom, 1000, true);
    const bool ok2 = band2_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, m.n_cols, slabs, h2, nullptr, geom, 1000, true);
    const bool ok0 = band2_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, slabs, h0, nullptr, geom, 1000);
    if (!ok1 || !ok2 || !ok0) { printf("FAIL band2: build declined\n"); return 1; }
    if (!h0.term.empty() || !same_band2(h0, h1)) { printf("FAIL band2: map without want_term, or other bytes with it\n"); return 1; }
    auto word = [&](size_t q) { return h1.ent.data() + (q / 2) * 4 + 2 + (q & 1); };
    if (check_map("band2", m, h1.term, h1.ent.size() / 2, word)) return 1;
    if (!same(h1.term, h2.term)) { printf("FAIL band2: the map depends on the values\n"); return 1; }
    apply(m, h1.term, word);
    if (!same_band2(h1, h2)) { printf("FAIL band2: updated layout != layout built from the new values\n"); return 1; }
    return 0;
}

// ---- xband (exact / blocked / gather) ----------------------------------------------------
bool same_xband(const XbandHost &a, const XbandHost &b) {
    return a.block_rows == b.block_rows && a.n_blocks == b.n_blocks && a.n_bands == b.n_bands && a.n_chunks == b.n_chunks &&
           same(a.chunk_start, b.chunk_start) && same(a.word, b.word) && same(a.val, b.val);
}

int check_xband(const Csr &m, XbBits bits, int waves, bool col_order) {
    XbandHost h1, h2, h0;
    const bool ok1 = xband_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, bits, waves, h1, col_order, 0, true);
    const bool ok2 = xband_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, m.n_cols, bits, waves, h2, col_order, 0, true);
    const bool ok0 = xband_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, bits, waves, h0, col_order);
    if (!ok1 || !ok2 || !ok0) { printf("FAIL xband: build declined\n"); return 1; }
    if (!h0.term.empty() || !same_xband(h0, h1)) { printf("FAIL xband: map without want_term, or other bytes with it\n"); return 1; }
    auto word = [&](size_t s) { return h1.val.data() + s; };
    if (check_map("xband", m, h1.term, h1.val.size(), word)) return 1;
    apply(m, h1.term, word);
    if (!same_xband(h1, h2)) { printf("FAIL xband: updated layout != layout built from the new values\n"); return 1; }
    return 0;
}

// ---- sell ----------------------------------------------------------------------------------
bool same_sell(const SellHost &a, const SellHost &b) {
    return a.n_slices == b.n_slices && a.padded == b.padded && same(a.off, b.off) && same(a.len, b.len) &&
           same(a.row, b.row) && same(a.row_len, b.row_len) && same(a.col, b.col) && same(a.val, b.val) &&
           same(a.long_rows, b.long_rows) && same(a.long_ptr, b.long_ptr);
}

int check_sell(const Csr &m, int32_t max_len, int64_t sigma, int streams) {
    SellHost h1, h2, h0;
    sell_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, max_len, h1, sigma, streams, nullptr, true);
    sell_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, max_len, h2, sigma, streams, nullptr, true);
    sell_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, max_len, h0, sigma, streams);
    if (!h0.term.empty() || !same_sell(h0, h1)) { printf("FAIL sell: map without want_term, or other bytes with it\n"); return 1; }
    auto word = [&](size_t s) { return h1.val.data() + s; };
    if (check_map("sell", m, h1.term, (size_t)h1.padded, word)) return 1;
    apply(m, h1.term, word);
    if (!same_sell(h1, h2)) { printf("FAIL sell: updated layout != layout built from the new values\n"); return 1; }
    // The codebook form holds ids, not values: no map even when asked.
    std::vector<uint8_t> ids(m.col.size(), 1);
    bool narrow = true;
    for (int32_t c : m.col) narrow = narrow && c < (1 << kSellCbColBits);
    if (narrow) {
        SellHost hc;
        sell_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, max_len, hc, sigma, streams, ids.data(), true);
        if (!hc.term.empty()) { printf("FAIL sell: a map in the codebook form\n"); return 1; }
    }
    return 0;
}

// ---- ccsell --------------------------------------------------------------------------------
bool same_ccsell(const CcsellHost &a, const CcsellHost &b) {
    return a.n_slices == b.n_slices && a.padded == b.padded && a.n_chunks == b.n_chunks && same(a.chunk_slice, b.chunk_slice) &&
           same(a.off, b.off) && same(a.len, b.len) && same(a.row, b.row) && same(a.row_len, b.row_len) &&
           same(a.word, b.word) && same(a.val, b.val);
}

int check_ccsell(const Csr &m, int chunk_log2, bool by_length) {
    CcsellHost h1, h2, h0;
    const bool ok1 = ccsell_build(m.rp.data(), m.col.data(), m.val1.data(), nullptr, m.n_rows, m.n_cols, chunk_log2, h1, by_length, true);
    const bool ok2 = ccsell_build(m.rp.data(), m.col.data(), m.val2.data(), nullptr, m.n_rows, m.n_cols, chunk_log2, h2, by_length, true);
    const bool ok0 = ccsell_build(m.rp.data(), m.col.data(), m.val1.data(), nullptr, m.n_rows, m.n_cols, chunk_log2, h0, by_length);
    if (!ok1 || !ok2 || !ok0) { printf("FAIL ccsell: build declined\n"); return 1; }
    if (!h0.term.empty() || !same_ccsell(h0, h1)) { printf("FAIL ccsell: map without want_term, or other bytes with it\n"); return 1; }
    auto word = [&](size_t s) { return h1.val.data() + s; };
    if (check_map("ccsell", m, h1.term, (size_t)h1.padded, word)) return 1;
    apply(m, h1.term, word);
    if (!same_ccsell(h1, h2)) { printf("FAIL ccsell: updated layout != layout built from the new values\n"); return 1; }
    return 0;
}

// ---- gcb -----------------------------------------------------------------------------------
bool same_gcb(const GcbHost &a, const GcbHost &b) {
    return a.n_bands == b.n_bands && a.n_blocks == b.n_blocks && a.n_slabs == b.n_slabs && a.slab_cols == b.slab_cols &&
           same(a.tile_band_start, b.tile_band_start) && same(a.band_clo, b.band_clo) && same(a.ent, b.ent);
}

int check_gcb(const Csr &m, int rows_log2, int slabs, int32_t window) {
    GcbHost h1, h2, h0;
    const bool ok1 = gcb_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, rows_log2, slabs, window, h1, true);
    const bool ok2 = gcb_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, m.n_cols, rows_log2, slabs, window, h2, true);
    const bool ok0 = gcb_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, rows_log2, slabs, window, h0);
    if (!ok1 || !ok2 || !ok0) { printf("FAIL gcb: build declined\n"); return 1; }
    if (!h0.term.empty() || !same_gcb(h0, h1)) { printf("FAIL gcb: map without want_term, or other bytes with it\n"); return 1; }
    auto word = [&](size_t q) { return h1.ent.data() + (q / 2) * 4 + 2 + (q & 1); };
    if (check_map("gcb", m, h1.term, h1.ent.size() / 2, word)) return 1;
    apply(m, h1.term, word);
    if (!same_gcb(h1, h2)) { printf("FAIL gcb: updated layout != layout built from the new values\n"); return 1; }
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    // band2: the wide and the dma3 geometry, one and several slabs; hub columns split by rows.
    for (int slabs : {1, 4}) {
        for (B2Geom g : {kB2Wide, kB2Dma3B2}) {
            bad += check_band2(random_csr(20011, 300001, 16, 1), slabs, g);
            bad += check_band2(random_csr(3001, 70001, 40, 2), slabs, g);
            bad += check_band2(random_csr(5000, 1000, 5, 4), slabs, g);
            bad += check_band2(random_csr(1, 50000, 30, 8), slabs, g);
        }
    }
    {
        std::mt19937 rng(11);
        Csr m;
        m.n_rows = 40000;
        m.n_cols = 20000;
        m.rp.assign(1, 0);
        for (int64_t r = 0; r < m.n_rows; r++) {
            std::vector<int32_t> c = {4097};
            if (r % 3 == 0) c.push_back(9000);
            for (int j = 0; j < 6; j++) c.push_back((int32_t)(rng() % m.n_cols));
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
            m.col.insert(m.col.end(), c.begin(), c.end());
            m.rp.push_back((int32_t)m.col.size());
        }
        fill_values(m, rng);
        bad += check_band2(m, 1, kB2Wide);
        bad += check_band2(m, 3, kB2Dma3B2);
    }
    // xband: the exact, blocked and gather kinds.
    {
        const XbBits exact = xb_bits(kXbExactBandLog2, kXbExactRowsLog2);
        const XbBits blocked = xb_bits(kXbBlockedBandLog2, kXbBlockedRowsLog2);
        const XbBits gather = xb_bits(kXbGatherBandLog2, kXbGatherRowsLog2);
        const struct { XbBits bits; int waves; bool col_order; } kinds[] = {
            {exact, kXbThreads / 64, false}, {blocked, kXbComputeWaves, false}, {gather, kXbThreads / 64, true}};
        for (const auto &k : kinds) {
            bad += check_xband(random_csr(9000, 70001, 40, 2), k.bits, k.waves, k.col_order);
            bad += check_xband(random_csr(4096, 32768, 7, 3), k.bits, k.waves, k.col_order);
            bad += check_xband(random_csr(5000, 1000, 5, 4), k.bits, k.waves, k.col_order);
            bad += check_xband(random_csr(5000, 40000, 8, 5), k.bits, k.waves, k.col_order);
        }
    }
    // sell: empty rows, rows cut into segments by a small max_len, windows and streams.
    for (int64_t n_rows : {1, 63, 64, 65, 1000, 70001}) {
        std::mt19937 rng(5 + (unsigned)n_rows);
        Csr m;
        m.n_rows = n_rows;
        m.n_cols = 100000;
        m.rp.assign(1, 0);
        for (int64_t r = 0; r < n_rows; r++) {
            int32_t n = r % 7 == 3 ? 0 : (int32_t)(rng() % 20);
            if (r == n_rows / 2) n = 1000;   // one long row
            for (int32_t j = 0; j < n; j++) m.col.push_back((int32_t)(rng() % 100000));
            m.rp.push_back((int32_t)m.col.size());
        }
        fill_values(m, rng);
        for (int32_t mx : {1, 16, 64, 2048}) {
            bad += check_sell(m, mx, 0, 1);
            bad += check_sell(m, mx, 1000, 8);
            bad += check_sell(m, mx, 64, 3);
        }
    }
    // ccsell: small chunks (many units per row), the default-sized one, row order.
    bad += check_ccsell(random_csr(9000, 70001, 40, 2, 11), 8, true);
    bad += check_ccsell(random_csr(5000, 300001, 40, 3, 11), 12, true);
    bad += check_ccsell(random_csr(3, 1000, 300, 4), 8, true);
    bad += check_ccsell(random_csr(20000, 1 << 20, 16, 5, 11), 20, true);
    bad += check_ccsell(random_csr(20000, 1 << 20, 16, 6, 11), 16, false);
    // gcb: 32K- and 16K-row tiles, slabs, narrow windows.
    bad += check_gcb(random_csr(20000, 3000001, 16, 1), 15, 1, 1 << 18);
    bad += check_gcb(random_csr(20000, 3000001, 16, 2), 14, 3, 1 << 18);
    bad += check_gcb(random_csr(9000, 70001, 40, 3), 14, 1, 4096);
    bad += check_gcb(random_csr(9000, 70001, 40, 4), 14, 2, 1 << 18);
    bad += check_gcb(random_csr(5000, 1000, 5, 5), 14, 2, 1 << 18);
    bad += check_gcb(random_csr(1, 50000, 300, 6), 14, 1, 1 << 18);
    // Rows that do not strictly ascend.  Repeated columns: the fixed band kinds and the sliced
    // ELL take them with a map that names every term once; band2, gcb and ccsell decline.  A
    // descending step: only the sliced ELL (stored order) is built.
    {
        const Csr rep = messy_csr(5000, 40000, 8, 21, false), desc = messy_csr(5000, 40000, 8, 22, true);
        const XbBits exact = xb_bits(kXbExactBandLog2, kXbExactRowsLog2);
        const XbBits blocked = xb_bits(kXbBlockedBandLog2, kXbBlockedRowsLog2);
        const struct { XbBits bits; int waves; bool col_order; } kinds[] = {
            {exact, kXbThreads / 64, false}, {blocked, kXbComputeWaves, false}, {blocked, kXbThreads / 64, true}};
        for (const auto &k : kinds) {
            bad += check_xband(rep, k.bits, k.waves, k.col_order);
            XbandHost xh;
            if (xband_build(desc.rp.data(), desc.col.data(), desc.val1.data(), desc.n_rows, desc.n_cols, k.bits, k.waves,
                            xh, k.col_order, 0, true)) {
                printf("FAIL xband: descending columns accepted\n");
                bad++;
            }
        }
        for (const Csr *m : {&rep, &desc}) {
            Band2Host b2;
            GcbHost gh;
            CcsellHost ch;
            if (band2_build(m->rp.data(), m->col.data(), m->val1.data(), m->n_rows, m->n_cols, 1, b2, nullptr, kB2Wide, 1000, true) ||
                gcb_build(m->rp.data(), m->col.data(), m->val1.data(), m->n_rows, m->n_cols, 14, 1, 1 << 18, gh, true) ||
                ccsell_build(m->rp.data(), m->col.data(), m->val1.data(), nullptr, m->n_rows, m->n_cols, 12, ch, true, true)) {
                printf("FAIL band2 / gcb / ccsell: columns not strictly ascending accepted\n");
                bad++;
            }
            bad += check_sell(*m, 16, 0, 1);
            bad += check_sell(*m, 2048, 1000, 8);
        }
    }
    printf(bad ? "valmap_asan: FAILED\n" : "valmap_asan: ok\n");
    return bad ? 1 : 0;
}
