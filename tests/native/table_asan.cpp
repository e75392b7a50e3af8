// Host-only check of the codebook forms built from GIVEN ids (sm_build_opts.table_updatable;
// band2.cpp, sell.cpp, ccsell.cpp, sweep.cpp), built with AddressSanitizer by
// tests/test_table_builder.py.  The table has two equal entries (ids 3 and 7) and an entry no
// term uses; for every builder:
//   * the words hold exactly the given ids: every real slot is a term (row, col) of the CSR with
//     that term's id (sell, ccsell, sweep), or the ids' histogram over the real slots is the
//     given one (cband, whose rows are relative to chunk headers) -- ids 3 and 7 stay apart;
//   * the layout built with (ids, table1[ids]) and the one built with (ids, table2[ids]) are the
//     same bytes: a new table changes the table alone.
// And the reason the given ids are needed: codebook_ids on the values collapses the equal entries.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "ccsell.h"
#include "sell.h"
#include "sweep.h"
#include "xband.h"

using namespace smamd;

namespace {

constexpr int kT = 12;   // table entries; 3 and 7 equal, 11 unused

struct Csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int32_t> rp, col;
    std::vector<uint8_t> ids;
    std::vector<float> val1, val2;
    std::map<std::pair<int32_t, int32_t>, uint8_t> id_of;   // (row, col) -> id
};

Csr random_csr(int64_t n_rows, int64_t n_cols, int per_row, unsigned seed) {
    std::mt19937 rng(seed);
    Csr m;
    m.n_rows = n_rows;
    m.n_cols = n_cols;
    m.rp.assign(1, 0);
    float t1[kT], t2[kT];
    for (int t = 0; t < kT; t++) {
        t1[t] = (float)(t + 1) * 0.25f;
        t2[t] = (float)(t + 1) * -1.5f;
    }
    t1[7] = t1[3];
    t2[7] = t2[3];
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c;
        const int len = r == n_rows / 2 ? (int)std::min<int64_t>(n_cols, 300) : per_row;   // one long row
        for (int j = 0; j < len; j++) c.push_back((int32_t)(rng() % (uint64_t)n_cols));
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        for (int32_t cc : c) {
            const uint8_t id = (uint8_t)(rng() % (kT - 1));   // id 11 is never used
            m.col.push_back(cc);
            m.ids.push_back(id);
            m.val1.push_back(t1[id]);
            m.val2.push_back(t2[id]);
            m.id_of[{(int32_t)r, cc}] = id;
        }
        m.rp.push_back((int32_t)m.col.size());
    }
    return m;
}

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// One real slot: must be a term of the CSR carrying that term's id.
struct SlotCheck {
    const Csr &m;
    const char *what;
    size_t seen = 0;
    int bad = 0;
    void slot(int64_t row, int64_t col, uint32_t id) {
        auto it = m.id_of.find({(int32_t)row, (int32_t)col});
        if (it == m.id_of.end() || it->second != id) {
            if (!bad++) printf("FAIL %s: slot (row %lld, col %lld) holds id %u\n", what, (long long)row, (long long)col, id);
        }
        seen++;
    }
    int done() {
        if (seen != m.col.size()) { printf("FAIL %s: %zu real slots, %zu terms\n", what, seen, m.col.size()); return 1; }
        return bad ? 1 : 0;
    }
};

int check_cband(const Csr &m, int slabs, B2Geom geom) {
    Band2Host h1, h2;
    if (!band2_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, m.n_cols, slabs, h1, m.ids.data(), geom) ||
        !band2_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, m.n_cols, slabs, h2, m.ids.data(), geom)) {
        printf("FAIL cband: build declined\n");
        return 1;
    }
    if (!h1.codebook || !same(h1.ent, h2.ent) || !same(h1.band_clo, h2.band_clo) ||
        !same(h1.tile_band_start, h2.tile_band_start) || h1.n_bands != h2.n_bands) {
        printf("FAIL cband: the words depend on the table\n");
        return 1;
    }
    std::vector<int64_t> want(256, 0), got(256, 0);
    for (uint8_t id : m.ids) want[id]++;
    for (uint32_t w : h1.ent) {
        const uint32_t id = ((w ^ geom.cb_dummy_word()) >> geom.cb_col) & 255u;
        if (id != kCbDummyId) got[id]++;
    }
    if (want != got || !got[3] || !got[7] || got[11]) {
        printf("FAIL cband: id histogram differs (3: %lld/%lld, 7: %lld/%lld)\n", (long long)got[3], (long long)want[3],
               (long long)got[7], (long long)want[7]);
        return 1;
    }
    return 0;
}

int check_sell(const Csr &m, int32_t max_len) {
    SellHost h1, h2;
    sell_build(m.rp.data(), m.col.data(), m.val1.data(), m.n_rows, max_len, h1, 0, 1, m.ids.data());
    sell_build(m.rp.data(), m.col.data(), m.val2.data(), m.n_rows, max_len, h2, 0, 1, m.ids.data());
    if (!h1.val.empty() || !same(h1.col, h2.col) || !same(h1.off, h2.off) || !same(h1.len, h2.len) ||
        !same(h1.row, h2.row) || !same(h1.row_len, h2.row_len)) {
        printf("FAIL sell: the words depend on the table\n");
        return 1;
    }
    // Whole rows: lane l of slice s holds row `row` in stored order.  Segments of the long row
    // (row <= -2) are consecutive pieces of it, in partial order.
    SlotCheck ck{m, "sell"};
    std::map<int32_t, int64_t> seg_next;   // long row -> next term
    std::vector<std::pair<int32_t, std::pair<int64_t, int>>> segs;   // (partial, (slice, lane))
    for (int64_t s = 0; s < h1.n_slices; s++)
        for (int l = 0; l < kSellLanes; l++) {
            const int32_t row = h1.row[(size_t)(s * kSellLanes + l)];
            const int32_t len = h1.row_len[(size_t)(s * kSellLanes + l)];
            if (row == -1) continue;
            if (row <= -2) { segs.push_back({-2 - row, {s, l}}); continue; }
            for (int32_t j = 0; j < len; j++) {
                const uint32_t w = (uint32_t)h1.col[(size_t)(h1.off[(size_t)s] + 64 * (int64_t)j + l)];
                ck.slot(row, w & 0xFFFFFFu, w >> 24);
            }
        }
    std::sort(segs.begin(), segs.end());
    for (size_t i = 0; i < h1.long_rows.size(); i++) {
        const int32_t row = h1.long_rows[i];
        for (const auto &sg : segs) {
            if (sg.first < h1.long_ptr[i] || sg.first >= h1.long_ptr[i + 1]) continue;
            const int64_t s = sg.second.first;
            const int l = sg.second.second;
            const int32_t len = h1.row_len[(size_t)(s * kSellLanes + l)];
            for (int32_t j = 0; j < len; j++) {
                const uint32_t w = (uint32_t)h1.col[(size_t)(h1.off[(size_t)s] + 64 * (int64_t)j + l)];
                ck.slot(row, w & 0xFFFFFFu, w >> 24);
            }
        }
    }
    return ck.done();
}

int check_ccsell(const Csr &m, int32_t chunk_log2) {
    CcsellHost h1, h2;
    if (!ccsell_build(m.rp.data(), m.col.data(), m.val1.data(), m.ids.data(), m.n_rows, m.n_cols, chunk_log2, h1) ||
        !ccsell_build(m.rp.data(), m.col.data(), m.val2.data(), m.ids.data(), m.n_rows, m.n_cols, chunk_log2, h2)) {
        printf("FAIL ccsell: build declined\n");
        return 1;
    }
    if (!h1.val.empty() || !same(h1.word, h2.word) || !same(h1.off, h2.off) || !same(h1.len, h2.len) ||
        !same(h1.row, h2.row) || !same(h1.row_len, h2.row_len)) {
        printf("FAIL ccsell: the words depend on the table\n");
        return 1;
    }
    SlotCheck ck{m, "ccsell"};
    for (int32_t c = 0; c < h1.n_chunks; c++)
        for (int64_t s = h1.chunk_slice[(size_t)c]; s < h1.chunk_slice[(size_t)c + 1]; s++)
            for (int l = 0; l < kSellLanes; l++) {
                const int32_t rw = h1.row[(size_t)(s * kSellLanes + l)];
                if (rw == -1) continue;
                const int32_t row = (int32_t)((uint32_t)rw & ~kCcFirst);
                const int32_t len = h1.row_len[(size_t)(s * kSellLanes + l)];
                for (int32_t j = 0; j < len; j++) {
                    const uint32_t w = h1.word[(size_t)(h1.off[(size_t)s] + 64 * (int64_t)j + l)];
                    ck.slot(row, ((int64_t)c << chunk_log2) + (w & ((1u << chunk_log2) - 1u)), w >> chunk_log2);
                }
            }
    return ck.done();
}

int check_sweep(const Csr &m) {
    SweepHost h1, h2;
    if (!sweep_build(m.rp.data(), m.col.data(), m.ids.data(), m.n_rows, h1) ||
        !sweep_build(m.rp.data(), m.col.data(), m.ids.data(), m.n_rows, h2)) {
        printf("FAIL sweep: build declined\n");
        return 1;
    }
    if (!same(h1.ent, h2.ent) || !same(h1.block_chunk, h2.block_chunk)) { printf("FAIL sweep: not deterministic\n"); return 1; }
    SlotCheck ck{m, "sweep"};
    for (int64_t b = 0; b < h1.n_blocks; b++)
        for (int64_t c = h1.block_chunk[(size_t)b]; c < h1.block_chunk[(size_t)b + 1]; c++)
            for (int l = 0; l < 64; l++) {
                const uint32_t col = h1.ent[(size_t)(2 * (64 * c + l))], meta = h1.ent[(size_t)(2 * (64 * c + l) + 1)];
                const uint32_t id = (meta >> 16) & 255u;
                if (id == kSwDummyId) continue;
                ck.slot(b * kSwRows + (meta & 0xFFFu), col, id);
            }
    return ck.done();
}

}  // namespace

int main() {
    int fails = 0;
    const Csr small = random_csr(700, 1000, 5, 1), wide = random_csr(3000, 70001, 20, 2);
    for (const Csr *m : {&small, &wide}) {
        // derived from the values, the codebook merges the equal entries: ids of its own
        std::vector<float> table;
        std::vector<uint8_t> ids;
        if (!codebook_ids(m->val1.data(), (int64_t)m->val1.size(), table, ids) || table.size() != kT - 2) {
            printf("FAIL: derived codebook has %zu entries, expected %d\n", table.size(), kT - 2);
            fails++;
        }
        for (int slabs : {1, 3})
            for (const B2Geom &g : {kB2Wide, kB2Dma3Cb}) fails += check_cband(*m, slabs, g);
        fails += check_sell(*m, 2048);
        fails += check_sell(*m, 64);   // the 300-term row cut in segments
        fails += check_ccsell(*m, 8);
        fails += check_ccsell(*m, 20);
        fails += check_sweep(*m);
    }
    if (fails) {
        printf("table_asan: %d failures\n", fails);
        return 1;
    }
    printf("table_asan: ok\n");
    return 0;
}
