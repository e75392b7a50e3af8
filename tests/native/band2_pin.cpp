// Pins the bytes of the balanced-band builder (sparsematrix_amd/csrc/band2.cpp): for a fixed
// list of small matrices from a hard-coded integer generator, one 64-bit FNV-1a per case over
// block_rows, n_blocks, n_slabs, slab_cols, slab0_cols, geom.window, tile_band_start, band_clo,
// ent and (codebook words) the table.  tests/test_band2_pin.py builds this with
// AddressSanitizer and compares the output with the fixture under tests/golden/, recorded from
// the builder as it stood before its placement heuristics moved to band2_place.h.  The cases
// are those of tests/test_gpu_devbuild_band2.py at sizes that run in a second or two: both
// encodings, the dma3 and wide geometries, one / three / sixteen slabs.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "xband.h"

using namespace smamd;

namespace {

struct Rng {   // 64-bit LCG (Knuth's MMIX constants), the high 32 bits
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 32);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

struct Csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int32_t> rp{0}, col;
    void row(std::vector<int32_t> c) {
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        col.insert(col.end(), c.begin(), c.end());
        rp.push_back((int32_t)col.size());
        n_rows++;
    }
};

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void *p, size_t n) {
        const uint8_t *b = static_cast<const uint8_t *>(p);
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    }
    template <class T>
    void vec(const std::vector<T> &v) { if (!v.empty()) add(v.data(), v.size() * sizeof(T)); }
};

bool first = true;

// values: 0 = many distinct fp32 values, else that many distinct values
void pin(const std::string &name, const Csr &m, int values, bool cband, const B2Geom &geom, int slabs,
         int permille = 1000) {
    Rng rng(12345);
    std::vector<float> val(m.col.size());
    for (float &v : val) {
        if (values == 0) v = (float)(int32_t)(rng.below(200001)) * 0.25f - 20000.0f;
        else v = (float)(int32_t)rng.below((uint32_t)values) * 0.375f - 40.0f;
    }
    // every one of `values` patterns present (the codebook edges)
    for (int i = 0; i < values && i < (int)val.size(); i++) val[(size_t)i] = (float)i * 0.375f - 40.0f;
    std::vector<float> table;
    std::vector<uint8_t> ids;
    const bool cb = cband && codebook_ids(val.data(), (int64_t)val.size(), table, ids);
    Band2Host h;
    const bool ok = band2_build(m.rp.data(), m.col.data(), val.data(), m.n_rows, m.n_cols, slabs, h,
                                cb ? ids.data() : nullptr, geom, permille);
    Fnv f;
    if (ok) {
        const int32_t g[6] = {h.block_rows, h.n_blocks, h.n_slabs, h.slab_cols, h.slab0_cols, h.geom.window};
        f.add(g, sizeof(g));
        f.vec(h.tile_band_start);
        f.vec(h.band_clo);
        f.vec(h.ent);
        if (cb) f.vec(table);
    }
    printf("%s  \"%s\": {\"built\": %d, \"codebook\": %d, \"bands\": %lld, \"fnv\": \"%016llx\"}", first ? "" : ",\n",
           name.c_str(), ok ? 1 : 0, cb ? 1 : 0, (long long)(ok ? h.n_bands : 0), (unsigned long long)(ok ? f.h : 0));
    first = false;
}

Csr uniform(int64_t n_rows, int64_t n_cols, int per_row, uint64_t seed) {
    Csr m;
    m.n_cols = n_cols;
    Rng rng(seed);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c((size_t)per_row);
        for (auto &v : c) v = (int32_t)rng.below((uint32_t)n_cols);
        m.row(c);
    }
    return m;
}

Csr runs(int64_t n_rows, int64_t n_cols, int w, uint64_t seed) {
    Csr m;
    m.n_cols = n_cols;
    Rng rng(seed);
    for (int64_t r = 0; r < n_rows; r++) {
        const int32_t s = (int32_t)rng.below((uint32_t)(n_cols - w));
        std::vector<int32_t> c;
        for (int j = 0; j < w; j++) c.push_back(s + j);
        m.row(c);
    }
    return m;
}

Csr hubs(int64_t n_rows, int64_t n_cols, uint64_t seed) {
    Csr m;
    m.n_cols = n_cols;
    Rng rng(seed);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c = {4097};
        if (r % 3 == 0) c.push_back(9000);
        for (int j = 0; j < 4; j++) c.push_back((int32_t)rng.below((uint32_t)n_cols));
        m.row(c);
    }
    return m;
}

Csr ragged(int64_t n_rows, int64_t n_cols, uint64_t seed) {
    Csr m;
    m.n_cols = n_cols;
    Rng rng(seed);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c;
        const int n = r == 777 ? 3000 : r % 5 == 0 ? 0 : (int)rng.below(9);
        // no terms in columns [100000, 400000)
        for (int j = 0; j < n; j++) {
            int32_t v = (int32_t)rng.below((uint32_t)(n_cols - 300000));
            c.push_back(v >= 100000 ? v + 300000 : v);
        }
        m.row(c);
    }
    return m;
}

Csr rowspan(int64_t n_rows, int64_t n_cols, uint64_t seed) {
    Csr m;
    m.n_cols = n_cols;
    Rng rng(seed);
    for (int64_t r = 0; r < n_rows; r++) {
        std::vector<int32_t> c;
        if (rng.below(300) == 0) c.push_back((int32_t)rng.below(7000));   // inside one window
        m.row(c);
    }
    return m;
}

void both(const std::string &name, const Csr &m, int slabs, int permille = 1000) {
    const std::string s = name + "/s" + std::to_string(slabs);
    pin(s + "/band2/dma3", m, 0, false, kB2Dma3B2, slabs, permille);
    pin(s + "/band2/wide", m, 0, false, kB2Wide, slabs, permille);
    pin(s + "/cband/dma3", m, 200, true, kB2Dma3Cb, slabs, permille);
    pin(s + "/cband/wide", m, 200, true, kB2Wide, slabs, permille);
}

}  // namespace

int main() {
    printf("{\n");
    for (int slabs : {1, 3, 16}) {
        both("uniform_5000x1000x5", uniform(5000, 1000, 5, 1), slabs);
        both("uniform_1x50000x30", uniform(1, 50000, 30, 4), slabs);
        both("uniform_16384x8192x1", uniform(16384, 8192, 1, 5), slabs);
    }
    both("uniform_40000x20000x3", uniform(40000, 20000, 3, 2), 3);   // three row blocks, the last partial
    both("uniform_3000x70001x40", uniform(3000, 70001, 40, 3), 1);
    both("uniform_3000x70001x40", uniform(3000, 70001, 40, 3), 16);
    both("runs40_1500x7000", runs(1500, 7000, 40, 6), 1);
    both("runs90_1000x7000", runs(1000, 7000, 90, 7), 3);
    both("hubs_20000x20000", hubs(20000, 20000, 8), 3);   // two row blocks: the hub columns split by rows
    both("ragged_20000x600000", ragged(20000, 600000, 9), 16);
    {
        const Csr m = rowspan(16384, 9000, 10);
        pin("rowspan_16384x9000/cband/dma3", m, 7, true, kB2Dma3Cb, 1);
        pin("rowspan_16384x9000/cband/wide", m, 7, true, kB2Wide, 1);
    }
    {   // codebook edges: 255 values take codebook words, 256 take 8-byte entries
        const Csr m = uniform(5000, 9000, 6, 11);
        pin("values255/dma3", m, 255, true, kB2Dma3Cb, 3);
        pin("values256/dma3", m, 256, true, kB2Dma3B2, 3);
    }
    both("slab0_900_20000x20000", uniform(20000, 20000, 3, 2), 4, 900);
    {   // declined: a row with swapped columns, a row with a repeated column
        Csr m = uniform(100, 9000, 6, 12);
        std::swap(m.col[3], m.col[4]);
        pin("swapped/dma3", m, 0, false, kB2Dma3B2, 1);
        m = uniform(100, 9000, 6, 12);
        m.col[4] = m.col[3];
        pin("repeated/dma3", m, 0, false, kB2Dma3B2, 1);
    }
    printf("\n}\n");
    return 0;
}
