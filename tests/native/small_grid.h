// The grid of small cases of tests/small_shapes.py, restated for the stand-alone builder
// programs: the same 13 shapes and 6 patterns with the same columns (no RNG in the structure).
// Values: `cb` takes 200 distinct bit patterns (a codebook), `plain` one per term, `small`
// integers in [-48, 48] (sell_asan.cpp derives its ids from them).  report() prints the line
// tests/test_xband_builder.py reads: whether the builder took or declined the case.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace small_grid {

struct Shape { int rows, cols; };
static const Shape kShapes[] = {{1, 1},     {1, 5},     {5, 1},     {2, 3},     {63, 65},
                                {64, 64},   {65, 63},   {255, 257}, {256, 256}, {257, 255},
                                {300, 513}, {300, 767}, {300, 768}};
static const char *const kPatterns[] = {"one", "diag", "last_col", "row0_full", "dense", "sparse"};
constexpr int kNumPatterns = 6;

struct Csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int32_t> rp, col;
    std::vector<float> cb, plain, small;
};

inline Csr make(Shape s, int pattern) {
    Csr m;
    m.n_rows = s.rows;
    m.n_cols = s.cols;
    m.rp.assign(1, 0);
    const char *p = kPatterns[pattern];
    for (int r = 0; r < s.rows; r++) {
        std::vector<int32_t> c;
        if (!strcmp(p, "one")) {
            if (r == s.rows - 1) c.push_back(s.cols - 1);
        } else if (!strcmp(p, "diag")) {
            if (r < s.cols) c.push_back(r);
        } else if (!strcmp(p, "last_col")) {
            c.push_back(s.cols - 1);
        } else if (!strcmp(p, "row0_full") || !strcmp(p, "dense")) {
            if (r == 0 || !strcmp(p, "dense"))
                for (int j = 0; j < s.cols; j++) c.push_back(j);
        } else if (r % 5 != 4) {   // sparse
            c = {(7 * r + 1) % s.cols, (13 * r + 5) % s.cols, (29 * r + 11) % s.cols};
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
        }
        m.col.insert(m.col.end(), c.begin(), c.end());
        m.rp.push_back((int32_t)m.col.size());
    }
    for (size_t e = 0; e < m.col.size(); e++) {
        m.cb.push_back((float)((37 * e + 11) % 200) * 0.25f - 9.0f);
        m.plain.push_back(1.0f + (float)e * 0.001f);
        m.small.push_back((float)((37 * e + 11) % 97) - 48.0f);
    }
    return m;
}

inline void report(const char *layout, Shape s, int pattern, bool built) {
    printf("grid %s %dx%d %s %s\n", layout, s.rows, s.cols, kPatterns[pattern], built ? "built" : "declined");
}

// for_each(f): f(shape, pattern index, csr) over the whole grid.
template <class F>
inline void for_each(F &&f) {
    for (const Shape &s : kShapes)
        for (int p = 0; p < kNumPatterns; p++) f(s, p, make(s, p));
}

}  // namespace small_grid
