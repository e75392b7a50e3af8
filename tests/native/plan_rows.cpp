// The stream kernel's row-tile planner (plan.cpp plan_rows) as a stand-alone program, built with
// AddressSanitizer and UBSan by tests/test_stream_plan_cpu.py, which holds its printout against
// the restatement in tests/stream_ref.py.
//   plan_rows FILE TILE_NNZ TILE_ROWS CHUNK_NNZ SERIAL_MAX
// FILE: a row_ptr as raw int32 (n_rows + 1 values).  Prints one line per tile ("tile r0 r1 flags"),
// per chunk ("chunk long_row begin end") and per long row ("long row first_chunk end_chunk"), then
// max_row_nnz, avg_row_nnz and "plan_rows: ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "encode.h"

using namespace smamd;

int main(int argc, char **argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s FILE TILE_NNZ TILE_ROWS CHUNK_NNZ SERIAL_MAX\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<int32_t> rp;
    int32_t v;
    while (fread(&v, sizeof v, 1, f) == 1) rp.push_back(v);
    fclose(f);
    if (rp.empty() || rp[0] != 0) {
        fprintf(stderr, "plan_rows: not a row_ptr\n");
        return 2;
    }
    for (size_t i = 1; i < rp.size(); ++i)
        if (rp[i] < rp[i - 1]) {
            fprintf(stderr, "plan_rows: row_ptr descends at %zu\n", i);
            return 2;
        }
    // exactly n_rows + 1 values on the heap: a read of rp[n_rows + 1] is ASan's to report
    std::vector<int32_t> exact(rp.begin(), rp.end());
    exact.shrink_to_fit();
    const int64_t n = (int64_t)exact.size() - 1;
    PlanHost p;
    plan_rows(exact.data(), n, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), p);
    for (const TileHost &t : p.tiles) printf("tile %d %d %d\n", t.r0, t.r1, t.flags);
    for (const ChunkHost &c : p.chunks) printf("chunk %d %d %d\n", c.lr, c.begin, c.end);
    if (p.long_ptr.size() != p.long_rows.size() + 1) {
        fprintf(stderr, "plan_rows: long_ptr has %zu entries for %zu long rows\n", p.long_ptr.size(),
                p.long_rows.size());
        return 1;
    }
    for (size_t i = 0; i < p.long_rows.size(); ++i)
        printf("long %d %d %d\n", p.long_rows[i], p.long_ptr[i], p.long_ptr[i + 1]);
    printf("max_row_nnz %d\n", p.max_row_nnz);
    printf("avg_row_nnz %.17g\n", p.avg_row_nnz);
    printf("plan_rows: ok\n");
    return 0;
}
