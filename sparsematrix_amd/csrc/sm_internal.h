// sm_internal.h -- internal types shared by the C-ABI host code and the HIP
// kernels of libsparsematrix_amd.so.  Not installed; the public surface is
// include/sparsematrix.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "sparsematrix.h"
#include "devmem.h"
#include "merge.h"

namespace smamd {

// ---- stream-kernel geometry (see DESIGN.md "Kernels") ----------------------
constexpr int kStreamThreads = 256;       // 4 wavefronts per workgroup
constexpr int kTileNnz = 4096;            // default terms staged in LDS per row tile (16 KiB)
constexpr int kTileRows = 1024;           // row cap per tile (empty-row heavy graphs)
constexpr int kLongChunk = 4096;          // terms per workgroup for rows > kTileNnz
constexpr int kSerialRowMax = SM_SERIAL_ROW_MAX;  // rows summed in reference order
constexpr int kPadElems = 64;             // zero tail on col/val for aligned x4 loads

// Development knobs.  Builds with -DSM_DEV (tools/*_ab.sh) read SM_* environment
// variables for A/B measurements and ablations; the shipped library reads none of
// them (a stray variable cannot change a caller's layouts or results) and holds no
// ablation kernels.  Layout choices reach it only through sm_build_opts.
inline const char *dev_env(const char *name) {
#ifdef SM_DEV
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Resolved layout options: sm_build_opts with the defaults of sm_build_opts_init filled in for
// what the caller's struct_size leaves out (resolve_opts, layouts.cpp).
using BuildOpts = sm_build_opts;

// Taking turns on scratch that belongs to a matrix (slab partials and hand-off words, long-row
// partials, the relabeled x; the table gradient's partials): work that uses it runs one after
// the other on the device, whatever stream or thread issues it -- correct, the way the
// reference's read-only AddMatMat allows concurrent callers (sparse-matrix.cc:139-194).
struct Turn {
    std::mutex mu;
    hipEvent_t ready = nullptr;   // recorded after the previous user's last launch
    bool recorded = false;
};

// Runs `launch` (which queues on `s` and returns its hipError_t) as the next user of the
// turn's scratch: the stream waits for the previous user's event and records it after its own
// launches, also when one failed (whatever was queued uses the scratch).  A stream being
// captured into a graph is ordered by that stream alone: no event is waited on or recorded.
// `needed` false: the launch uses no scratch and takes no turn.
template <class F>
hipError_t with_turn(Turn &t, hipStream_t s, bool needed, F &&launch) {
    if (!needed) return launch();
    std::lock_guard<std::mutex> lk(t.mu);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
    const bool ordered = cs == hipStreamCaptureStatusNone;
    hipError_t e = hipSuccess;
    if (ordered && !t.ready) e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
    if (ordered && e == hipSuccess && t.recorded) e = hipStreamWaitEvent(s, t.ready, 0);
    if (e != hipSuccess) return e;
    e = launch();
    if (ordered) {
        const hipError_t er = hipEventRecord(t.ready, s);
        if (er == hipSuccess) t.recorded = true;
        if (e == hipSuccess) e = er;
    }
    return e;
}

// Row tile: rows [r0, r1) whose terms fit one LDS tile.  flags bit0: the tile
// holds a row longer than kSerialRowMax (wave-parallel reduction pass needed).
struct alignas(16) Tile {
    int32_t r0, r1, flags, pad;
};

// Chunk of a long row: terms [begin, end) of long row `lr` (index into
// long_rows).  Partial sums are combined in chunk order by the finalize kernel.
struct alignas(16) Chunk {
    int32_t lr, begin, end, pad;
};

// Device copies of the column-band layouts (xband.h, gcb.h): three families of different bytes.
// BandTiles is what all of them hold under one meaning: tiles = n_blocks * n_slabs, each tile a
// block of rows times a slab of columns, walked band by band.
struct BandTiles {
    int32_t kind = 0;                 // XbKind (sm_info.has_xband); 0 when not built
    int32_t block_rows = 0, n_blocks = 0, n_bands = 0;   // n_blocks == 0 when not built
    int32_t n_slabs = 1;
    // Slab scratch (alloc_slab_scratch; null with one slab), one SpMV in flight:
    float *d_partials = nullptr;      // row sets of slab partial sums
    int32_t *d_tickets = nullptr;     // 4 x n_blocks slab hand-off control words, zero between SpMVs
    // Updatable matrices (sm_build_opts.updatable): the slot -> term map of the kinds that hold
    // their own copy of the values, -1: a dummy slot.  XbandDev: one entry per d_val slot (n_term =
    // the slots); Band2Dev / GcbDev: two per 16-byte lane entry of d_ent (n_term = the entries).
    int32_t *d_term = nullptr;
    int64_t n_term = 0;
};

// Exact / blocked / gather kinds (xband.cpp, kernels_xband.hip).
struct XbandDev : BandTiles {
    int32_t *d_chunk_start = nullptr; // per (block, band): its first chunk
    uint32_t *d_word = nullptr;       // per slot: row, rank and column in the band
    float *d_val = nullptr;           // per slot
    int32_t slab_bands = 0, band_cols = 0;   // bands per slab (a multiple of 8), columns per band
    int64_t max_chunks_per_band = 0;  // register capacity the launcher picks its kernel by
    int32_t slab_cols() const { return (int32_t)std::min<int64_t>((int64_t)slab_bands * band_cols, INT32_MAX); }
};

// Band2 / cband kinds (band2.cpp, kernels_band2.hip); also the hot column prefix (Plan::hot).
struct Band2Dev : BandTiles {
    int32_t *d_tile_band = nullptr, *d_band_clo = nullptr;   // tile -> first band (tiles + 1), each band's first column
    uint32_t *d_ent = nullptr;        // lane-interleaved entries: band2 column/row + value, cband words
    float *d_table = nullptr;         // cband: the codebook (table_size <= 255 of 256 floats) the ids index
    int32_t table_size = 0;
    int32_t window = 0;               // x columns a band stages (B2Geom::window)
    int32_t slab_cols = 0, slab0_cols = 0;   // columns per slab s >= 1, and of slab 0
};

// Gathered chunk bands (gcb.cpp / builddev_gcb.hip, kernels_gcb.hip).
struct GcbDev : BandTiles {
    int32_t *d_tile_band = nullptr, *d_band_clo = nullptr;   // tile -> first band (tiles + 1), each band's first column
    uint32_t *d_ent = nullptr;        // lane-interleaved entries, kGcbBandWords per band
    int32_t slab_cols = 0, window = 0;   // columns per slab, the widest column range of a band
};

// Device copy of the sorted sliced-ELL layout (sell.h).
struct SellDev {
    int64_t n_slices = 0;             // 0 when not built
    int64_t *d_off = nullptr;         // n_slices
    int32_t *d_len = nullptr;         // n_slices
    int32_t *d_row = nullptr;         // n_slices * 64 (-1: no row)
    int32_t *d_row_len = nullptr;     // n_slices * 64
    int32_t *d_col = nullptr;         // padded slots (relabeled columns when n_relabel > 0)
    float *d_val = nullptr;           // nullptr in the codebook form
    // Codebook form (sell.h): d_col holds column | id << 24 words, values in d_table.
    float *d_table = nullptr;         // table_size fp32 values (nullptr: plain form)
    int32_t table_size = 0;
    int32_t max_len = 0;              // rows up to this length are whole lanes
    // Rows longer than max_len: cut in segments (lanes with row = -2 - partial).
    int32_t n_long = 0;
    int32_t *d_long_rows = nullptr;   // n_long
    int32_t *d_long_ptr = nullptr;    // n_long + 1 offsets into d_partials
    float *d_partials = nullptr;      // one per segment (one SpMV in flight per matrix)
    // Updatable matrices: per d_val slot the CSR index of its term, -1 = padding (n_term slots).
    int32_t *d_term = nullptr;
    int64_t n_term = 0;
};

// Device copy of the column-chunked sorted sliced-ELL layout (ccsell.h).
struct CcsellDev {
    int64_t n_slices = 0;             // 0 when not built
    int32_t n_chunks = 0, chunk_log2 = 0;
    std::vector<int64_t> chunk_slice; // host: n_chunks + 1 (one launch per chunk)
    int64_t *d_off = nullptr;
    int32_t *d_len = nullptr;
    int32_t *d_row = nullptr;         // row | kCcFirst, -1: no row
    uint16_t *d_row_len = nullptr;
    uint32_t *d_word = nullptr;       // column in chunk (| id << chunk_log2 in the codebook form)
    float *d_val = nullptr;           // plain form
    float *d_table = nullptr;         // codebook form
    int32_t table_size = 0;
    // Updatable matrices: per d_val slot the CSR index of its term, -1 = padding (n_term slots).
    int32_t *d_term = nullptr;
    int64_t n_term = 0;
};

// Device copy of the reference's own stream (native.hip): uint8 deltas + ids, each
// panel's run starting 16-byte aligned (padded with zero-delta fillers).
struct NatBatch {   // one batch of the native two-kernel form (16 bytes, one load)
    int64_t start;     // first entry in the padded stream
    int32_t len;       // entries (<= kNatBatchEntries)
    int32_t carry;     // in-panel offset before the batch (kernel.cc:780-781)
};

struct NativeDev {
    int32_t n_panels = 0;             // panels with entries; 0 when not built
    int32_t n_all = 0;                // + the empty 256-column blocks (beta != 1 launches)
    int64_t s_rows = 0, s_cols = 0;
    uint8_t *d_pos = nullptr, *d_val = nullptr;
    int64_t *d_beg = nullptr, *d_end = nullptr;
    int32_t *d_col = nullptr;
    float *d_table = nullptr;         // table_size raw values
    int32_t table_size = 0;
    // Two-kernel form (panels of more than kNatFusedBatches batches of 4096 entries):
    // per batch its panel and the in-panel offset before it (the reference's running
    // pos_offset, kernel.cc:780-781), per (batch, group of 64 columns) the start of its
    // column lists in d_lists (4 bytes per live entry) and per (batch, group, column)
    // the list's [begin, end) written by the decode kernel.
    int32_t n_batches = 0, max_panel_batches = 0;
    int32_t *d_pbatch = nullptr;      // n_all + 1: first batch of each panel
    NatBatch *d_bmeta = nullptr;      // per batch: stream start, entries, carry
    int32_t *d_boff = nullptr;        // per (batch, group)
    uint32_t *d_lists = nullptr;      // live entries: m = 1 the term's bits, else row | id << 23
    uint32_t *d_hdr = nullptr;        // per (batch, group, column): begin | end << 16
};
constexpr int kNatBatchEntries = 4096;
constexpr int kNatFusedBatches = 2;   // panels of at most this many batches: one fused kernel

struct SweepDev {   // column-swept row blocks (sweep.h)
    int64_t n_blocks = 0, n_chunks = 0;   // n_blocks == 0 when not built
    int64_t *d_block_chunk = nullptr;
    uint32_t *d_ent = nullptr;           // n_chunks * 128
    float *d_table = nullptr;            // 256 raw values (0 past table_size)
    int32_t table_size = 0;
};

// Merge-path SpMV, per workgroup: its first row's end part when that row began in an earlier
// workgroup (first_row >= 0), and its last row's open part (last_row >= 0; last_fresh: the
// part starts with the row's beta * y).
struct MergeRec {
    int32_t first_row;
    float first_val;
    int32_t last_row;
    float last_val;
    int32_t last_fresh;
    int32_t pad[3];
};
// The merge path's staging stream: every slice's terms in ascending column order, as
// (column << 8 | codebook id) words and their place in the slice -- so a wave's x gathers
// hit few cache lines where columns repeat (the hot, relabeled prefix of a skewed graph).
struct MergeStage {
    const uint32_t *w = nullptr;   // nnz words, slice by slice at the CSR positions [z0, z1)
    const uint16_t *z = nullptr;   // nnz positions in the slice (term z0 + z[k] of the CSR)
    const float *table = nullptr;  // 256 codebook values (0 past the table)
};
hipError_t launch_spmv_merge(int32_t n, int32_t nnz, const int32_t *rp, const int32_t *col, const float *val,
                             const float *x, float *y, float alpha, float beta, const int2 *corner, MergeRec *rec,
                             hipStream_t s, const MergeStage *stage = nullptr);

struct Plan {
    // The band layout: at most one of the three families is built (n_blocks == 0 when not).
    XbandDev xb;
    Band2Dev b2;
    GcbDev gcb;
    // What the built family shares with the others (built at all? how many slabs?), or null.
    const BandTiles *band() const {
        if (xb.n_blocks > 0) return &xb;
        if (b2.n_blocks > 0) return &b2;
        return gcb.n_blocks > 0 ? &gcb : nullptr;
    }
    int32_t band_slabs() const { return band() ? band()->n_slabs : 0; }
    // Columns per slab, and of slab 0 (band2 / cband may make it narrower); 0 without bands.
    int32_t band_slab_cols() const { return xb.n_blocks > 0 ? xb.slab_cols() : b2.n_blocks > 0 ? b2.slab_cols : gcb.slab_cols; }
    int32_t band_slab0_cols() const { return b2.n_blocks > 0 && b2.slab0_cols > 0 ? b2.slab0_cols : band_slab_cols(); }
    SellDev sell;                    // n_slices == 0 when not built
    // Unsegmented sorted sliced ELL (every row, any length, in the reference's order):
    // SM_ALGO_EXACT's kernel when no other built layout keeps that order.
    SellDev xsell;
    CcsellDev cc;                     // n_slices == 0 when not built
    NativeDev nat;                    // n_panels == 0 when not built (dense-index matrices)
    SweepDev sw;                      // n_blocks == 0 when not built
    // Skewed graphs: the hottest relabeled columns [0, hot_cols) as codebook bands (x in
    // LDS), the sell layout holding only the other terms.
    Band2Dev hot;                     // n_blocks == 0 when not built
    int32_t hot_cols = 0;
    int32_t tile_nnz = kTileNnz;      // one of 1024, 2048, 4096, 8192
    int32_t n_tiles = 0;
    Tile *d_tiles = nullptr;
    int32_t n_long = 0;
    int32_t *d_long_rows = nullptr;   // n_long
    int32_t *d_long_ptr = nullptr;    // n_long + 1 offsets into chunks
    int32_t n_chunks = 0;
    Chunk *d_chunks = nullptr;
    float *d_partials = nullptr;      // n_chunks long-row partial sums (one SpMV in flight)
    int32_t max_row_nnz = 0;
    double avg_row_nnz = 0.0;
    // Column relabeling for the stream kernel (skewed column degrees):
    // columns renumbered by descending number of terms, so the hot part of x is
    // a dense prefix that stays in L2.  Terms keep their stored order (bit-identical).
    int64_t n_relabel = 0;            // n_cols when built, else 0
    int32_t *d_perm = nullptr;        // original column -> new column (x is scattered)
    int32_t *d_rcol = nullptr;        // relabeled col_idx (nnz + kPadElems, zero tail)
    float *d_xperm = nullptr;         // x in the new numbering (one SpMV in flight)
    // Merge-path SpMV (kernels_merge.hip): one record per workgroup (one SpMV in flight).
    MergeRec *d_merge = nullptr;
    int2 *d_merge_corner = nullptr;   // merge_blocks + 1 slice corners
    uint32_t *d_mstage_w = nullptr;   // the merge path's column-sorted staging stream (MergeStage)
    uint16_t *d_mstage_z = nullptr;
    float *d_mstage_tab = nullptr;
};

// Host launchers (kernels.hip).  All return hipError_t of the launch.
hipError_t launch_spmv_parity(int32_t n, const int32_t *rp, const int32_t *col, const float *val,
                              const float *x, float *y, float alpha, float beta, hipStream_t s);
hipError_t launch_spmv_stream(const Plan &p, const int32_t *rp, const int32_t *col,
                              const float *val, const float *x, float *y, float alpha,
                              float beta, float *partials, hipStream_t s);
hipError_t launch_spmv_xband(const XbandDev &xb, int32_t n_rows, int32_t n_cols, const float *x,
                             float *y, float alpha, float beta, hipStream_t s);
// Sorted sliced-ELL (kernels_sell.hip): rows up to the plan's tile size.
hipError_t launch_spmv_sell(const SellDev &sd, const float *x, float *y, float alpha, float beta,
                            hipStream_t s);
// y[long_rows[i]] = beta * y + partials[long_ptr[i] .. long_ptr[i+1]) in order.
hipError_t launch_long_finalize(int32_t n_long, const int32_t *long_rows, const int32_t *long_ptr,
                                const float *partials, float *y, float beta, hipStream_t s);
// Column-chunked sorted sliced-ELL (kernels_ccsell.hip): one launch per column chunk.
hipError_t launch_spmv_sweep(const SweepDev &sd, int32_t n_rows, int32_t n_cols, const float *x,
                             float *y, float alpha, float beta, hipStream_t s);
hipError_t launch_spmv_ccsell(const CcsellDev &cd, const float *x, float *y, float alpha,
                              float beta, hipStream_t s);
// AddMatMat on the reference's stream (native.hip): C = alpha * A * S + beta * C.
hipError_t launch_native_addmatmat(const NativeDev &nd, int32_t m, const float *a, int32_t lda,
                                   float *c, int32_t ldc, float alpha, float beta, hipStream_t s);
// Gathered chunk bands (kernels_gcb.hip) and the balanced-band kinds (kernels_band2.hip).
hipError_t launch_spmv_gcb(const GcbDev &xb, int32_t n_rows, int32_t n_cols, const float *x, float *y,
                           float alpha, float beta, hipStream_t s);
hipError_t launch_spmv_band2(const Band2Dev &xb, int32_t n_rows, int32_t n_cols, const float *x,
                             float *y, float alpha, float beta, hipStream_t s);
// The launcher of the band family the plan has built (Plan::band() is not null).
inline hipError_t launch_spmv_band(const Plan &p, int32_t n, int32_t nc, const float *x, float *y, float a, float b, hipStream_t s) {
    if (p.b2.n_blocks > 0) return launch_spmv_band2(p.b2, n, nc, x, y, a, b, s);
    if (p.gcb.n_blocks > 0) return launch_spmv_gcb(p.gcb, n, nc, x, y, a, b, s);
    return launch_spmv_xband(p.xb, n, nc, x, y, a, b, s);
}
// xp[rank[c]] = x[c], c < n (rank: original column -> new column).
hipError_t launch_x_relabel(int64_t n, const int32_t *rank, const float *x, float *xp,
                            hipStream_t s);
hipError_t launch_spmv_vector(int32_t n, double avg_row, const int32_t *rp, const int32_t *col,
                              const float *val, const float *x, float *y, float alpha, float beta,
                              hipStream_t s);
// Y(j, i) = beta*Y + alpha * sum_e B[j][e] * X(col_e, i), strides given per index.
hipError_t launch_spmm_generic(int32_t n, int32_t nrhs, const int32_t *rp, const int32_t *col,
                               const float *val, const float *X, int64_t x_sk, int64_t x_si,
                               float *Y, int64_t y_sj, int64_t y_si, float alpha, float beta,
                               bool rhs_fastest, hipStream_t s);
// Row-major X (k x nrhs, ldx) / Y (n x nrhs, ldy), nrhs % 4 == 0, 16-byte aligned.
hipError_t launch_spmm_mfma(int32_t n, const int32_t *rp, const int32_t *col, const float *val,
                            int32_t nnz, const float *X, int64_t ldx, int64_t x_rows, float *Y,
                            int64_t ldy, float alpha, float beta, hipStream_t s);
hipError_t launch_spmm_rowpanel(int32_t n, int32_t nrhs, const int32_t *rp, const int32_t *col,
                                const float *val, int32_t nnz, const float *X, int64_t ldx,
                                int64_t x_rows, float *Y, int64_t ldy, float alpha, float beta,
                                bool allow_pipelined, hipStream_t s);
// SDDMM (kernels_sddmm.hip): out[e] = alpha * <G[row_e, :], X[col_e, :]> + beta * out[e] for every
// stored term e in CSR order.  launch_sddmm_term: one lane per term, the SM_ALGO_PARITY order, any
// placement.  launch_sddmm_panel: lanes share a term's dot; only where sddmm_panel_ok holds
// (n_rhs % 4 == 0, ld % 4 == 0, G and X 16-byte aligned and under 4 GiB).  Workgroups of the
// panel kernel take kSddmmChunk consecutive terms each.
constexpr int kSddmmChunk = 2048;
hipError_t launch_sddmm_term(int32_t n_rows, int32_t nnz, int32_t n_rhs, const int32_t *rp, const int32_t *col,
                             const float *G, int64_t ldg, const float *X, int64_t ldx, float *out, float alpha,
                             float beta, hipStream_t s);
bool sddmm_panel_ok(int64_t n_rows, int64_t n_cols, int32_t n_rhs, const float *G, int64_t ldg, const float *X,
                    int64_t ldx);
hipError_t launch_sddmm_panel(int32_t n_rows, int32_t n_cols, int32_t nnz, int32_t n_rhs, const int32_t *rp,
                              const int32_t *col, const float *G, int64_t ldg, const float *X, int64_t ldx,
                              float *out, float alpha, float beta, hipStream_t s);
// sm_sddmm_table (kernels_sddmm.hip): the same dots, binned by the terms' ids instead of stored.
// One workgroup per chunk of kSddmmChunk terms forms its terms' dots (`panel`: the vector kernel's
// order, only where sddmm_panel_ok holds; else the PARITY order) into LDS and writes
// partials[k * kTablePartialStride + t], t < table_size; launch_table_finish then adds the chunks'
// partials in ascending k and applies alpha / beta.  No atomics; no nnz-sized array.
constexpr int kTablePartialStride = 256;
hipError_t launch_sddmm_table(bool panel, int32_t n_rows, int32_t n_cols, int32_t nnz, int32_t n_rhs,
                              const int32_t *rp, const int32_t *col, const uint8_t *ids, int32_t table_size,
                              const float *G, int64_t ldg, const float *X, int64_t ldx, float *partials,
                              hipStream_t s);
hipError_t launch_table_finish(int64_t n_chunks, int32_t table_size, const float *partials, float *out,
                               float alpha, float beta, hipStream_t s);
hipError_t launch_beta(float *c, int32_t m, int32_t n, int64_t ldc, float beta, hipStream_t s);
hipError_t launch_transpose(const float *a, int32_t m, int32_t n, int64_t lda, float *sa,
                            int64_t ldsa, hipStream_t s);
// Device CopyForm scan (encode_dev.hip).  trans: one count per index row (B row);
// otherwise one count per (chunk of chunk_rows index rows, index column), chunk-major.
hipError_t launch_encode_count(const uint8_t *dm, int32_t rows, int32_t cols, int32_t stride,
                               bool trans, int32_t chunk_rows, int32_t n_chunks, uint8_t T,
                               int32_t *cnt, hipStream_t s);
hipError_t launch_encode_fill(const uint8_t *dm, int32_t rows, int32_t cols, int32_t stride,
                              bool trans, int32_t chunk_rows, int32_t n_chunks, uint8_t T,
                              const int32_t *offs, const float *table, int32_t *col, float *val,
                              uint8_t *ids, hipStream_t s);
// The reference encoding from a device CSR (refenc_dev.hip): encode_csr_ref's result and
// return codes (encode.h), -5 on a HIP error (err).  d_ids: the terms' ids (then `table`
// is the codebook they index), else ids from the values (table, or the derived codebook).
struct EncodeResult;
int encode_csr_ref_device(const int32_t *d_rp, const int32_t *d_col, const float *d_val, const uint8_t *d_ids,
                          int64_t n_rows, int64_t n_cols, int64_t nnz, const float *table,
                          int32_t table_size, EncodeResult &out, hipStream_t s, hipError_t &err);
// Device builders (builddev.hip) on a matrix whose CSR is on the device: the column
// relabeling (check_skew: only if the top 1/16 of the columns hold >= 40 % of the terms) and
// the sorted sliced ELL (codebook form when the values allow), the bytes upload_relabel and
// upload_sell build on the host.  0 built or declined as the host would, -5 HIP error (err).
int devbuild_relabel(sm_matrix *m, bool check_skew, hipStream_t s, hipError_t &err);
int devbuild_sell(sm_matrix *m, int32_t max_len, bool codebook, hipStream_t s, hipError_t &err);
// The codebook of a device value array (builddev.hip), as codebook_ids derives it: `table` in
// first-occurrence order, d_ids[e] (n bytes on the device) the id of value e.  0 built, 1 more
// than 255 distinct bit patterns, -5 HIP error (err).
int devbuild_codebook(const float *d_val, int64_t n, std::vector<float> &table, uint8_t *d_ids, hipStream_t s,
                      hipError_t &err);
// The merge path's staging stream (merge_stage_build's bytes) from the device CSR and the
// plan's slice corners: 0 built, 1 declined as the host would, < 0 on a HIP error (err).
int devbuild_merge_stage(sm_matrix *m, hipStream_t s, hipError_t &err);
// Layout decisions and host builders (layouts.cpp), which the constructors of create.cpp end in.
// resolve_opts: the caller's sm_build_opts with defaults for what its struct_size leaves out
// and, in -DSM_DEV builds only, the SM_* development variables on top.  check_opts: the
// options' ranges and exclusions (`table_ok`: the constructor builds a table matrix, the only
// ones that honour table_updatable).
BuildOpts resolve_opts(const sm_build_opts *o);
sm_status check_opts(const sm_build_opts *o, bool table_ok = false);
// The CSR arrays of `m` (its sizes set): col / val carry a zeroed tail of kPadElems.
sm_status alloc_csr(sm_matrix *m);
// Common tails of the constructors.  Host CSR: uploads it, plans and builds the layouts.
// Device CSR: `m` holds its sizes, options and the CSR arrays (alloc_csr) filled on `s`;
// validates them by a kernel, plans, and builds the layouts on the device or the host as the
// options ask; synchronises `s`.  `exact_sell`: also the unsegmented sliced ELL where
// want_exact_sell asks for it (the host constructors' last step).  A table_updatable matrix's
// host builders take the matrix's own ids and table: the host tail is given them (`ids`, `table`),
// the device tail downloads m->d_tab_ids and m->d_tab itself.
sm_status finish_from_host_csr(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val,
                               const uint8_t *ids = nullptr, const float *table = nullptr);
sm_status finish_from_device_csr(sm_matrix *m, hipStream_t s, bool exact_sell);
// The reference's stream the matrix holds on the host, on the device (native.hip).
sm_status upload_native(sm_matrix *m);
// SM_ALGO_EXACT's choice for `m` (x 16-byte aligned: `x16`): an sm_algo, or kAlgoExactSell
// for the unsegmented sliced ELL built for it.
constexpr int kAlgoExactSell = 100;
int exact_algo(const sm_matrix *m, bool x16);
// The gathered chunk bands (builddev_gcb.hip): gcb_build's bytes into m->plan.gcb's d_tile_band,
// d_band_clo and d_ent, the geometry in `meta` (its vectors stay empty).  0 built, 1 declined as
// gcb_build would (the caller drops what it allocated till then: DevMem::release_since), < 0 on
// a HIP error (err) or a builder inconsistency.
struct GcbHost;
int devbuild_gcb(sm_matrix *m, int rows_log2, int32_t n_slabs, int32_t window, GcbHost &meta, hipStream_t s,
                 hipError_t &err);
// The balanced bands (builddev_band2.hip): the bytes build_band2 has band2_build produce -- the
// geometry by `geo_opt` (sm_build_opts.band_tall: dma3 first unless 6, wide where dma3's bands
// would be under 70 % full and not `forced`), codebook words for `kind` kXbCband where the values
// take at most 255 bit patterns (`table`: the codebook) -- into m->plan.b2's d_tile_band,
// d_band_clo and d_ent, the geometry in `meta` (its vectors stay empty).  0 built, 1 declined as
// build_band2 would, or because a development knob is set or the scratch does not fit the device
// (the caller drops what was allocated till then: DevMem::release_since), < 0 on a HIP error (err)
// or a builder inconsistency.
struct Band2Host;
int devbuild_band2(sm_matrix *m, int32_t kind, int32_t geo_opt, int32_t n_slabs, bool forced, int32_t slab0_permille,
                   Band2Host &meta, std::vector<float> &table, hipStream_t s, hipError_t &err);
// The CSR of B^T (transpose_dev.hip) from the device CSR of B (n_rows x n_cols, validated): row c
// holds column c's terms by ascending source row, equal rows in stored order; values bit for
// bit.  t_rp: n_cols + 1, t_col / t_val: nnz, on the same device.  Synchronises `s`; frees its
// scratch and leaves no sticky HIP error on failure.
hipError_t transpose_csr_device(const int32_t *rp, const int32_t *col, const float *val, int64_t n_rows,
                                int64_t n_cols, int64_t nnz, int32_t *t_rp, int32_t *t_col, float *t_val,
                                hipStream_t s);
// The terms' codebook ids (one byte per term, CSR order, on the device) in the order the
// transposition above gives the terms.
hipError_t transpose_ids_device(const int32_t *rp, const int32_t *col, const uint8_t *ids, int64_t n_rows,
                                int64_t n_cols, int64_t nnz, uint8_t *t_ids, hipStream_t s);
// The transposition's term map: t_src[j] = the CSR index in B of term j of B^T (sm_set_values
// with SM_VALUES_SOURCE) -- the term index carried through the same pack / sort / unpack.
hipError_t transpose_terms_device(const int32_t *rp, const int32_t *col, int64_t n_rows, int64_t n_cols,
                                  int64_t nnz, int32_t *t_src, hipStream_t s);
// In-place value updates (kernels_values.hip).  CSR step: val[e] = in[i] (axpy: fl(val[e] +
// fl(a * in[i]))), i = e, or src[e] when `src` is given.  Refresh steps: slot s takes val[map[s]]
// where map[s] >= 0 -- plain float slots, or the value words 2-3 of 16-byte lane entries (two map
// entries per lane entry).
hipError_t launch_values_csr(int64_t nnz, bool axpy, float a, const float *in, const int32_t *src, float *val,
                             hipStream_t s);
hipError_t launch_refresh_plain(int64_t n_slots, const int32_t *map, const float *val, float *slot, hipStream_t s);
hipError_t launch_refresh_entry(int64_t n_ent, const int32_t *map, const float *val, uint32_t *ent, hipStream_t s);
// In-place table updates (kernels_values.hip).  Table step: one workgroup computes the new entries
// (set: in[t]; axpy: fl(tab[t] + fl(a * in[t]))), t < table_size, and stores them into the
// authoritative table and every layout's copy (dst[i], n[i] entries: zero past table_size).
// CSR step: val[e] = tab[ids[e]], one pass of 1 + 4 bytes per term.
struct TableDst {
    float *p[8];
    int32_t n[8];
    int32_t count;
};
hipError_t launch_table_step(int32_t table_size, bool axpy, float a, const float *in, float *tab,
                             const TableDst &dst, hipStream_t s);
hipError_t launch_values_from_table(int64_t nnz, const uint8_t *ids, const float *tab, float *val, hipStream_t s);
// Quantising the stored values (kernels_quantize.hip).  launch_expand_ids: val[e] = table[ids[e]]
// bit for bit (`table`: T floats on the device; any alignment of `ids`), *flag |= 1 on an id >= T.
// launch_quantize_minmax: parts[2b], parts[2b + 1] = the least / greatest value of workgroup b's
// share (quantize_minmax_blocks(nnz) workgroups), *flag |= 1 on a NaN or Inf.
// launch_quantize_assign: sm_quantize_assign's rule for every term.  launch_quantize_chunks: the
// per-chunk sums, counts and squared distances of sm_quantize_update into psum / pcnt
// (ceil(nnz / kSddmmChunk) rows of kTablePartialStride; the sse in slot 255), *flag |= 1 on an id
// >= T.  launch_quantize_finish: the chunks in ascending order, the new table, counts and sse
// (either may be null).
hipError_t launch_expand_ids(int64_t nnz, const uint8_t *ids, const float *table, int32_t T, float *val,
                             int32_t *flag, hipStream_t s);
int64_t quantize_minmax_blocks(int64_t nnz);
hipError_t launch_quantize_minmax(int64_t nnz, const float *val, float *parts, int32_t *flag, hipStream_t s);
hipError_t launch_quantize_assign(int64_t nnz, const float *val, const float *table, int32_t T, uint8_t *ids,
                                  hipStream_t s);
hipError_t launch_quantize_chunks(int64_t nnz, const float *val, const float *table, int32_t T, const uint8_t *ids,
                                  double *psum, int32_t *pcnt, int32_t *flag, hipStream_t s);
hipError_t launch_quantize_finish(int64_t n_chunks, int32_t T, const double *psum, const int32_t *pcnt, float *table,
                                  int32_t *counts, double *sse, hipStream_t s);
// Pruning the stored terms (kernels_prune.hip).  prune_mask_device: sm_prune_mask's rule for the
// values of a validated device CSR into keep[0, nnz) (any alignment), *kept (host, may be null)
// the number of ones; the arguments are checked by the caller; allocates its scratch, synchronises
// `s` and leaves no sticky HIP error on failure.  prune_positions_device: pos[e] = the number of
// kept terms before e, for e in [0, nnz] (`pos`: nnz + 1 entries), *new_nnz = pos[nnz];
// synchronises `s`.  launch_prune_compact: new_rp[r] = pos[rp[r]] and, for every kept term e,
// new_col / new_val / src_term (/ new_ids when `ids` is given) at pos[e]; `any_kept` false: only
// the row pointer (the term arrays may then be null).
hipError_t prune_mask_device(const int32_t *rp, const float *val, int64_t n_rows, int64_t nnz, sm_prune_mode mode,
                             int64_t count, float threshold, uint8_t *keep, int64_t *kept, hipStream_t s);
hipError_t prune_positions_device(int64_t nnz, const uint8_t *keep, int32_t *pos, int64_t *new_nnz, hipStream_t s);
hipError_t launch_prune_compact(int64_t n_rows, int64_t nnz, const uint8_t *keep, const int32_t *pos,
                                const int32_t *rp, const int32_t *col, const float *val, const uint8_t *ids,
                                int32_t *new_rp, int32_t *new_col, float *new_val, int32_t *src_term, uint8_t *new_ids,
                                bool any_kept, hipStream_t s);
// From and to dense weights (kernels_dense.hip).  dense_mask_device: sm_prune_mask's rule for the
// full CSR that W stands for (n_rows x n_cols at w[r * ld + c], E = n_rows * n_cols in
// [1, 2^32 - 1], the arguments checked by the caller, a top-k count >= 1) into a byte mask over
// whole chunks of kSddmmChunk elements in i = r * n_cols + c order (zero past E) and base[ch], the
// kept elements before chunk ch (n_chunks + 1 entries), both allocated from `t`; *kept = their
// number.  Synchronises `s`; leaves no sticky HIP error on failure.  launch_dense_fill: the
// compaction by that mask into rp (n_rows + 1), col and val (kept < 2^31 entries).
// launch_dense_zero: zeros over columns [0, width) of `rows` rows of `out`.  launch_scatter_terms:
// launch_scatter_dense's stores by one thread per term, for a matrix whose rows strictly ascend.
hipError_t dense_mask_device(const float *w, int64_t n_rows, int64_t n_cols, int64_t ld, sm_prune_mode mode,
                             int64_t count, float threshold, DevScratch &t, uint8_t **keep, uint32_t **base,
                             int64_t *kept, hipStream_t s);
hipError_t launch_dense_fill(const float *w, int64_t n_rows, int64_t n_cols, int64_t ld, const uint8_t *keep,
                             const uint32_t *base, int32_t *rp, int32_t *col, float *val, hipStream_t s);
hipError_t launch_dense_zero(float *out, int64_t rows, int64_t width, int64_t ld, hipStream_t s);
hipError_t launch_scatter_terms(int32_t n_rows, int64_t nnz, const int32_t *rp, const int32_t *col, const float *val,
                                float *out, int64_t ld, bool b_layout, hipStream_t s);
// The sum of two matrices (kernels_sum.hip), both validated device CSRs of n_rows rows whose rows
// strictly ascend.  sum_count_device: the match words of A's terms (m[i] = B's term index where B
// stores the position, ~(the lower bound of the column in B's row) where not), their exclusive
// scan S (nnz_a + 1 entries) and the union's row pointer rp_c (n_rows + 1 entries, formed in
// unsigned 32 bits), all allocated from `t`; *nnz_c = the union's size, which the caller checks
// before it reads rp_c as int32.  Synchronises `s`; leaves no sticky HIP error on failure.
// launch_sum_fill: col_c, val_c (sm_create_sum's value rule) and both source maps, nnz_c entries
// each, every one written once.
hipError_t sum_count_device(int64_t n_rows, int64_t nnz_a, int64_t nnz_b, const int32_t *rp_a, const int32_t *col_a,
                            const int32_t *rp_b, const int32_t *col_b, DevScratch &t, int32_t **m, int32_t **S,
                            int32_t **rp_c, uint64_t *nnz_c, hipStream_t s);
hipError_t launch_sum_fill(int64_t n_rows, int64_t nnz_a, int64_t nnz_b, const int32_t *rp_a, const int32_t *col_a,
                           const float *val_a, float alpha, const int32_t *rp_b, const int32_t *col_b,
                           const float *val_b, float beta, const int32_t *m, const int32_t *S, const int32_t *rp_c,
                           int32_t *col_c, float *val_c, int32_t *terms_a, int32_t *terms_b, hipStream_t s);
// *d_flag |= 1, 2, 4 (row_ptr: start, end, order or range), 8 (a column out of range): the CSR is
// invalid; |= kCsrNotAscending where some row has col[e] >= col[e + 1]: valid, but see
// sm_matrix::rows_ascend.
constexpr int32_t kCsrInvalid = 15, kCsrNotAscending = 16;
hipError_t launch_validate(int32_t n_rows, int32_t n_cols, int32_t nnz, const int32_t *rp,
                           const int32_t *col, int32_t *d_flag, hipStream_t s);
// Dense decode: out is zeroed by the caller.  b_layout: out[row*stride+col]
// (B = S^T, CopyTo Trans); else out[col*stride+row] (S, CopyTo NoTrans).
hipError_t launch_scatter_dense(int32_t n, const int32_t *rp, const int32_t *col,
                                const float *val, float *out, int64_t stride, bool b_layout,
                                hipStream_t s);
hipError_t launch_panel_kernel(int variant, int32_t m, int32_t n, int32_t k, const float *a,
                               int32_t lda, float *c, int32_t ldc, float alpha,
                               const uint8_t *ppos, const uint8_t *pval, int32_t pos_len,
                               const float *table, int32_t valid_table_size, void *workspace,
                               hipStream_t s);
size_t panel_kernel_workspace_bytes(int32_t pos_len, int32_t n);

}  // namespace smamd

// The opaque handle.
struct sm_matrix {
    int32_t device = 0;
    int64_t n_rows = 0, n_cols = 0, nnz = 0;   // CSR of B = S^T
    int64_t s_rows = 0, s_cols = 0;            // reference S view
    int32_t *d_row_ptr = nullptr;
    int32_t *d_col = nullptr;
    float *d_val = nullptr;
    smamd::Plan plan;
    smamd::BuildOpts opts;                     // layout options the matrix was built with
    // Every device buffer the matrix keeps (the raw d_* pointers here and in `plan` point into
    // it); mem.bytes is sm_info.device_bytes.  ~sm_matrix frees them all.
    smamd::DevMem mem;
    uint32_t built_on_device = 0;              // SM_BUILT_DEV_* of the layouts the device builders made
    // Every row's columns strictly ascend (found by the constructors' validation): no (row, column)
    // is stored twice, so sm_to_dense_device may scatter the terms in any order.
    bool rows_ascend = false;
    ~sm_matrix();
    // Reference encoding (only for matrices built by sm_create_from_dense_index).
    bool has_ref = false;
    bool from_index = false;   // built by the CopyForm constructors (the reference's path)
    int32_t table_size = 0;
    std::vector<float> table;                  // table_size + 1, last = 0
    // The terms' ids into `table` (nnz bytes, CSR order), only on a matrix sm_create_transpose
    // made from a CopyForm-built one: equal codebook entries keep the ids the index gave them,
    // so sm_build_ref_stream with that codebook yields the reference's own stream.  Invariant:
    // they index `table` and exist only while has_ref is false (sm_build_ref_stream frees them:
    // the stream then holds the ids, and sm_create_transpose reads them back from it).
    uint8_t *d_term_ids = nullptr;
    // Updatable matrix made by sm_create_transpose, and every matrix made by sm_create_masked /
    // sm_create_pruned: per term its CSR index in the source matrix (nnz entries), so values given
    // in the source's order reach it (SM_VALUES_SOURCE; sm_copy_source_terms_device reads it).
    int32_t *d_src_term = nullptr;
    bool has_src_term = false;   // (also true with nnz == 0, where there is nothing to allocate)
    // Every matrix made by sm_create_sum: per term its CSR index in each operand, or -1 (nnz
    // entries each; sm_copy_sum_terms_device reads them).  There is no single source, so
    // has_src_term stays false.
    int32_t *d_sum_terms_a = nullptr, *d_sum_terms_b = nullptr;
    bool has_sum_terms = false;   // (also true with nnz == 0)
    // Table matrix (sm_create_from_csr_ids and its transposes): the terms' ids (nnz bytes, CSR
    // order) and the authoritative table (256 floats, zero past tab_size) on the device, and the
    // per-chunk partials of sm_sddmm_table (tab_chunks * kTablePartialStride floats), used in
    // turn (table_turn).  These fields are apart from table / d_term_ids above, whose invariants
    // belong to the dense-index path.
    bool is_table = false;
    int32_t tab_size = 0;
    uint8_t *d_tab_ids = nullptr;
    float *d_tab = nullptr;
    float *d_tab_partials = nullptr;
    int64_t tab_chunks = 0;
    mutable smamd::Turn table_turn;
    // While a table_updatable matrix's host builders run: the host copies they take their ids and
    // table from (set and cleared by layouts.cpp's build_host_layouts alone; null otherwise).
    const uint8_t *build_ids = nullptr;
    const float *build_table = nullptr;
    std::vector<uint8_t> pos, val;
    std::vector<int32_t> panel_row_off, panel_col_off;
    std::vector<int64_t> panel_begin, panel_end;
    // Workspace of the row-panel AddMatMat (sm_addmatmat, 2 <= m <= 128), kept across
    // calls.  Each call makes its stream wait on ws_ready (recorded after the previous
    // call's last kernel), so calls on any streams use it in turn; it grows (after its
    // last user has drained) only when a call needs more.
    mutable std::mutex ws_mu;
    mutable float *d_ws = nullptr;
    mutable size_t ws_bytes = 0;
    mutable hipEvent_t ws_ready = nullptr;
    // SpMV scratch (slab partials and hand-off words, long-row partials, the relabeled x, the
    // native form's column lists) belongs to the matrix: SpMVs that use it take turns.
    mutable smamd::Turn scratch_turn;
};
