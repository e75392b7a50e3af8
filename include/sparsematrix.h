/*
 * sparsematrix.h -- C ABI of sparsematrix_amd (libsparsematrix_amd.so), an
 * MI355X-native (gfx950) replacement for NeverLEX/sparsematrix's sparse x dense
 * multiply.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Orientation.  The reference stores S (k x n) and computes, for a dense
 * row-major A (m x k) and C (m x n),  C = alpha*A*S + beta*C
 * (sparse-matrix.h:37, sparse-matrix.cc:139-194).  Here the matrix is held on
 * the device as CSR of B = S^T (n rows x k columns, int32 row_ptr/col_idx,
 * fp32 values), so m = 1 is the SpMV  y = alpha*B*x + beta*y  and a panel of
 * N right-hand sides is the SpMM  Y = alpha*B*X + beta*Y  (X: k x N, Y: n x N,
 * both row-major).  sm_num_rows/sm_num_cols report the reference's S view
 * (rows_ = k, cols_ = n; sparse-matrix.h:39-40).  The other orientation,
 * y = alpha*B^T*x + beta*y  (the reference's  C = alpha*A*S^T + beta*C), is the same
 * product on the matrix sm_create_transpose builds from a held one.
 *
 * Semantics kept from the reference (SURVEY.md §7 "Drop-in semantics"):
 *   - beta is applied by multiplication whenever beta != 1 (so beta = 0
 *     propagates NaN/Inf already in C/y)                 kernel.cc:10-29
 *   - alpha == 0 skips the product entirely              sparse-matrix.cc:152
 *   - alpha is folded into the stored value first: each term is
 *     x * (v * alpha), added one at a time               kernel.cc:791, 580-582
 *   - ids >= table_size are not stored; explicit 0.0 table entries are
 *                                                        sparse-matrix.cc:44, 77
 *   - subnormal operands, terms and sums are kept: no kernel flushes them, and the build must
 *     not enable flush-to-zero (-fgpu-flush-denormals-to-zero changes every subnormal result)
 *   - "bit-identical" covers every output that is not a NaN.  A NaN result is a NaN where the
 *     reference has one; its sign and payload are the hardware's, and no kernel canonicalises
 *     them.  The x86 reference generates 0xFFC00000 for inf - inf and for 0 * inf; the MI355X
 *     was observed to generate 0xFFC00000 for both as well (tests/test_gpu_range_edges.py), but
 *     only the NaN itself is promised.
 * Summation order: SM_ALGO_PARITY adds the terms of every output in stored
 * (ascending column) order, exactly as the reference does, so results are
 * bit-identical to the reference CPU kernel.  SM_ALGO_XBAND keeps that order for
 * every row on the exact band layout (sm_info.has_xband == 1, or any layout with
 * xband_slabs == 1); the slab layouts (has_xband 2-5) sum each column slab in
 * order and add the slab sums in slab order (band2 / cband after beta*y:
 * sm_info.xband_beta_last).  SM_ALGO_SELL keeps it for every row
 * of up to 2048 terms and adds longer rows' 2048-term segment sums in order.  The
 * SpMM kernels keep it for every row.  SM_ALGO_STREAM keeps it for rows of up to
 * SM_SERIAL_ROW_MAX terms and uses a tree sum for longer rows.  The bound for
 * every non-exact case is |y - y_ref| <= 1e-6 * sum|terms|.
 *
 * Operands: any 4-byte aligned x / y / X / Y / a / c and any ld >= the row length; placement
 * only selects the kernel (band layouts need x at 16 bytes, the row-panel SpMM ld % 4 == 0 and
 * X, Y at 16 bytes, SM_ALGO_MFMA 8 bytes), and nothing outside y[0, n) or inside the padding
 * columns [n_rhs, ld) is ever written ("Operand placement").  Size selects the
 * kernel in the same way: the gather-pipelined row-panel SpMM and SM_ALGO_MFMA form 32-bit byte
 * offsets, so they run only with X and the term arrays under 4 GiB (n_cols * ldx * 4 and
 * nnz * 4 bytes, each below 0xFFFFFFF0); past either limit the SpMM runs the plain row-panel
 * kernel (the same bits) and SM_ALGO_MFMA returns SM_ERR_NOT_SUPPORTED.
 *
 * Concurrency: calls on one matrix from several streams or threads are correct;
 * SpMVs that use the matrix's scratch take turns on the device.
 * sm_set_values / sm_axpy_values are the exception: they write the matrix, so the caller
 * orders them against products of the same matrix on other streams (an event, or one
 * stream: a stream's own order is enough).
 *
 * Errors: every call returns sm_status; sm_last_error() gives a message for
 * the calling thread.  Device calls are asynchronous on `stream` (a
 * hipStream_t; NULL = the legacy default stream) unless stated otherwise.
 */
#ifndef SPARSEMATRIX_AMD_H
#define SPARSEMATRIX_AMD_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define SM_API __attribute__((visibility("default")))
#else
#define SM_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sm_status {
    SM_OK = 0,
    SM_ERR_INVALID_ARG = 1,     /* bad shape, stride, pointer or enum          */
    SM_ERR_OUT_OF_MEMORY = 2,   /* host or device allocation failed            */
    SM_ERR_HIP = 3,             /* a HIP runtime call failed                   */
    SM_ERR_NOT_SUPPORTED = 4,   /* operation not available for this matrix     */
    SM_ERR_TOO_LARGE = 5,       /* exceeds int32 indexing (nnz or rows >= 2^31) */
    SM_ERR_INVALID_MATRIX = 6,  /* CSR failed validation (col out of range...) */
    SM_ERR_NO_DEVICE = 7        /* no HIP device visible                       */
} sm_status;

/* SBLAS_TRANSPOSE, sparse-matrix.h:20-23 */
typedef enum sm_trans { SM_NO_TRANS = 0, SM_TRANS = 1 } sm_trans;

typedef enum sm_algo {
    SM_ALGO_AUTO = 0,     /* band layout if built, else sell, else stream (SpMV); row-panel (SpMM) */
    SM_ALGO_PARITY = 1,   /* bit-exact with the reference for every row            */
    SM_ALGO_STREAM = 2,   /* nnz-balanced row tiles through LDS (+ long-row split).  One fixed
                             order per row, every operation rounded separately, a term being
                             t = fl(x[c] * fl(v * alpha)) and by = fl(beta * y) (y itself when
                             beta == 1):
                             - a row of <= SM_SERIAL_ROW_MAX terms: by, then its terms in stored
                               order (the reference's bits);
                             - a longer row of <= tile_nnz terms: lane l of 64 adds the row's
                               terms l, l + 64, ... from +0.0, the lane sums are added in an
                               xor tree at lane distances 32 .. 1, y = fl(by + that);
                             - a row of more than tile_nnz terms (sm_info.n_long_rows counts
                               them) is cut into chunks of 4096 terms from its first term.  In
                               a chunk [begin, end), thread t of 256 adds the term indices
                               (begin & ~3) + 4 t + q + 1024 j, q = 0 .. 3, j = 0, 1, ..., that
                               lie in the chunk, ascending, from +0.0; each wavefront's 64 sums
                               go through the same xor tree; wavefronts 0 .. 3 are added in
                               order; the chunk sums are added onto by in chunk order.
                             So a row's bits depend on tile_nnz only through which of the last
                             two cases it falls in: sm_build_opts.tile_nnz changes the bits of
                             the rows whose length lies between two sizes, and of no other row.
                             Deterministic; every row within the sum|terms| bound.            */
    SM_ALGO_VECTOR = 3,   /* L lanes per row (CSR-vector), L = the first of 2, 4, .. 64 that is
                             not below nnz / n_rows: lane l adds the row's terms l, l + L, ...
                             from +0.0 (terms as for STREAM), the L sums are added in an xor tree
                             at lane distances L/2 .. 1, y = fl(by + that) -- for every row, so a
                             row without terms ends as fl(by + 0.0) (+0.0 where by is -0.0).
                             Deterministic; every row within the sum|terms| bound.            */
    SM_ALGO_XBAND = 4,    /* x staged through LDS in column bands (the layout built at
                             creation, see sm_info.has_xband); falls back to SELL, then
                             STREAM, when the matrix holds no band layout             */
    SM_ALGO_SELL = 5,     /* sorted sliced-ELL, one lane per row (every row up to 2048
                             terms bit-identical; longer rows in 2048-term segments whose
                             sums are added in order); STREAM when not built           */
    SM_ALGO_NATIVE = 6,   /* the reference's own stream (uint8 deltas + ids, 256-column
                             panels) decoded on the device; bit-identical for every
                             output; only for matrices built from the dense index
                             (SM_ERR_NOT_SUPPORTED otherwise)                          */
    SM_ALGO_EXACT = 7,    /* the fastest kernel built for the matrix that adds every
                             output's terms in the reference's order (bit-identical):
                             the column-swept or one-slab band layout, the column-chunked
                             or segment-free sliced ELL, the stream kernel when no row
                             exceeds SM_SERIAL_ROW_MAX terms, else PARITY.  SpMM and
                             AddMatMat with m > 1: the row-panel kernels (every row in
                             order).  What the reference's C++ surface (libsblas) runs. */
    SM_ALGO_MFMA = 8,     /* SpMM with n_rhs == 32 only: 16-row tiles on the matrix cores
                             (v_mfma_f32_16x16x4_f32, four terms per step), one fused
                             multiply-add per term: within the sum|terms| bound, not
                             bit-identical; X must be finite (a non-finite X row makes
                             the tile's other outputs NaN).  X and the term arrays under
                             4 GiB (n_cols * ldx * 4 and nnz * 4 bytes, each below
                             0xFFFFFFF0).  SM_ERR_NOT_SUPPORTED otherwise, for other
                             shapes and for SpMV.                                      */
    SM_ALGO_MERGE = 9     /* SpMV by merge path (Merrill & Garland): every workgroup and
                             thread an equal share of rows + terms, rows cut anywhere.
                             A row inside one thread's share is summed in stored order
                             (bit-identical); cut rows join their parts in a fixed order
                             (within the sum|terms| bound, deterministic).  SpMM: as AUTO. */
} sm_algo;

/* Rows with at most this many terms are summed in reference order by the
 * fast kernels (bit-exact); longer rows use a tree reduction. */
#define SM_SERIAL_ROW_MAX 64

typedef struct sm_matrix sm_matrix;   /* opaque, device-resident */
typedef void *sm_stream;              /* hipStream_t */

typedef struct sm_info {
    int64_t s_rows, s_cols;     /* reference S view: rows_ = k, cols_ = n      */
    int64_t n_rows, n_cols;     /* CSR of B = S^T: n rows, k columns          */
    int64_t nnz;                /* stored entries (explicit zeros included)    */
    int32_t table_size;         /* codebook size T (0 if built from CSR values) */
    int32_t has_ref_stream;     /* 1 if the reference encoding is held         */
    int64_t n_entries;          /* reference stream length (nnz + fillers)     */
    int64_t n_panels;           /* reference panels (block_bounds_.size())     */
    int32_t device;             /* HIP device ordinal holding the matrix       */
    int32_t n_tiles;            /* stream-kernel row tiles                     */
    int32_t n_long_rows;        /* rows split across workgroups                */
    int32_t max_row_nnz;        /* longest row                                 */
    int32_t has_xband;          /* column-band layout: 0 none, 1 exact (bit-identical),
                                   2 blocked, 3 gather, 4 band2 (balanced bands),
                                   5 cband (balanced bands, codebook words),
                                   6 gcb (gathered chunk bands);
                                   2-6 sum each column slab in the reference's
                                   order and add the slab sums in slab order     */
    int32_t xband_blocks, xband_bands;
    int32_t xband_slabs;        /* column slabs per row block (1: bit-identical) */
    int32_t xband_block_rows;   /* rows per block                              */
    int64_t device_bytes;       /* device memory held by the matrix            */
    int32_t col_relabel;        /* 1: the stream SpMV gathers x through a column
                                   relabeling by descending degree (skewed graphs) */
    int32_t xband_slab_cols;    /* columns per slab (slab s = [s*c, (s+1)*c))   */
    int64_t sell_slices;        /* sorted sliced-ELL slices of 64 rows (0: not built) */
    int32_t sell_codebook;      /* 1: the slices hold 4-byte column | codebook-id words */
    int32_t ccsell_chunks;      /* column chunks of the column-chunked sliced ELL (0: not built);
                                   it serves SpMV when built (AUTO, SELL): every row bit-identical */
    int32_t hot_cols;           /* > 0: the relabeled columns [0, hot_cols) run as codebook bands
                                   before the sliced ELL adds the other terms (AUTO, SELL)  */
    int32_t sweep_blocks;       /* row blocks of the column-swept layout (0: not built); it
                                   serves SpMV when built (AUTO): every row bit-identical    */
    int64_t exact_sell_slices;  /* slices of the unsegmented sliced ELL (sm_build_opts.exact_sell;
                                   0: not built) that SM_ALGO_EXACT runs                   */
    int32_t exact_algo;         /* the sm_algo SM_ALGO_EXACT runs for a 16-byte aligned x
                                   (SM_ALGO_SELL also for the unsegmented sliced ELL)       */
    int32_t xband_slab0_cols;   /* columns of slab 0 (slab s >= 1 covers [slab0 + (s-1) *
                                   xband_slab_cols, slab0 + s * xband_slab_cols)); equal to
                                   xband_slab_cols when the slabs are even                  */
    int32_t merge_stage;        /* 1: SM_ALGO_MERGE stages terms from the column-sorted copy
                                   (sm_build_opts.merge_stage)                               */
    int32_t xband_beta_last;    /* 1: the slab sums are added after beta*y -- y = (((beta*y +
                                   P_0) + P_1) + ...), every P_s summed from -0.0 (band2 / cband
                                   with several slabs); 0: slab 0 starts from beta*y          */
    int32_t updatable;          /* 1: built with sm_build_opts.updatable (sm_set_values,
                                   sm_axpy_values apply)                                     */
    int32_t table_updatable;    /* 1: a table matrix built with sm_build_opts.table_updatable
                                   (sm_set_table, sm_axpy_table apply)                       */
} sm_info;

/* ---- library ----------------------------------------------------------- */
SM_API const char *sm_version(void);
SM_API const char *sm_status_string(sm_status s);
SM_API const char *sm_last_error(void);
SM_API sm_status sm_device_count(int32_t *count);

/* ---- construction ---------------------------------------------------------
 * sm_create_from_dense_index: replaces SparseMatrix::CopyForm
 * (sparse-matrix.cc:20-99; ctor sparse-matrix.h:29-31).  `index` is a
 * rows x stride uint8 matrix of codebook ids; ids >= table_size are empty.
 * NoTrans: S = index (rows x cols).  Trans: S = index^T (cols x rows).
 * table_size must be in [0, 255]; 0 yields an empty 0 x 0 matrix
 * (sparse-matrix.cc:25-26).  Host pointers; the CSR is uploaded to `device`. */
SM_API sm_status sm_create_from_dense_index(const uint8_t *index, int32_t rows, int32_t cols,
                                            int32_t stride, const float *table,
                                            int32_t table_size, sm_trans trans,
                                            int32_t device, sm_matrix **out);

/* Same as sm_create_from_dense_index with the index already on `device`
 * (`d_index`, rows x stride bytes; `table` stays a host pointer): the scan runs
 * on the device (count, host prefix sum, fill) and yields
 * the same CSR bit for bit.  No reference stream is kept, so sm_copy_ref_stream
 * does not apply.  Synchronises `stream`. */
SM_API sm_status sm_create_from_dense_index_device(const uint8_t *d_index, int32_t rows,
                                                   int32_t cols, int32_t stride,
                                                   const float *table, int32_t table_size,
                                                   sm_trans trans, int32_t device,
                                                   sm_stream stream, sm_matrix **out);

/* Additive CSR ingestion (no reference equivalent: the reference cannot encode
 * the north-star sizes).  B is n_rows x n_cols; row_ptr has
 * n_rows+1 entries.  Host pointers, validated on the host.
 *
 * Rows: a row may hold its columns in any order and may repeat a column; B is the sum of
 * its stored terms, and "the reference's order" for such a row is its stored order.
 * The layouts that need a row's columns ascending (the band kinds exact, blocked, gather,
 * band2, cband, gcb; the column sweep; the column-chunked sliced ELL) are not built for a
 * matrix with a descending step in a row, forced or not: a forced one leaves
 * sm_info.has_xband == 0, sweep_blocks == 0, ccsell_chunks == 0, and the matrix is served by
 * the layouts that remain (sliced ELL, merge, the CSR kernels), within the same bound.
 * Of these only exact, blocked and gather take a row whose columns ascend with repeats; the
 * others need strictly ascending columns and are not built for it either.  sm_to_dense keeps the last stored of several
 * repeats; sm_build_ref_stream refuses a matrix with a repeated (row, column). */
SM_API sm_status sm_create_from_csr(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                    const int32_t *row_ptr, const int32_t *col_idx,
                                    const float *val, int32_t device, sm_matrix **out);

/* Same, from device pointers on `device` (copied device-to-device on `stream`
 * and validated by a kernel; synchronises `stream`).  The column relabeling, the sorted
 * sliced ELL, the gathered chunk bands, the balanced bands (band2, cband) and the merge
 * staging copy are built on the device from the device CSR (sm_build_opts.host_build,
 * sm_built_on_device).  The other layouts are built on the host: for them the columns (and,
 * for a layout that stores them, the values) are copied to the host once, at creation --
 * 4 + 4 bytes per term over PCIe. */
SM_API sm_status sm_create_from_csr_device(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                           const int32_t *d_row_ptr, const int32_t *d_col_idx,
                                           const float *d_val, int32_t device, sm_stream stream,
                                           sm_matrix **out);

/* ---- layout options ---------------------------------------------------------
 * The constructors pick the SpMV layout themselves (SM_LAYOUT_AUTO).
 * sm_create_from_csr_ex / _device_ex take these options instead, to force a layout
 * (tests, A/B measurements).  Every layout computes the same product; they differ
 * in speed and in where the bit-exact reference order holds (sm_info.has_xband).
 * Fields past `struct_size` keep their defaults, so callers built against an
 * older header stay valid.  Initialise with sm_build_opts_init. */
typedef enum sm_layout {
    SM_LAYOUT_AUTO = 0,      /* cost model: balanced codebook bands / bands / sell / stream */
    SM_LAYOUT_EXACT = 1,     /* column bands, one slab: every row in the reference's order */
    SM_LAYOUT_BLOCKED = 2,   /* column bands in slabs (x staged through LDS)               */
    SM_LAYOUT_GATHER = 3,    /* column-ordered bands, x gathered                           */
    SM_LAYOUT_BAND2 = 4,     /* balanced bands, 8-byte entries                             */
    SM_LAYOUT_CBAND = 5,     /* balanced bands, 4-byte codebook words                      */
    SM_LAYOUT_NO_BANDS = 6,  /* no band layout: sorted sliced-ELL, else the stream kernel   */
    SM_LAYOUT_BANDS = 7,     /* a band layout even where the cost model would decline; the
                                kind as AUTO would pick it                                */
    SM_LAYOUT_SWEEP = 8,     /* column-swept row blocks (wide matrices, <= 255 values): one
                                wavefront per 256 rows, terms in column order, no barrier  */
    SM_LAYOUT_GCB = 9        /* gathered chunk bands (wide matrices, x far beyond L2): 32K-row
                                tiles, bands of up to 2016 terms within 2^18 columns, x
                                gathered per term, rows' sums in LDS                      */
} sm_layout;

typedef struct sm_build_opts {
    int32_t struct_size;       /* sizeof(sm_build_opts) as the caller compiled it      */
    int32_t layout;            /* sm_layout                                            */
    int32_t band_slabs;        /* balanced bands: column slabs per row block, 0 = auto  */
    int32_t band_tall;         /* balanced-band geometry: 0 or 4 = dma3 (a loader wave
                                  stages x by LDS-DMA into three 7680-column buffers; the
                                  default), 6 = wide (8192-column windows staged by every
                                  wave); other values are SM_ERR_INVALID_ARG            */
    int32_t gather_band_log2;  /* gather bands: 13, 14 or 15 (log2 columns), 0 = auto  */
    int32_t sell;              /* sorted sliced-ELL: -1 auto (built when no band layout), 0 never */
    int32_t sell_codebook;     /* sell slots as column|id words: -1 auto, 0 never      */
    int32_t sell_max_len;      /* rows longer than this are cut in segments, 0 = 2048  */
    int32_t sell_streams;      /* XCD streams of sort windows, 0 = auto                */
    int64_t sell_sigma;        /* sort rows by length within windows of this many rows, 0 = globally */
    int32_t relabel;           /* column relabeling by degree: -1 auto, 0 never, 1 always */
    int32_t tile_nnz;          /* stream-kernel tile: 1024/2048/4096/8192 terms; 0 = auto: 4096, or
                                  2048 when the longest row exceeds 64 x the mean row length;
                                  any other value is SM_ERR_INVALID_ARG.  A tile takes rows, in
                                  order, while it holds <= tile_nnz terms and <= 1024 rows
                                  (sm_info.n_tiles); a row of more than tile_nnz terms is a long
                                  row, summed in chunks across workgroups (sm_info.n_long_rows).
                                  The size therefore changes SM_ALGO_STREAM's bits for the rows
                                  longer than one size and not the other (see SM_ALGO_STREAM)  */
    int32_t ccsell;            /* column-chunked sliced-ELL (wide x): -1 auto, 0 never, 1 always
                                  (where no band layout is built and it applies)       */
    int32_t ccsell_chunk_log2; /* its column chunk, log2 columns (8..24), 0 = 20 (4 MiB of x) */
    int32_t hot_cols;          /* skewed graphs (column relabeling built), opt-in: > 0 sends the
                                  hottest this many relabeled columns through codebook bands
                                  with x in LDS, the rest through the sliced ELL (within the
                                  Sum|terms| bound); 0 / -1 never (slower on R-MAT 24)     */
    int32_t exact_sell;        /* an unsegmented sorted sliced ELL beside the layout above, for
                                  SM_ALGO_EXACT when no built layout keeps the reference's order
                                  for every row: 0 auto (matrices from the dense index, i.e.
                                  the reference's CopyForm path), 1 always, -1 never        */
    int32_t band_slab0_permille; /* balanced bands with several slabs: slab 0's columns as a
                                  share of an even split, in permille (0 = auto = 1000, even
                                  slabs); the other slabs share the rest evenly.  The slab-0
                                  tile also loads and scales y before its first band        */
    int32_t merge_stage;       /* SM_ALGO_MERGE on skewed graphs: 1 builds a column-sorted copy of
                                  each merge tile's terms (4-byte column | codebook-id words and
                                  2-byte slots, 6 bytes per term) when the values form a codebook
                                  and n_cols <= 2^24; the tile gathers x in column order (R-MAT 24:
                                  1.91 -> 1.68 ms), same bits as without.  0 = never (default)  */
    int32_t host_build;        /* sm_create_from_csr_device, sm_create_transpose: 0 = auto -- the
                                  column relabeling and the sorted sliced ELL are built on the
                                  device where they are the only layouts wanted, the gathered
                                  chunk bands and the balanced bands (band2, cband) where they are
                                  the band kind (builddev*.hip; the same bytes as the host
                                  builders, sm_layout_digest; sm_built_on_device tells which ran);
                                  1 = always on the host.  updatable and table_updatable matrices,
                                  hot_cols and the column sweep keep the host builders: their
                                  slot -> term maps and given ids are not built on the device  */
    int32_t updatable;         /* 1: the stored values can be replaced in place (sm_set_values,
                                  sm_axpy_values).  No layout decision then reads the values: the
                                  matrix is built as if they took more than 255 bit patterns --
                                  AUTO / SM_LAYOUT_BANDS take band2's 8-byte entries where they
                                  would take cband, the sliced ELL and the column-chunked ELL their
                                  plain form -- and every layout that holds its own copy of the
                                  values also keeps a slot -> term map on the device (4 bytes per
                                  value slot, counted in sm_info.device_bytes).  What exists only
                                  in codebook form is SM_ERR_INVALID_ARG with it: SM_LAYOUT_CBAND,
                                  SM_LAYOUT_SWEEP, hot_cols > 0, merge_stage = 1.  The layouts are
                                  built by the host builders (as host_build = 1: the device
                                  builders emit no maps).  sm_build_ref_stream is
                                  SM_ERR_NOT_SUPPORTED on such a matrix (the stream would go
                                  stale), so SM_ALGO_NATIVE stays unavailable.  0 (default):
                                  nothing changes -- the same layouts, bytes and digests       */
    int32_t table_updatable;   /* 1: the table of a table matrix (sm_create_from_csr_ids, its
                                  _device form, sm_create_quantized, and
                                  sm_create_transpose of one) can be replaced in place
                                  (sm_set_table, sm_axpy_table).  Every layout that holds values
                                  then takes its codebook form with the GIVEN ids and the GIVEN
                                  table -- T entries in the given order, equal entries apart, unused
                                  entries kept -- so no layout decision reads the values and a new
                                  table reaches every layout by rewriting its table copy alone.
                                  AUTO / SM_LAYOUT_BANDS choose among the codebook forms only (cband,
                                  the sliced ELLs' and the column-chunked ELL's codebook form,
                                  SM_LAYOUT_SWEEP when forced); where none applies (the sliced ELL
                                  past 2^24 columns) none is built and the CSR kernels serve.
                                  SM_ERR_INVALID_ARG with it: SM_LAYOUT_EXACT / BLOCKED / GATHER /
                                  BAND2 / GCB (plain form only), sell_codebook = 0, hot_cols > 0,
                                  merge_stage = 1, updatable = 1, and every constructor but the two
                                  above.  Host builders only, and no sm_build_ref_stream
                                  (SM_ERR_NOT_SUPPORTED), as for `updatable`.  0 (default): nothing
                                  changes                                                     */
} sm_build_opts;

SM_API void sm_build_opts_init(sm_build_opts *opts);

SM_API sm_status sm_create_from_csr_ex(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                       const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *val, int32_t device,
                                       const sm_build_opts *opts, sm_matrix **out);
SM_API sm_status sm_create_from_csr_device_ex(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                              const int32_t *d_row_ptr, const int32_t *d_col_idx,
                                              const float *d_val, int32_t device,
                                              sm_stream stream, const sm_build_opts *opts,
                                              sm_matrix **out);

/* A new matrix holding B^T of `src` (n_cols x n_rows; the reference view S^T: s_rows/s_cols
 * swapped), transposed on src's device from its device CSR; layouts per `opts` (NULL: as the
 * constructors choose).  Synchronises `stream`.  `src` is only read: concurrent products on
 * it are fine.
 * Row c of B^T holds the terms of column c of B by ascending source row, equal rows in stored
 * order (a stable sort by column); values bit for bit.  The result is an ordinary matrix (every
 * algorithm and layout; it holds a second copy of the terms).  A source built from the dense
 * index hands on its codebook and the dense-index constructors' default options, so the result
 * is what CopyForm builds from the same index with the other `trans`; no reference stream is
 * kept (sm_build_ref_stream adds it; given the source's codebook it uses the ids the index gave
 * the terms, which the result keeps at one byte per term -- equal codebook entries stay apart,
 * the stream is the reference's own byte for byte).  Scratch while building: 24 bytes per term.
 * A dense-index source costs more: its ids are read back from its reference stream on the host
 * (one O(nnz) walk, a row_ptr download, an id upload) and sorted in a second pass of the same
 * kernels, 32 bytes of scratch per term (+ 1 for the source's ids).
 * opts->updatable = 1: the result is updatable and also keeps, per term, the term's CSR index in
 * `src` (int32, nnz entries; one more pass of the same sort), so values given in src's order
 * update it too (sm_set_values with SM_VALUES_SOURCE); `src` itself need not be updatable.  A
 * dense-index source is SM_ERR_NOT_SUPPORTED with it: its values are its codebook. */
SM_API sm_status sm_create_transpose(const sm_matrix *src, const sm_build_opts *opts,
                                     sm_stream stream, sm_matrix **out);

/* A table matrix: the terms of B as (row, col, id) plus one table of T <= 255 floats, the stored
 * value of term e being table[ids[e]] bit for bit (weight-shared values: quantised centroids).
 * Host pointers; ids has nnz bytes in CSR order.  table_size must be in [1, 255] when nnz > 0
 * (SM_ERR_INVALID_ARG otherwise); an id >= table_size is SM_ERR_INVALID_MATRIX.
 * Without opts->table_updatable the matrix is exactly what sm_create_from_csr_ex builds from the
 * expanded values (same layouts, digests and products); it only remembers, on the device, the ids
 * (nnz bytes) and the table, and holds the scratch of sm_sddmm_table (ceil(nnz / 2048) * 256
 * floats) -- all counted in sm_info.device_bytes.  sm_info.table_size reports T.
 * The device copy of the table is the authoritative one (sm_set_table / sm_axpy_table are
 * asynchronous); sm_copy_table_device reads it.  sm_create_transpose of a table matrix gives a
 * table matrix (the ids travel with the terms, the table is the source's current one) and
 * honours opts->table_updatable.
 * Dense-index (CopyForm) matrices are not table matrices: every call of this family returns
 * SM_ERR_NOT_SUPPORTED on them (INTEGRATION.md shows how to turn an index and its table into
 * (row_ptr, col_idx, ids, table) for this constructor). */
SM_API sm_status sm_create_from_csr_ids(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                        const int32_t *row_ptr, const int32_t *col_idx,
                                        const uint8_t *ids, const float *table, int32_t table_size,
                                        int32_t device, const sm_build_opts *opts /* NULL: defaults */,
                                        sm_matrix **out);
/* sm_create_from_csr_ids from device pointers on `device` (all five arrays; ids of any alignment):
 * the CSR arrays are copied device to device on `stream`, one kernel writes the stored values
 * val[e] = table[ids[e]] (a bit copy) and finds an id >= table_size (SM_ERR_INVALID_MATRIX), the
 * ids and the table are copied device to device, and the tail of sm_create_from_csr_device_ex
 * validates the CSR and builds the layouts.  Synchronises `stream`.  The argument checks are the
 * host constructor's and run before any device work; in addition opts->updatable = 1 is
 * SM_ERR_INVALID_ARG here (a table matrix takes new values through its table).
 * The result is the matrix sm_create_from_csr_ids builds from the same arrays on the host with the
 * same options: sm_equal, sm_layout_digest, sm_info (device_bytes aside), every product of every
 * sm_algo, sm_copy_table_device and sm_copy_term_ids_device, bit for bit.
 * Without opts->table_updatable the layouts are built where sm_create_from_csr_device_ex builds
 * them from the expanded values (the device builders where they apply; sm_built_on_device reports
 * the same mask).  With opts->table_updatable = 1 the host builders are needed and take the given
 * ids and table: the ids (1 byte per term) and the table are copied to the host once, at
 * creation; the other layouts' downloads are those of sm_create_from_csr_device. */
SM_API sm_status sm_create_from_csr_ids_device(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                               const int32_t *d_row_ptr, const int32_t *d_col_idx,
                                               const uint8_t *d_ids, const float *d_table,
                                               int32_t table_size, int32_t device, sm_stream stream,
                                               const sm_build_opts *opts /* NULL: defaults */,
                                               sm_matrix **out);

/* ---- quantising the stored values: 1-D k-means (Lloyd) on the device ---------------------------
 * The "quantise" step of prune -> quantise -> fine-tune: from the stored fp32 values of any matrix
 * (m->d_val in CSR order, whatever constructor made it) to an (ids, table) pair with T <= 255
 * entries, and from there to a table matrix.  The matrix is only read.  The two step calls
 * allocate their own scratch and synchronise `stream`: they are not meant for graph capture.
 * table_size must be in [1, 255] (SM_ERR_INVALID_ARG, checked before the matrix is looked at).
 *
 * sm_quantize_assign: ids[e] = the nearest entry of `table` (T floats on the device, any 4-byte
 * alignment) to val[e]; d_ids: nnz bytes on the device, any alignment; nothing outside
 * ids[0, nnz) is written.  nnz == 0 launches nothing.  The rule, in this order:
 *   1. The candidates are formed from the table: NaN entries are dropped; the rest are compared
 *      as floats, so -0.0 = +0.0; each distinct value is represented by its lowest t.
 *   2. For a value v, lo is the greatest candidate <= v and hi the least candidate > v.
 *   3. If only one of them exists, it is chosen.
 *   4. If both exist, dl = fl32(v - lo) and dh = fl32(hi - v).  lo is chosen, unless dh < dl, or
 *      dh == dl and t_hi < t_lo.
 *   5. A NaN v, or a table with no candidate at all, gives id 0.
 * This is the real-number nearest entry whenever the two distances differ by more than one fp32
 * rounding (each of dl, dh carries at most one); nearer than that, either neighbour may be chosen
 * -- always the same one.
 *
 * sm_quantize_update: one Lloyd update from given ids, table[t] <- the mean of the values with id
 * t.  d_ids: nnz bytes, any alignment; d_table: T floats, in: the old table, out: the new one;
 * d_counts: T int32 or NULL; d_sse: one double (8-byte aligned) or NULL.  Deterministic: no
 * atomics, the launch geometry a function of nnz alone, every operation below one IEEE double
 * operation, round to nearest:
 *   1. Chunk k holds the terms [2048 k, 2048 (k+1)) in CSR order.  p[k][t] = the sum of
 *      (double)val[e] over the chunk's terms with id t, added in ascending e, one add each, from
 *      +0.0; c[k][t] their number.
 *   2. S[t] = p[0][t], p[1][t], ... added in ascending k, one add each, from +0.0; n[t] the sum of
 *      the c[k][t].
 *   3. n[t] > 0: table[t] = (float)(S[t] / (double)n[t]).  Otherwise table[t] keeps its bits: an
 *      empty cluster keeps its entry.
 *   4. counts[t] = n[t].
 *   5. With old_table the table as it was on entry: q[k] = the sum over the chunk's terms of
 *      d * d, d = (double)val[e] - (double)old_table[id_e] (the square rounded once), added in
 *      ascending e from +0.0; sse = q[0], q[1], ... added in ascending k from +0.0.
 * An id >= T is SM_ERR_INVALID_MATRIX, found by the pass and reported after the synchronise (the
 * table, counts and sse hold no meaning then).  nnz == 0: the table is unchanged, counts are 0
 * and sse is 0.0.
 *
 * sm_create_quantized: a new, independent table matrix with src's pattern whose ids and table
 * come from `iters` Lloyd steps on src's stored values; `src` is untouched and may be any matrix
 * (an updatable one is the common case).  iters < 0 is SM_ERR_INVALID_ARG; a stored value that is
 * NaN or Inf is SM_ERR_INVALID_MATRIX (the pass that finds the least and greatest value finds it;
 * it runs also when d_init is given).
 *   Start: d_init (T floats on the device), or NULL for the linear table between lo and hi, the
 *   least and greatest stored value, a zero bound counting as +0.0, computed on the host:
 *     table[t] = (float)((double)lo + ((double)hi - (double)lo) * ((double)t / (double)(T - 1))),
 *     T = 1: table[0] = (float)(((double)lo + (double)hi) / 2).
 *   Steps: `iters` times assign, then update (the kernels of the two calls above, so ids and
 *   table are bit for bit what those calls give, without their allocations and synchronises);
 *   one last assign, so the ids are those of the final table; then sm_create_from_csr_ids_device on src's own device row_ptr / col_idx,
 *   the ids and the table, with `opts` (table_updatable is honoured; updatable = 1 is
 *   SM_ERR_INVALID_ARG).
 * The result may hold fewer distinct values than T (empty clusters keep their entry); nnz == 0
 * gives an empty table matrix with the starting table (all zeros for the linear one).
 * Synchronises `stream`.  Scratch while it runs: 1 byte per term and, with iters > 0, 12 bytes per
 * 2048 terms and table slot (ceil(nnz / 2048) * 256 * 12 bytes). */
SM_API sm_status sm_quantize_assign(const sm_matrix *m, const float *d_table, int32_t table_size,
                                    uint8_t *d_ids, sm_stream stream);
SM_API sm_status sm_quantize_update(const sm_matrix *m, const uint8_t *d_ids, int32_t table_size,
                                    float *d_table /* in: old, out: new */,
                                    int32_t *d_counts /* T, may be NULL */,
                                    double *d_sse /* 1, may be NULL */, sm_stream stream);
SM_API sm_status sm_create_quantized(const sm_matrix *src, int32_t table_size, int32_t iters,
                                     const float *d_init /* T floats on the device, or NULL: linear */,
                                     const sm_build_opts *opts, sm_stream stream, sm_matrix **out);

/* The current table (T floats) / the terms' ids (nnz bytes, CSR order) of a table matrix into
 * buffers on its device, asynchronous on `stream`.  SM_ERR_NOT_SUPPORTED on any other matrix. */
SM_API sm_status sm_copy_table_device(const sm_matrix *m, float *d_table, sm_stream stream);
SM_API sm_status sm_copy_term_ids_device(const sm_matrix *m, uint8_t *d_ids, sm_stream stream);

/* ---- pruning the stored terms by magnitude: mask, compact, rebuild ------------------------------
 * The "prune" step of prune -> quantise -> fine-tune: from the stored fp32 values of any matrix
 * (m->d_val in CSR order, whatever constructor made it) to a mask of the terms to keep, and from a
 * mask to a new matrix that holds the kept terms and remembers where each came from.  The source
 * is only read.  The calls allocate their own scratch and synchronise `stream`: they are not meant
 * for graph capture.
 *
 * The selection rule (sm_prune_mask), on integers only, so that it can be restated bit for bit:
 *   Key.  key(v) = bits(v) & 0x7FFFFFFF, compared as an unsigned integer: -0.0 and +0.0 tie,
 *     subnormals order as their magnitudes, Inf beats every finite value and a NaN has the greatest
 *     keys of all -- it is kept first; the library never drops a NaN weight silently.  Unlike
 *     sm_create_quantized, no stored value is an error here.
 *   SM_PRUNE_GLOBAL_TOPK.  The terms ordered by (key descending, CSR index ascending); the first
 *     min(count, nnz) are kept.  Ties at the cut go to the lower CSR index.
 *   SM_PRUNE_ROW_TOPK.  The same order within every row (ties to the earlier stored position);
 *     the first min(count, row length) of each row are kept.
 *   SM_PRUNE_THRESHOLD.  Term e is kept iff key(val[e]) >= key(threshold).  `count` is ignored.
 *     threshold = 0 keeps every term, explicit zeros included; -0.0 counts as 0.
 * Argument errors, all SM_ERR_INVALID_ARG and checked before the matrix is looked at: an unknown
 *   mode; count < 0 in the two top-k modes; a NaN or negative threshold (but -0.0) in
 *   SM_PRUNE_THRESHOLD (`threshold` is ignored in the other modes); a null `out`.  Then a null
 *   matrix, and a null d_keep with nnz > 0.  count = 0 is legal: an all-zero mask, an empty matrix.
 * d_keep: nnz bytes on the matrix's device at any alignment, keep[e] = 1 or 0; nothing outside
 *   keep[0, nnz) is written.  *kept (host, may be NULL) = the number of ones.  nnz == 0 launches
 *   nothing.
 * Deterministic: the mask is a function of the stored values (and row_ptr) alone.  The kernels use
 *   integer atomics on counters (counts are exact and their order reaches nothing) and no float
 *   arithmetic at all; every launch geometry is a function of nnz and n_rows alone.
 * Scratch: GLOBAL_TOPK 8 bytes per 2048 terms + 4 KiB + hipCUB's scan storage; ROW_TOPK 4 bytes
 *   per row + at most 16 KiB; THRESHOLD at most 8 KiB.
 *
 * sm_create_masked: a new, independent matrix holding the terms of src whose keep[e] != 0, in
 * stored order (d_keep: nnz bytes on src's device, any alignment; NULL only with nnz == 0).  One
 * exclusive scan of the mask over nnz + 1 positions gives every kept term's new index, the new
 * nnz and the new row pointer (new_rp[r] = pos[old_rp[r]]); one kernel scatters the columns, the
 * values (a bit copy) and the source map; then the tail of the device constructors runs, so the
 * layouts, and where the device builders run, are exactly those of sm_create_from_csr_device_ex
 * (a table source: sm_create_from_csr_ids_device) on the compacted arrays with the same `opts`
 * (NULL: defaults): sm_equal, sm_layout_digest, sm_info (device_bytes aside), sm_built_on_device
 * and every product of every sm_algo, bit for bit.  Rows with unsorted or repeated columns pass
 * through in stored order; the layouts that need ascending columns decline them as ever.
 *   A table source (sm_create_from_csr_ids and its kin) gives a table matrix: the ids go through
 *   the same scatter, the table is the source's current one (all table_size entries, also those no
 *   kept term uses), opts->table_updatable is honoured (the ids and the table are copied to the
 *   host once for the host builders) -- as sm_create_transpose hands a table matrix on.
 *   A dense-index (CopyForm) source gives an ordinary CSR matrix of its values: neither the
 *   codebook nor the reference stream is handed on (sm_info.table_size and has_ref_stream are 0).
 *   The source map -- per kept term its CSR index in src, int32, counted in sm_info.device_bytes
 *   -- is always kept: sm_copy_source_terms_device reads it, and with opts->updatable = 1 the
 *   result takes sm_set_values / sm_axpy_values in SM_VALUES_SOURCE order, so values, gradients
 *   and optimiser state laid out for the unpruned matrix can be used as they are.
 * Scratch while building: 4 bytes per term of src + hipCUB's scan storage.
 *
 * sm_create_pruned: sm_prune_mask, then sm_create_masked, the mask (1 more byte per term of
 * scratch) never being the caller's.
 *
 * sm_copy_source_terms_device: for a matrix made by sm_create_masked / sm_create_pruned, and by
 * sm_create_transpose with opts->updatable = 1 (which holds the same map): terms[e] = the CSR
 * index in the source of the matrix's term e.  nnz int32 on the matrix's device, asynchronous on
 * `stream`.  SM_ERR_NOT_SUPPORTED on a matrix that holds no such map. */
typedef enum sm_prune_mode {
    SM_PRUNE_GLOBAL_TOPK = 0,  /* keep the `count` terms of greatest |value| of the whole matrix   */
    SM_PRUNE_ROW_TOPK    = 1,  /* keep, in every row, its `count` terms of greatest |value|         */
    SM_PRUNE_THRESHOLD   = 2   /* keep the terms whose |value| is not below `threshold`             */
} sm_prune_mode;
SM_API sm_status sm_prune_mask(const sm_matrix *m, sm_prune_mode mode, int64_t count, float threshold,
                               uint8_t *d_keep, int64_t *kept /* host, may be NULL */, sm_stream stream);
SM_API sm_status sm_create_masked(const sm_matrix *src, const uint8_t *d_keep, const sm_build_opts *opts,
                                  sm_stream stream, sm_matrix **out);
SM_API sm_status sm_create_pruned(const sm_matrix *src, sm_prune_mode mode, int64_t count, float threshold,
                                  const sm_build_opts *opts, sm_stream stream, sm_matrix **out);
SM_API sm_status sm_copy_source_terms_device(const sm_matrix *m, int32_t *d_terms, sm_stream stream);

/* ---- from dense weights: select and compact on the device ---------------------------------------
 * The entrance of the pipeline: a matrix from a dense fp32 weight matrix on the device, without
 * the caller composing abs / sort / compare / to-CSR, and with the rule stated bit for bit.
 * d_w is B itself, in sm_create_from_csr's orientation: n_rows x n_cols, row-major on `device`,
 * element (r, c) at d_w[r * ld + c], ld >= n_cols (ld is not looked at when n_rows <= 1).  Any
 * 4-byte alignment and any ld are correct; placement only selects the kernel (16-byte loads where
 * d_w is 16-byte aligned and either ld == n_cols or ld and n_cols are multiples of 4).  The
 * padding columns [n_cols, ld) are never read; d_w is never written.
 *
 * The rule is sm_prune_mask's, with no new wording: the dense matrix stands for the full CSR in
 * which every one of its E = n_rows * n_cols elements is a stored term -- term index
 * i = r * n_cols + c, columns ascending, zeros included -- and `mode`, `count`, `threshold` select
 * exactly the terms sm_prune_mask would keep on that matrix: keys are bits & 0x7FFFFFFF, ties go
 * to the lower i, a NaN is kept first.  So SM_PRUNE_THRESHOLD with the smallest subnormal (key 1)
 * keeps exactly the non-zeros, threshold 0 keeps every element, and a top-k whose count exceeds
 * the number of non-zeros keeps zeros, lowest index first.
 *
 * The result is the matrix sm_create_from_csr_device_ex builds from the kept terms (rows with
 * ascending columns, values as bit copies) with the same `opts`: sm_equal, sm_layout_digest,
 * sm_info (device_bytes aside), sm_built_on_device and every product of every sm_algo, bit for
 * bit.  opts->updatable is honoured; opts->table_updatable = 1 is SM_ERR_INVALID_ARG.  No source
 * map is kept (sm_copy_source_terms_device: SM_ERR_NOT_SUPPORTED): a term's origin is its
 * (row, column).  The full matrix, or an E-sized int32 / float copy of it, is never formed.
 *
 * Checks, in this order and before any device work: a null `out`; mode, count and threshold as
 * for sm_prune_mask; n_rows < 0, n_cols < 0, or ld < n_cols with n_rows > 1 (SM_ERR_INVALID_ARG);
 * the options; n_rows or n_cols >= 2^31 - 1, E > 2^32 - 1 (the select's 32-bit bins count every
 * element), or a kept count known in advance -- SM_PRUNE_GLOBAL_TOPK: min(count, E),
 * SM_PRUNE_ROW_TOPK: n_rows * min(count, n_cols) -- past sm_create_from_csr's nnz limit
 * (SM_ERR_TOO_LARGE); a null d_w with E > 0.  SM_PRUNE_THRESHOLD learns its kept count from the
 * count pass and returns SM_ERR_TOO_LARGE there, with nothing leaked.  E = 0: an empty matrix,
 * nothing launched, d_w may be NULL.  count = 0: an empty matrix of the given shape.
 *
 * Deterministic: integers only, integer atomics on counters only, every launch geometry a
 * function of (n_rows, n_cols, the alignment class of d_w and ld).  The call allocates its
 * scratch and synchronises `stream`: it is not for graph capture.
 * Scratch while selecting: a byte mask, 1 byte per dense element (rounded up to 2048), 8 bytes per
 * 2048 elements of chunk counts and bases, 4 KiB of select state + hipCUB's scan storage. */
SM_API sm_status sm_create_from_dense_device(const float *d_w, int64_t n_rows, int64_t n_cols, int64_t ld,
                                             sm_prune_mode mode, int64_t count, float threshold,
                                             int32_t device, sm_stream stream,
                                             const sm_build_opts *opts /* NULL: defaults */, sm_matrix **out);

/* ---- the sum of two matrices: C = alpha A + beta B on the union of their patterns ----------------
 * The one call that puts terms into a held matrix: the csrgeam of a sparse BLAS, the merge of a
 * sparse delta into a sparse weight, and -- as sm_create_sum(A, 1, G, 0) -- the regrow step of
 * dynamic sparse training.  sm_create_sum makes a new, independent matrix C of the operands' shape
 * on their device; `a` and `b` are only read, and a == b is allowed.  The call allocates its own
 * scratch and synchronises `stream`: it is not meant for graph capture.
 *
 * The pattern, on integers only:
 *   Row r of C holds the union of the columns of row r of A and of row r of B, ascending; each
 *   (row, column) is stored once.  A term stays a stored term whatever its value: explicit zeros
 *   of either operand and sums that cancel to 0 are kept.  Nothing is dropped by value.
 * The value of a term of C at (r, c), so that it can be restated bit for bit:
 *   A's contribution is absent if A does not store (r, c) or alpha == 0 -- A's values are then
 *     never read (the library's "alpha == 0 skips" rule: a NaN there does not reach C).  Otherwise
 *     it is pa = a's bits as they are if alpha == 1, and pa = fl(alpha * a) in every other case.
 *   B's contribution pb: the same with beta.
 *   Both present: fl(pa + pb) -- two separately rounded products and one add, never a fused
 *     multiply-add.  One present: its bits.  None present: +0.0.
 *   Subnormals are kept.  A NaN result is a NaN where the rule gives one (Inf - Inf, 0 * Inf, a NaN
 *     operand); its payload is the hardware's.
 *   So sm_create_sum(A, 1, G, 0) is A's values, bit for bit, on the union pattern, the positions
 *   only G stores at +0.0; (1, -1) is A - B; (0, 0) is the union pattern at +0.0.
 * The source maps, always kept and counted in sm_info.device_bytes: for term e of C, terms_a[e] is
 *   the CSR index of that position in A, or -1 where A does not store it; terms_b[e] the same for
 *   B.  sm_copy_sum_terms_device copies them (nnz int32 each, on the matrix's device, asynchronous
 *   on `stream`; either array may be NULL and is then skipped); SM_ERR_NOT_SUPPORTED on a matrix
 *   sm_create_sum did not make; nnz == 0 is SM_OK with nothing launched.  There is no single source
 *   term, so SM_VALUES_SOURCE stays SM_ERR_NOT_SUPPORTED on a sum matrix and
 *   sm_copy_source_terms_device refuses it; state laid out for A is carried with terms_a.
 * The result is the matrix sm_create_from_csr_device_ex builds from the restated (row_ptr, col_idx,
 *   val) with the same `opts` (NULL: defaults): sm_equal, sm_layout_digest, sm_info (device_bytes
 *   aside), sm_built_on_device and every product of every sm_algo, bit for bit.  opts->updatable is
 *   honoured; opts->table_updatable = 1 is SM_ERR_INVALID_ARG.  Table sources and dense-index
 *   (CopyForm) sources contribute their stored values; C is an ordinary CSR matrix
 *   (sm_info.table_size and has_ref_stream are 0).
 * Checks, in this order, the first five before any device work: a null `out`; a null `a` or `b`;
 *   the options; differing n_rows / n_cols or differing devices (SM_ERR_INVALID_ARG); an operand
 *   with a row whose columns do not strictly ascend (SM_ERR_NOT_SUPPORTED, the message names the
 *   operand: such a row has no merge and no single source term).  After the count pass: a union
 *   past sm_create_from_csr's nnz limit (SM_ERR_TOO_LARGE, nothing leaked; the row lengths sum to
 *   at most nnzA + nnzB < 2^32 and are scanned in unsigned 32 bits).
 * Deterministic: the structure is integers only, no atomics at all, every launch geometry a
 *   function of (n_rows, nnzA, nnzB); C is a function of the operands, alpha and beta alone.
 * Scratch while building: 8 bytes per term of A (the match word and its scan), 8 bytes per row
 *   (the lengths and their scan) + hipCUB's scan storage.  B's terms need none. */
SM_API sm_status sm_create_sum(const sm_matrix *a, float alpha, const sm_matrix *b, float beta,
                               const sm_build_opts *opts /* NULL: defaults */, sm_stream stream,
                               sm_matrix **out);
SM_API sm_status sm_copy_sum_terms_device(const sm_matrix *m, int32_t *d_terms_a, int32_t *d_terms_b,
                                          sm_stream stream);   /* either array may be NULL: skipped */

/* Destroy: sparse-matrix.cc:9-18 (frees host and device storage). */
SM_API void sm_destroy(sm_matrix *m);

/* ---- queries ----------------------------------------------------------- */
/* sm_info grew in 0.2 (xband_slab_cols, sell_slices, sell_codebook): a caller built
 * against an older header passes its own sizeof to sm_get_info_ex, which writes only
 * that many bytes.  sm_get_info writes the whole struct of this header. */
SM_API sm_status sm_get_info(const sm_matrix *m, sm_info *info);
SM_API sm_status sm_get_info_ex(const sm_matrix *m, sm_info *info, size_t info_bytes);
/* Diagnostics: 64-bit FNV-1a digests of the device layout arrays, so two builds can be
 * compared byte for byte (sm_build_opts.host_build): [0] the column relabeling (new column
 * of every original column, relabeled col_idx), [1] the sorted sliced ELL's structure
 * (slice offsets and lengths, lane rows and lengths, long rows and their partial offsets),
 * [2] its slots (column words, values), [3] its codebook and the merge path's staging copy
 * (sm_build_opts.merge_stage: column words, offsets, table).  0 for a part not built.  With the
 * gathered chunk bands (SM_LAYOUT_GCB) [1] is their geometry, tile -> band offsets and band
 * start columns, [2] the bands' words.  With the balanced bands (band2, cband) and no sliced
 * ELL beside them [1] is their geometry (block rows, window, blocks, slabs, slab columns),
 * tile -> band offsets and band start columns, [2] the bands' entry words, [3] for cband the
 * layout's copy of the table (256 floats) and its size.  Synchronises the device. */
SM_API sm_status sm_layout_digest(const sm_matrix *m, uint64_t digest[4]);
/* Which layouts of `m` the device builders made (0: all built on the host, or none built). */
#define SM_BUILT_DEV_RELABEL 1u      /* the column relabeling */
#define SM_BUILT_DEV_SELL 2u         /* the sorted sliced ELL */
#define SM_BUILT_DEV_GCB 4u          /* the gathered chunk bands */
#define SM_BUILT_DEV_MERGE_STAGE 8u  /* the merge path's staging copy */
#define SM_BUILT_DEV_BANDS 16u       /* the balanced bands (band2, cband) */
SM_API sm_status sm_built_on_device(const sm_matrix *m, uint32_t *mask);
SM_API int32_t sm_num_rows(const sm_matrix *m);   /* NumRows, sparse-matrix.h:39 */
SM_API int32_t sm_num_cols(const sm_matrix *m);   /* NumCols, sparse-matrix.h:40 */

/* The reference encoding (sparse-matrix.h:46-52): E delta steps and ids, and
 * per panel (row_off, col_off, begin, end).  Sizes from sm_get_info. */
SM_API sm_status sm_copy_ref_stream(const sm_matrix *m, uint8_t *pos, uint8_t *val,
                                    int32_t *panel_row_off, int32_t *panel_col_off,
                                    int64_t *panel_begin, int64_t *panel_end);

/* The reference encoding of a matrix built from CSR (sm_create_from_csr*, or the
 * device CopyForm scan), built on the host from its CSR by the reference's own stream
 * rules (sparse-matrix.cc:20-99: 256-column panels, row-major, uint8 delta steps with
 * (255, T) fillers, uint8 ids): afterwards sm_copy_ref_stream, sm_equal's member-wise
 * comparison and SM_ALGO_NATIVE serve the matrix.  `table` (table_size <= 255 entries)
 * is the codebook every value must match bit for bit (the first equal entry's id);
 * NULL takes the values' distinct bit patterns in CSR order (SM_ERR_NOT_SUPPORTED past
 * 255).  A matrix sm_create_transpose made from a dense-index one, given that one's codebook,
 * uses the ids the index gave the terms instead (equal entries stay apart).
 * A matrix that already holds the encoding is left as it is.  SM_ERR_NOT_SUPPORTED on a matrix
 * built with sm_build_opts.updatable (the stream would go stale), and on a matrix that stores
 * a (row, column) more than once: the reference's format comes from a dense index and cannot
 * hold one (the matrix stays as it was).  Rows with unsorted columns are fine: the encoder
 * sorts.  Not concurrent with
 * other calls on the matrix.  Additive: the reference cannot hold a matrix without it. */
SM_API sm_status sm_build_ref_stream(sm_matrix *m, const float *table, int32_t table_size);

/* Host copy of the device CSR (row_ptr n_rows+1, col_idx/val nnz). */
SM_API sm_status sm_copy_csr(const sm_matrix *m, int32_t *row_ptr, int32_t *col_idx, float *val);

/* Device copy of the device CSR (row_ptr n_rows+1, col_idx / val nnz) into buffers on the
 * matrix's device, asynchronous on `stream`; any of the three pointers may be NULL to skip that
 * array.  With sm_create_from_csr_device it rebuilds a matrix from updated values without a
 * host round trip; a matrix built with sm_build_opts.updatable takes new values in place
 * instead (sm_set_values, sm_axpy_values). */
SM_API sm_status sm_copy_csr_device(const sm_matrix *m, int32_t *d_row_ptr, int32_t *d_col_idx,
                                    float *d_val, sm_stream stream);

/* CopyTo (sparse-matrix.cc:101-137), host output.  NoTrans writes S
 * (s_rows x stride), Trans writes S^T (s_cols x stride); untouched elements
 * are zeroed.  Decoded on the device.  A (row, column) stored more than once gets the value
 * of its last stored term (the products add every one). */
SM_API sm_status sm_to_dense(const sm_matrix *m, float *out, int32_t stride, sm_trans trans);

/* sm_to_dense with a device output: NoTrans writes S (s_rows x s_cols, B transposed), Trans
 * writes S^T = B (n_rows x n_cols), row-major with rows `ld` apart (ld >= the row width, 64-bit).
 * d_out is on the matrix's device at any 4-byte alignment.  Exactly the columns [0, width) of
 * each output row are written -- zeros where B stores nothing; the padding columns [width, ld)
 * and everything outside are untouched (the library's operand rule, not sm_to_dense's whole-stride
 * memset).  A (row, column) stored more than once gets its last stored term's value,
 * deterministically: matrices whose rows all strictly ascend (found when the matrix is made)
 * scatter one thread per term, others one thread per row in stored order.  Asynchronous on
 * `stream`: no allocation, no host synchronisation, no matrix scratch, the matrix only read -- it
 * can be captured in a HIP graph, and calls from several streams need no ordering.  An empty
 * output is SM_OK with nothing launched.  SM_ERR_INVALID_ARG, before any device work: a null
 * matrix, a bad `trans`, a null d_out with a non-empty output, ld < width. */
SM_API sm_status sm_to_dense_device(const sm_matrix *m, float *d_out, int64_t ld, sm_trans trans,
                                    sm_stream stream);

/* operator== (sparse-matrix.cc:197-207) on semantic content: shape, stored
 * (row, col, value) triples and, for codebook matrices, the table. */
SM_API int32_t sm_equal(const sm_matrix *a, const sm_matrix *b);

/* ---- compute on device pointers ----------------------------------------- */
/* y[n_rows] = alpha * B * x[n_cols] + beta * y */
SM_API sm_status sm_spmv(const sm_matrix *m, float alpha, const float *x, float beta, float *y,
                         sm_algo algo, sm_stream stream);

/* Y (n_rows x n_rhs, ldy) = alpha * B * X (n_cols x n_rhs, ldx) + beta * Y */
SM_API sm_status sm_spmm(const sm_matrix *m, int32_t n_rhs, float alpha, const float *X,
                         int64_t ldx, float beta, float *Y, int64_t ldy, sm_algo algo,
                         sm_stream stream);

/* Sampled dense-dense product over the matrix's own pattern (SDDMM), no reference equivalent:
 *   out[e] = alpha * sum_j G[r_e*ldg + j] * X[c_e*ldx + j] + beta * out[e],   0 <= j < n_rhs,
 * for every stored term e = (r_e, c_e) of B in CSR order (the order sm_copy_csr returns).  With
 * G = dL/dY it is dL/dval of Y = alpha * B * X: the gradient of the stored values.
 * Operands: G is n_rows x n_rhs and X is n_cols x n_rhs, both row-major with ldg, ldx >= n_rhs;
 *   `out` has nnz floats and must not overlap G or X.  n_rhs >= 1 (else SM_ERR_INVALID_ARG);
 *   n_rhs = 1 is the SpMV case g[r] * x[c].
 * Terms: the stored entries of the B = S^T CSR, explicit zeros included, whatever constructor
 *   made the matrix.  nnz = 0 returns SM_OK and launches nothing.
 * Placement: any 4-byte aligned G, X, out and any ld is correct; placement only selects the
 *   kernel.  The vector kernel takes 16-byte aligned G and X with ldg % 4 == 0, ldx % 4 == 0
 *   (and n_rhs % 4 == 0, G and X each under 4 GiB); the one-lane-per-term kernel takes everything
 *   else.  Nothing outside out[0, nnz) is written; G and X are never written; row offsets are
 *   formed in 64 bits.
 * beta, alpha: as everywhere in the library.  `out` is multiplied by beta whenever beta != 1 (so
 *   beta = 0 propagates NaN/Inf already in `out`) and added unscaled when beta == 1.  alpha == 0
 *   skips the product: G and X are not read and may be NULL, only the beta scaling runs.
 * SM_ALGO_PARITY: one order, every operation rounded separately (no fused multiply-add):
 *     s = fl(G[r,0] * X[c,0]);   s = fl(s + fl(G[r,j] * X[c,j]))  for j = 1 .. n_rhs-1;
 *     t = fl(alpha * s);   out = fl(out + t) if beta == 1, else fl(fl(beta * out) + t)
 *   -- bit-identical to that restatement for every term (n_rhs + 2 roundings on the longest path).
 * SM_ALGO_AUTO (every other sm_algo value runs as AUTO: the SpMV layouts do not matter here):
 *   deterministic -- the same inputs give the same bits on every run; no float atomics, and the
 *   launch geometry is a function of n_rhs alone.  n_rhs <= 3, or a placement the vector kernel
 *   does not take: the PARITY kernel, bit-identical to PARITY (so n_rhs = 1 always is).
 *   Otherwise the vector kernel: L = min(64, the power of two >= n_rhs / 4) lanes share a term,
 *   lane g owns the elements [4g, 4g+4) + 4L*t, t = 0 .. T-1, T = ceil(n_rhs / 4L); its partial is
 *   one fused multiply-add per element in ascending j (4T roundings), the L partials are added in
 *   a fixed xor tree, lane distances L/2 ... 1 (log2 L roundings), then t = fl(alpha * s) and the
 *   add onto beta * out as above: 4T + log2 L + 2 roundings on the longest path -- 6 at n_rhs = 4,
 *   9 at 32, 12 at 256, 16 at 512.  Every result is within
 *     |out - exact| <= 1e-6 * (|alpha| * sum_j |G*X| + |beta * out_0|)
 *   in the worst case while that count is <= 16 (16 * 2^-24 < 1e-6), i.e. for the vector kernel up
 *   to n_rhs = 512 and for the one-lane-per-term kernel up to n_rhs = 14; past that the bound
 *   holds for all but adversarial data (errors of random sign grow with the square root).
 * Streams: asynchronous on `stream`; no allocation, no host synchronisation and no matrix scratch,
 *   so the call can be captured in a HIP graph, and calls on one matrix from several streams need
 *   no ordering (the matrix is only read). */
SM_API sm_status sm_sddmm(const sm_matrix *m, int32_t n_rhs, float alpha, const float *G, int64_t ldg,
                          const float *X, int64_t ldx, float beta, float *out, sm_algo algo,
                          sm_stream stream);

/* New values for the stored terms, in place (no reference equivalent), for a matrix built with
 * sm_build_opts.updatable = 1 (SM_ERR_NOT_SUPPORTED otherwise):
 *   sm_set_values:   val[e] = v[i], bit for bit (NaN payloads, -0.0, denormals);
 *   sm_axpy_values:  val[e] = fl(val[e] + fl(a * delta[i])) -- two roundings, no fused multiply-add.
 * `order` says how the array is indexed.  SM_VALUES_OWN: i = e, the matrix's own CSR order (the
 * order of sm_copy_csr and of sm_sddmm's `out`).  SM_VALUES_SOURCE: the array is in the CSR order
 * of the matrix this one was made from -- transposed (sm_create_transpose) or pruned
 * (sm_create_masked / sm_create_pruned) -- and term e reads the element of its source term; only
 * on a matrix one of those calls made with opts->updatable = 1 (SM_ERR_NOT_SUPPORTED otherwise).
 * Both orders apply the same roundings to the same operands: after the same call on a matrix
 * and on its transposed companion the two hold the same bits per term.
 * Afterwards the matrix is what sm_create_from_csr_device_ex builds from (row_ptr, col_idx, the
 * new values) with the same options: the CSR values, every layout's slots, sm_layout_digest and
 * every product of every sm_algo, bit for bit.
 * Arrays: device pointers to nnz floats, 4-byte aligned.  A null `m` is SM_ERR_INVALID_ARG, and so
 *   is a null array with nnz > 0 (sm_axpy_values: only when a != 0).  nnz == 0: SM_OK, nothing
 *   launched.  a == 0: SM_OK, nothing launched, `delta` is not read and may be NULL (the
 *   library's "alpha == 0 skips" rule).
 * Streams: asynchronous on `stream`: one kernel for the CSR values and one per layout that holds
 *   its own copy of them.  No allocation, no host synchronisation and no matrix scratch, so the
 *   call can be captured in a HIP graph.  The call WRITES the matrix: the caller orders it against
 *   products of the same matrix on other streams; on one stream the stream's order is enough.
 * The slot -> term maps of device-built layouts are out of scope: an updatable matrix is built by
 *   the host builders. */
typedef enum sm_values_order { SM_VALUES_OWN = 0, SM_VALUES_SOURCE = 1 } sm_values_order;
SM_API sm_status sm_set_values(sm_matrix *m, const float *d_v, sm_values_order order, sm_stream stream);
SM_API sm_status sm_axpy_values(sm_matrix *m, float a, const float *d_delta, sm_values_order order,
                                sm_stream stream);

/* The gradient of the table of a table matrix (sm_create_from_csr_ids with or without
 * table_updatable, and its transposes; SM_ERR_NOT_SUPPORTED on every other matrix):
 *   out[t] = alpha * sum over the terms e with id_e = t of <G[r_e, :], X[c_e, :]> + beta * out[t],
 * t < T -- the sum of sm_sddmm's per-term gradients over the terms that share a table entry,
 * in one fused pass that writes no nnz-sized array.
 * Operands: G, X, ldg, ldx, n_rhs as for sm_sddmm (placement only selects the kernel, row offsets
 *   in 64 bits).  d_out: T floats on the device, any 4-byte alignment, not overlapping G or X.
 * Summation order (deterministic: no float atomics, the launch geometry a function of nnz and
 * n_rhs alone; both algorithms, which differ only in d_e):
 *   1. d_e: the term's dot exactly as sm_sddmm forms s before alpha -- SM_ALGO_PARITY the
 *      separate-roundings order; AUTO (every other value) the vector kernel's order where that
 *      kernel takes the placement, else the PARITY order.  The same device code as sm_sddmm.
 *   2. chunk k holds the terms [2048 k, 2048 (k+1)) in CSR order; p[k][t] = the d_e of the
 *      chunk's terms with id t in ascending e, added one at a time (round to nearest), from -0.0.
 *   3. S[t] = p[0][t], p[1][t], ... in ascending k, added one at a time, from -0.0.
 *   4. out[t] = fl(o + fl(alpha * S[t])), o = out[t] if beta == 1 else fl(beta * out[t]).
 * Longest rounding path of out[t]: R_t = R_dot + max_k |{e in chunk k : id_e = t}| +
 *   ceil(nnz / 2048) + 2, R_dot = sm_sddmm's count for the dot itself (n_rhs for PARITY,
 *   4T + log2 L for the vector kernel), and
 *     |out[t] - exact| <= R_t * 2^-24 * (|alpha| * sum_e sum_j |G*X| over the id's terms + |beta*out_0|)
 *   to first order.
 * alpha == 0 skips the product (G and X may be NULL; only the beta scaling runs).  nnz == 0: the
 *   finish step alone runs with every S[t] = -0.0.  n_rhs < 1 is SM_ERR_INVALID_ARG.
 * Streams: asynchronous on `stream`; no allocation and no host synchronisation.  The per-chunk
 *   partials live in the matrix (allocated at creation): calls on one matrix from any streams
 *   take turns on the device through an event of their own (they do not serialise with SpMVs);
 *   into a stream being captured the stream's own order holds, as for the scratch-using SpMVs. */
SM_API sm_status sm_sddmm_table(const sm_matrix *m, int32_t n_rhs, float alpha, const float *G,
                                int64_t ldg, const float *X, int64_t ldx, float beta, float *d_out,
                                sm_algo algo, sm_stream stream);

/* A new table for a table matrix built with sm_build_opts.table_updatable = 1, in place
 * (SM_ERR_NOT_SUPPORTED otherwise):
 *   sm_set_table:   table[t] = v[t], bit for bit (NaN payloads, -0.0, denormals);
 *   sm_axpy_table:  table[t] = fl(table[t] + fl(a * delta[t])) -- two roundings, no fused multiply-add.
 * Arrays: device pointers to T floats, 4-byte aligned; a null array with T > 0 is
 *   SM_ERR_INVALID_ARG.  a == 0: SM_OK, nothing launched, `delta` may be NULL.
 * The calls write the authoritative table, every layout's own table copy (the zero padding past T
 * of the 256-entry copies included) and the CSR values val[e] = table[ids[e]] (one pass, 1 + 4
 * bytes per term).  Afterwards the matrix is what sm_create_from_csr_ids builds from the same
 * pattern and ids, the new table and the same options: the CSR values, sm_equal, sm_layout_digest
 * and every product of every sm_algo, bit for bit.  A transposed companion takes the same call
 * with the same array (the table has no term order).
 * Streams: asynchronous on `stream`, two launches; no allocation, no host synchronisation, no
 *   scratch, so the calls can be captured.  They WRITE the matrix: ordering as for sm_set_values. */
SM_API sm_status sm_set_table(sm_matrix *m, const float *d_table, sm_stream stream);
SM_API sm_status sm_axpy_table(sm_matrix *m, float a, const float *d_delta, sm_stream stream);

/* AddMatMat (sparse-matrix.cc:139-194) on device pointers:
 * C (m x n, ldc) = alpha * A (m x k, lda) * S + beta * C.
 * m = 1: sm_spmv.  2 <= m <= 128 with algo != SM_ALGO_PARITY: transposes + row-panel
 * SpMM in the matrix's workspace, asynchronous on `stream`: the stream first waits on
 * an event recorded after the previous call's last use of the workspace (calls from
 * any streams take turns on the device; the host blocks only when a larger m makes
 * the workspace grow); m > 128: the same per group of 128 rows of A and C.
 * SM_ALGO_PARITY: one thread per output reads A and C in place. */
SM_API sm_status sm_addmatmat(const sm_matrix *mat, const float *a, int32_t m, int32_t lda,
                              float *c, int32_t ldc, float alpha, float beta, sm_algo algo,
                              sm_stream stream);

/* Synchronous drop-in for AddMatMat on HOST pointers (uploads A and C, computes with
 * SM_ALGO_EXACT, downloads C).  Bit-identical to the reference. */
SM_API sm_status sm_addmatmat_host(const sm_matrix *mat, const float *a, int32_t m, int32_t lda,
                                   float *c, int32_t ldc, float alpha, float beta);

/* ---- kernel.h helpers (kernel.cc:10-187), device pointers ---------------- */
/* c[i*ldc + j] *= beta for i < m, j < n */
SM_API sm_status sm_beta_scale(float *c, int32_t m, int32_t n, int32_t ldc, float beta,
                               sm_stream stream);
/* sa[j*ldsa + i] = a[i*lda + j] for i < m, j < n (out of place) */
SM_API sm_status sm_transpose(const float *a, int32_t m, int32_t n, int32_t lda, float *sa,
                              int32_t ldsa, sm_stream stream);

/* ---- reference-format panel kernels (kernel.h:42-62), device pointers -----
 * One panel of the reference stream (ppos/pval, pos_len entries; positions
 * are row*256 + col inside the panel), codebook `table` of valid_table_size+1
 * floats.  variant: 0 = sblas_kernel_operation, 1 = _naive (A m x k lda,
 * C m x n ldc), 2 = _trans, 3 = _trans_ex (A^T k x lda, C^T n x ldc). */
SM_API sm_status sm_panel_kernel(int32_t variant, int32_t m, int32_t n, int32_t k,
                                 const float *a, int32_t lda, float *c, int32_t ldc, float alpha,
                                 const uint8_t *ppos, const uint8_t *pval, int32_t pos_len,
                                 const float *table, int32_t valid_table_size, sm_stream stream);

/* Synchronise the stream and report asynchronous kernel errors. */
SM_API sm_status sm_stream_sync(sm_stream stream);

/* Testing hook: set the slab hand-off launch counter of every row block of a band2 /
 * cband layout (xband_dev.h, 64-bit, monotonic) to `started` and clear its arrival
 * words, as if `started` tiles had run before -- e.g. 2^32 - 1 to run launches across
 * the 32-bit boundary.  Synchronous; no SpMV on the matrix may be in flight.
 * SM_ERR_NOT_SUPPORTED when the matrix has no multi-slab band2 / cband layout, or when
 * `started` is not a whole number of launches (a multiple of the slab count). */
SM_API sm_status sm_debug_seed_handoff(sm_matrix *m, uint64_t started);

/* ---- multi-GPU: row partition + one RCCL all-gather per product ------------
 * SURVEY.md §8(e).  One process per GPU of one node.  Rank r holds its rows of B
 * (any contiguous split; sm_multi_partition gives the equal one) as an sm_matrix with
 * GLOBAL column indices, so its n_cols is the global column count.  x is split in
 * nranks equal slices (n_cols % nranks == 0): rank r supplies x[r*L, (r+1)*L),
 * L = n_cols / nranks.  Per product the only exchange is one ncclAllGather of the x
 * slices (SpMM: of the X panel's row slices) over xGMI into the context's buffer,
 * then the local SpMV / SpMM on the same stream.  No other collective: the reference's
 * panels already write disjoint outputs (sparse-matrix.cc:164-190).
 * RCCL is loaded at run time (the copy already in the process if any, else
 * $SM_RCCL_LIB if set, else the system's); without it sm_multi_create returns
 * SM_ERR_NOT_SUPPORTED (sm_multi_create_with takes any all-gather instead).
 * Errors: sm_multi_last_error(). */
#define SM_UNIQUE_ID_BYTES 128
typedef struct sm_unique_id { char internal[SM_UNIQUE_ID_BYTES]; } sm_unique_id;
typedef struct sm_multi sm_multi;

SM_API const char *sm_multi_last_error(void);
/* Rows [r0, r1) of rank `rank` in the equal split of n rows (the first n % nranks ranks
 * get one row more).  Pure arithmetic, no device. */
SM_API sm_status sm_multi_partition(int64_t n, int32_t nranks, int32_t rank, int64_t *r0,
                                    int64_t *r1);
/* Rank 0 creates the id and passes it to every rank out of band (MPI, a file,
 * torch.distributed). */
SM_API sm_status sm_multi_unique_id(sm_unique_id *id);
/* Collective: every rank calls it with the same id and nranks.  The context refers to
 * `local` (not owned; keep it alive) and joins the communicator on its device. */
SM_API sm_status sm_multi_create(const sm_unique_id *id, int32_t nranks, int32_t rank,
                                 const sm_matrix *local, sm_multi **out);
/* A caller-supplied all-gather instead of RCCL (no reference equivalent: the reference
 * has no multi-device path).  `allgather` gathers `count` floats from every rank's
 * `send` into `recv` in rank order (rank r's slice at recv + r*count), ordered on
 * `stream` (a hipStream_t): it may enqueue device work on `stream`, or synchronise
 * `stream` and block the host until `recv` holds the result (a host-staged gather over
 * MPI, gloo, ...).  It returns 0 on success.  Everything else -- the partition, the two
 * gather buffers, their stream ordering, the pipelined batch -- is the context's, as
 * with RCCL.  sm_multi_unique_id is not needed. */
typedef int32_t (*sm_allgather_fn)(const float *send, float *recv, int64_t count,
                                   sm_stream stream, void *user);
typedef struct sm_collective {
    sm_allgather_fn allgather;
    void *user;   /* passed back to every call */
} sm_collective;
SM_API sm_status sm_multi_create_with(const sm_collective *coll, int32_t nranks, int32_t rank,
                                      const sm_matrix *local, sm_multi **out);
SM_API void sm_multi_destroy(sm_multi *mc);
/* y_local = alpha * B_local * x + beta * y_local, x = all-gather of the x_local slices. */
SM_API sm_status sm_multi_spmv(sm_multi *mc, float alpha, const float *x_local, float beta,
                               float *y_local, sm_algo algo, sm_stream stream);
/* Y_local (rows x n_rhs, ldy) = alpha * B_local * X + beta * Y_local; X_local is this
 * rank's L x n_rhs row-major slice of X (contiguous, ldx = n_rhs). */
SM_API sm_status sm_multi_spmm(sm_multi *mc, int32_t n_rhs, float alpha, const float *X_local,
                               float beta, float *Y_local, int64_t ldy, sm_algo algo,
                               sm_stream stream);
/* `count` independent products y_local[i] = alpha * B_i * x + beta * y_local[i], x the
 * all-gather of x_local[i], B_i = locals[i] (NULL: the context's matrix; others must
 * have the same global columns and device): the all-gather of product i+1 runs on the
 * context's own stream beside the SpMV of product i on `stream` (two gather buffers
 * alternate); still one all-gather per product.  Returns with the whole batch ordered
 * before later work on `stream`. */
SM_API sm_status sm_multi_spmv_batch(sm_multi *mc, int32_t count, const sm_matrix *const *locals,
                                     float alpha, const float *const *x_local, float beta,
                                     float *const *y_local, sm_algo algo, sm_stream stream);
/* The all-gather alone (n_rhs = 1 for x), into the context's buffer; *x_full (optional)
 * receives its device address, valid until the next call on the context (which waits
 * for the work queued on `stream` up to this call, not for reads the caller adds later
 * on other streams).
 * Buffer ordering: every product records, on the stream that ran it, that it has read
 * the gathered x; any later all-gather into that buffer waits for it, from whatever
 * stream.  Calls on one context therefore may come from several streams.  Inside a
 * stream capture, the captured products are ordered by the capture only: a graph replay
 * is not tracked, so the caller orders replays of captured products against eager calls
 * on other streams (an event after each replay).  A capture cannot grow the gather
 * buffers (that needs a device sync): a captured product larger than every earlier one
 * fails with SM_ERR_NOT_SUPPORTED -- run one eager product of that size first. */
SM_API sm_status sm_multi_allgather(sm_multi *mc, const float *x_local, int32_t n_rhs,
                                    sm_stream stream, const float **x_full);
/* Device timing of sm_multi_spmv / _spmm (HIP events around the all-gather and the
 * local product); sm_multi_last_times waits for the last call and reports both. */
SM_API sm_status sm_multi_set_timing(sm_multi *mc, int32_t on);
SM_API sm_status sm_multi_last_times(sm_multi *mc, float *allgather_ms, float *compute_ms);

#ifdef __cplusplus
}
#endif
#endif /* SPARSEMATRIX_AMD_H */
