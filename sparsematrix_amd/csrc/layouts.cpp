// layouts.cpp -- what decides and builds a matrix's layouts, on the host side: the resolved
// options, the cost models, the want_* decisions (each reads what was built before it, so their
// order is significant), the upload_* builders and the two tails the constructors of create.cpp
// end in.  The device builders are builddev.hip and builddev_gcb.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "capi_util.h"
#include "ccsell.h"
#include "sweep.h"
#include "encode.h"
#include "gcb.h"
#include "sm_internal.h"
#include "sell.h"
#include "xband.h"

namespace smamd {

BuildOpts resolve_opts(const sm_build_opts *o) {
    BuildOpts r;
    sm_build_opts_init(&r);
    if (o) memcpy(&r, o, std::min<size_t>(sizeof(r), (size_t)std::max<int32_t>(o->struct_size, 0)));
    r.struct_size = (int32_t)sizeof(r);
    if (const char *e = dev_env("SM_XBAND")) r.layout = atoi(e) ? SM_LAYOUT_BANDS : SM_LAYOUT_NO_BANDS;
    if (const char *e = dev_env("SM_XBAND_KIND")) {
        static const char *names[] = {"", "exact", "blocked", "gather", "band2", "cband"};
        for (int k = 1; k <= 5; ++k)
            if (strcmp(e, names[k]) == 0) r.layout = k;
        if (strcmp(e, "sweep") == 0) r.layout = SM_LAYOUT_SWEEP;
        if (strcmp(e, "gcb") == 0) r.layout = SM_LAYOUT_GCB;
    }
    if (const char *e = dev_env("SM_BAND_TALL")) r.band_tall = atoi(e);
    if (const char *e = dev_env("SM_BAND2_SLABS")) r.band_slabs = atoi(e);
    if (const char *e = dev_env("SM_BAND_SLAB0")) r.band_slab0_permille = atoi(e);
    if (const char *e = dev_env("SM_XBAND_GBAND")) r.gather_band_log2 = atoi(e);
    if (const char *e = dev_env("SM_RELABEL")) r.relabel = atoi(e);
    if (const char *e = dev_env("SM_SELL")) r.sell = atoi(e) ? -1 : 0;
    if (const char *e = dev_env("SM_SELL_CB")) r.sell_codebook = atoi(e) ? -1 : 0;
    if (const char *e = dev_env("SM_SELL_MAX")) r.sell_max_len = atoi(e);
    if (const char *e = dev_env("SM_SELL_SIGMA")) r.sell_sigma = atoll(e);
    if (const char *e = dev_env("SM_SELL_STREAMS")) r.sell_streams = atoi(e);
    if (const char *e = dev_env("SM_TILE_NNZ")) r.tile_nnz = atoi(e);
    if (const char *e = dev_env("SM_CCSELL")) r.ccsell = atoi(e);
    if (const char *e = dev_env("SM_CCSELL_CHUNK")) r.ccsell_chunk_log2 = atoi(e);
    if (const char *e = dev_env("SM_HOT_COLS")) r.hot_cols = atoi(e);
    if (const char *e = dev_env("SM_MERGE_STAGE")) r.merge_stage = atoi(e);
    if (const char *e = dev_env("SM_HOST_BUILD")) r.host_build = atoi(e);
    return r;
}

sm_status check_opts(const sm_build_opts *o, bool table_ok) {
    if (!o) return SM_OK;
    if (o->struct_size < (int32_t)(2 * sizeof(int32_t)))
        return fail(SM_ERR_INVALID_ARG, "sm_build_opts.struct_size %d: call sm_build_opts_init",
                    o->struct_size);
    const BuildOpts r = resolve_opts(o);
    if (r.layout < SM_LAYOUT_AUTO || r.layout > SM_LAYOUT_GCB)
        return fail(SM_ERR_INVALID_ARG, "unknown layout %d", r.layout);
    if (r.band_slabs < 0 || r.band_slabs > 16) return fail(SM_ERR_INVALID_ARG, "band_slabs not in [0, 16]");
    if (r.band_tall != 0 && r.band_tall != 4 && r.band_tall != 6)
        return fail(SM_ERR_INVALID_ARG, "band_tall must be 0 (dma3), 4 (dma3) or 6 (wide)");
    if (r.gather_band_log2 != 0 && (r.gather_band_log2 < 13 || r.gather_band_log2 > 15))
        return fail(SM_ERR_INVALID_ARG, "gather_band_log2 must be 0 or 13..15");
    if (r.tile_nnz != 0 && r.tile_nnz != 1024 && r.tile_nnz != 2048 && r.tile_nnz != 4096 &&
        r.tile_nnz != 8192)
        return fail(SM_ERR_INVALID_ARG, "tile_nnz must be 0, 1024, 2048, 4096 or 8192");
    if (r.sell_max_len < 0 || r.sell_streams < 0 || r.sell_sigma < 0)
        return fail(SM_ERR_INVALID_ARG, "negative sell option");
    if (r.ccsell_chunk_log2 != 0 && (r.ccsell_chunk_log2 < 8 || r.ccsell_chunk_log2 > 24))
        return fail(SM_ERR_INVALID_ARG, "ccsell_chunk_log2 must be 0 or 8..24");
    if (r.hot_cols < -1) return fail(SM_ERR_INVALID_ARG, "hot_cols must be -1, 0 or positive");
    if (r.exact_sell < -1 || r.exact_sell > 1) return fail(SM_ERR_INVALID_ARG, "exact_sell must be -1, 0 or 1");
    if (r.band_slab0_permille != 0 && (r.band_slab0_permille < 500 || r.band_slab0_permille > 1000))
        return fail(SM_ERR_INVALID_ARG, "band_slab0_permille must be 0 or 500..1000");
    if (r.merge_stage != 0 && r.merge_stage != 1) return fail(SM_ERR_INVALID_ARG, "merge_stage must be 0 or 1");
    if (r.host_build != 0 && r.host_build != 1) return fail(SM_ERR_INVALID_ARG, "host_build must be 0 or 1");
    if (r.updatable != 0 && r.updatable != 1) return fail(SM_ERR_INVALID_ARG, "updatable must be 0 or 1");
    if (r.updatable) {   // no codebook forms: their words hold ids chosen from the values
        if (r.layout == SM_LAYOUT_CBAND || r.layout == SM_LAYOUT_SWEEP)
            return fail(SM_ERR_INVALID_ARG, "updatable: layout %d exists only in codebook form", r.layout);
        if (r.hot_cols > 0) return fail(SM_ERR_INVALID_ARG, "updatable: hot_cols exists only in codebook form");
        if (r.merge_stage == 1) return fail(SM_ERR_INVALID_ARG, "updatable: merge_stage exists only in codebook form");
    }
    if (r.table_updatable != 0 && r.table_updatable != 1)
        return fail(SM_ERR_INVALID_ARG, "table_updatable must be 0 or 1");
    if (r.table_updatable) {   // codebook forms only, from the given ids and table
        if (!table_ok)
            return fail(SM_ERR_INVALID_ARG, "table_updatable: only sm_create_from_csr_ids and sm_create_transpose "
                                            "of a table matrix honour it");
        if (r.updatable) return fail(SM_ERR_INVALID_ARG, "table_updatable and updatable exclude each other");
        if ((r.layout >= SM_LAYOUT_EXACT && r.layout <= SM_LAYOUT_BAND2) || r.layout == SM_LAYOUT_GCB)
            return fail(SM_ERR_INVALID_ARG, "table_updatable: layout %d exists only in plain form", r.layout);
        if (r.sell_codebook == 0) return fail(SM_ERR_INVALID_ARG, "table_updatable: sell_codebook = 0 asks for the plain form");
        if (r.hot_cols > 0) return fail(SM_ERR_INVALID_ARG, "table_updatable: hot_cols is not supported");
        if (r.merge_stage == 1) return fail(SM_ERR_INVALID_ARG, "table_updatable: merge_stage is not supported");
    }
    return SM_OK;
}

int32_t tile_nnz_setting(const sm_matrix *m) {
    const int v = m->opts.tile_nnz;
    return (v == 1024 || v == 2048 || v == 4096 || v == 8192) ? v : kTileNnz;
}

bool kind_forced(const sm_matrix *m) {
    return (m->opts.layout >= SM_LAYOUT_EXACT && m->opts.layout <= SM_LAYOUT_CBAND) ||
           m->opts.layout == SM_LAYOUT_GCB;
}

// Column-band layout.  SM_LAYOUT_NO_BANDS disables it,
// SM_LAYOUT_BANDS (or a forced kind) builds it; otherwise it is built when sweeping x
// through every tile's LDS costs less than the random gathers it replaces.  Cost model
// from profiles/r01_microbench.txt: a tile streams x into LDS at ~85 GB/s per CU
// (~22 TB/s chip-wide) while 4-byte gathers run at 75-200 G/s by the size of x,
// so the sweep wins while its bytes stay under ~20x the matrix's 8 B per term.
// AUTO's kind: cband (balanced bands of codebook words, kernels_band2.hip; band2 when
// the values take more than 255 bit patterns; it falls back to blocked when its bands
// would be < 70 % filled), or gather for wide matrices -- measured per rank of the
// bench's row partition (1M rows, 16 terms per row), blocked vs gather
// with 16K- / 32K-column bands: 1M columns 46 vs 59 / -, 2M 59 vs 60 / 66, 4M 85 vs
// 77 / 73, 8M 145 vs - / 93 us.  Past ~3M columns each blocked tile sweeps more x
// through LDS than gathering its terms' x costs.
constexpr int64_t kGatherCols = 3 * ((int64_t)1 << 20);   // gather kind: > 3M columns
// Gathered chunk bands (gcb.h): past 16M columns (config 5's 64M-column rank slices: 0.83 vs
// 1.61 ms for the gather kind) -- the gather kind's 32K-column bands hold too
// few terms there; where the gather kind's own cost model accepts a band layout.
constexpr int64_t kGcbCols = (int64_t)1 << 24;

XbKind xband_kind_setting(const sm_matrix *m) {
    switch (m->opts.layout) {
    case SM_LAYOUT_EXACT: return kXbExact;
    case SM_LAYOUT_BLOCKED: return kXbBlocked;
    case SM_LAYOUT_GATHER: return kXbGather;
    case SM_LAYOUT_BAND2: return kXbBand2;
    case SM_LAYOUT_CBAND: return kXbCband;
    case SM_LAYOUT_GCB: return kXbGcb;
    default: break;
    }
    // Updatable matrices take no codebook form: band2's 8-byte entries where cband would serve.
    // table_updatable ones take only codebook forms: cband wherever a band layout is built.
    if (m->opts.table_updatable) return kXbCband;
    return m->n_cols >= kGcbCols ? kXbGcb : m->n_cols > kGatherCols ? kXbGather
           : m->opts.updatable ? kXbBand2 : kXbCband;
}

// The slot -> term map of a layout built for an updatable matrix (empty otherwise: nothing
// allocated), uploaded beside the layout's slots.
sm_status upload_term_map(sm_matrix *m, const std::vector<int32_t> &term, int32_t **d_term) {
    if (term.empty()) return SM_OK;
    SM_TRY_HIP(dev_upload(m->mem, d_term, term));
    return SM_OK;
}

// Sweeping x through LDS (or walking its bands) pays when the L2 -> LDS bytes of
// one kind's row blocks stay within 20x the matrix stream.  The gather kind sweeps no
// x: its cost is its bands' skeleton plus its terms, set against the sliced ELL's cost
// per term on wide uniform matrices -- constants from the two measured wide shapes
// (config 2 rows at 8M columns: 16K bands of 1K terms, 93 us; config 5's rank slice,
// 8M x 64M: 1M bands of 128 terms, 1.60 ms; its ccsell 2.30 ms = 17 ps per term).
static bool gather_cost_ok(const sm_matrix *m) {
    // Calibrated on uniform rows: skewed ones (longest row > 64x the mean, e.g. R-MAT)
    // keep the sliced ELL, whose long-row segments balance them.
    if ((double)m->plan.max_row_nnz > 64.0 * (double)m->nnz / (double)std::max<int64_t>(1, m->n_rows))
        return false;
    const int64_t nblk = (m->n_rows + (1 << kXbGatherRowsLog2) - 1) >> kXbGatherRowsLog2;
    const double bands = (double)nblk * (double)((m->n_cols + (1 << kXbGatherWideBandLog2) - 1) >>
                                                 kXbGatherWideBandLog2);
    const double per_band_us = 0.25 + 1.2e-3 * (double)m->nnz / bands;
    const double gather_us = bands / 256.0 * per_band_us;
    const double sell_us = 1.7e-5 * (double)m->nnz;
    return gather_us < sell_us;
}

// Below this many terms AUTO keeps the sorted sliced ELL instead of a swept band layout: a
// band SpMV carries ~20 us of fixed cost (x staging per tile, the slab hand-off) that small
// matrices do not amortise, and their few row blocks leave CUs idle (16K rows: 16 tiles).
// Uniform 16-per-row squares, eager SpMV incl. launch (tools/small_auto_ab.py,
// profiles/r06_small_auto_ab.txt): 2^18 rows (4.2 M terms) cband 31.3 vs sell 22.3 us,
// 2^19 (8.4 M) 34.6 vs 41.6 us.
constexpr int64_t kBandMinNnz = 6 * ((int64_t)1 << 20);

static bool xband_cost_ok(const sm_matrix *m, XbKind kind) {
    if ((kind == kXbGather || kind == kXbGcb) && m->n_cols > kGatherCols && m->opts.gather_band_log2 == 0)
        return gather_cost_ok(m);   // gcb: ~2x faster than the gather kind it is priced as
    if (m->nnz < kBandMinNnz) return false;
    const int rows_log2 = kind == kXbExact    ? kXbExactRowsLog2
                          : kind == kXbBand2 || kind == kXbCband ? kB2RowBits
                          : kind == kXbGather ? kXbGatherRowsLog2
                                              : kXbBlockedRowsLog2;
    const int64_t nblk = (m->n_rows + (1 << rows_log2) - 1) >> rows_log2;
    const double x_sweep = (double)nblk * 4.0 * (double)m->n_cols;   // L2 -> LDS bytes
    const double stream = 8.0 * (double)m->nnz;                      // HBM bytes
    return x_sweep <= 20.0 * stream && m->n_cols >= 8192;
}

bool want_xband(const sm_matrix *m) {
    const int32_t L = m->opts.layout;
    if (L == SM_LAYOUT_NO_BANDS || L == SM_LAYOUT_SWEEP) return false;
    if (m->nnz == 0 || m->n_rows == 0) return false;
    if (L != SM_LAYOUT_AUTO) return true;   // a forced kind, or SM_LAYOUT_BANDS
    return xband_cost_ok(m, xband_kind_setting(m));
}

// The one source of (table, ids) for the codebook forms.  A table_updatable matrix gives its own:
// the T entries in the given order (equal entries apart, unused ones kept) and the given ids --
// nothing is derived from the value bits.  Every other matrix derives them from the values
// (codebook_ids: distinct bit patterns in CSR order; false past 255).  `ids` points into `own`
// or at the matrix's ids (all nnz terms of the CSR, in its order).
static bool codebook_source(const sm_matrix *m, const float *val, int64_t nnz, std::vector<float> &table,
                            std::vector<uint8_t> &own, const uint8_t *&ids) {
    if (m->opts.table_updatable) {
        if (!m->build_ids || !m->build_table || nnz != m->nnz) return false;
        table.assign(m->build_table, m->build_table + m->tab_size);
        ids = m->build_ids;
        return true;
    }
    if (!codebook_ids(val, nnz, table, own)) return false;
    ids = own.data();
    return true;
}

// The slab scratch of a band layout whose n_blocks and n_slabs are set: `row_sets` sets of n_rows
// partial sums, each set 16-byte aligned, and the hand-off control words, 4 per block and zero
// between SpMVs.  Nothing for one slab.
static sm_status alloc_slab_scratch(sm_matrix *m, BandTiles &d, int64_t n_rows, int64_t row_sets) {
    if (d.n_slabs <= 1) return SM_OK;
    SM_TRY_HIP(m->mem.alloc(&d.d_partials, row_sets * ((n_rows + 3) & ~(int64_t)3)));
    SM_TRY_HIP(m->mem.alloc(&d.d_tickets, 4 * (int64_t)d.n_blocks));
    SM_TRY_HIP(hipMemset(d.d_tickets, 0, (size_t)d.n_blocks * 4 * sizeof(int32_t)));
    return SM_OK;
}

// Balanced-band layout (band2.cpp, kernels_band2.hip): slabs so there are about
// kXbTargetTiles tiles of <= 16K rows.  kind cband: 4-byte codebook words when the
// values take <= 255 distinct bit patterns, else (or kind band2) 8-byte entries.
// Builds into `d` the balanced bands of an n_rows x n_cols CSR (the matrix's own, or
// the hot column prefix of a relabeled graph); `forced`: keep mostly-padding bands.
// Geometry (sm_build_opts.band_tall): 0 = the default (dma3, both encodings: a loader wave
// stages x -- config 2 34.0-34.6 vs 36.9-37.1 us for the wide geometry with codebook words,
// 37.9-38.0 vs 38.6-38.7 with 8-byte entries), 4 = dma3, 6 = wide.  dma3
// bands that would be < 70 % full fall back to wide.
// The slabs a band2 layout asks band2_build for (sm_build_opts.band_slabs, or about
// kXbTargetTiles tiles).
static int32_t band2_want_slabs(int64_t n_rows, int32_t slabs) {
    const int64_t br = std::min<int64_t>(kB2BlockRows, n_rows);
    const int64_t nblk = (n_rows + br - 1) / br;
    int32_t want = (int32_t)std::max<int64_t>(
        1, std::min<int64_t>(16, (kXbTargetTiles + nblk - 1) / nblk));
    if (slabs > 0) want = std::max(1, std::min(16, slabs));
    return want;
}

// The rest of a built band2 / cband layout (its bands already in d_tile_band / d_band_clo /
// d_ent, by the host or the device builder): the descriptor, the codebook and the slab scratch.
static sm_status band2_finish(sm_matrix *m, Band2Dev &d, const Band2Host &bh, const std::vector<float> &table,
                              int64_t n_rows) {
    d.kind = bh.codebook ? kXbCband : kXbBand2;
    d.block_rows = bh.block_rows;
    d.n_blocks = bh.n_blocks;
    d.n_bands = (int32_t)std::min<int64_t>(bh.n_bands, INT32_MAX);
    d.n_slabs = bh.n_slabs;
    d.window = bh.geom.window;
    d.slab_cols = bh.slab_cols;
    d.slab0_cols = bh.slab0_cols;
    if (bh.codebook) {
        SM_TRY_HIP(dev_upload_table(m->mem, &d.d_table, table.data(), (int32_t)table.size()));
        d.table_size = (int32_t)table.size();
    }
    // One row set per slab: the beta-last hand-off (kernels_band2.hip SM_B2_BL) publishes slab 0's
    // sums too (the other form writes them into y and leaves the last one unused).
    return alloc_slab_scratch(m, d, n_rows, bh.n_slabs);
}

static sm_status build_band2(sm_matrix *m, Band2Dev &d, int64_t n_rows, int64_t n_cols, int64_t nnz,
                             const int32_t *rp, const int32_t *col, const float *val, XbKind kind,
                             int32_t geo_opt, int32_t slabs, bool forced, int32_t slab0_permille = 1000) {
    const bool dma3 = geo_opt != 6;
    const int32_t want = band2_want_slabs(n_rows, slabs);
    std::vector<float> table;
    std::vector<uint8_t> ids;
    const uint8_t *idp = nullptr;
    const bool upd = m->opts.updatable != 0;   // no layout decision reads the values
    const bool cb = kind == kXbCband && !upd && codebook_source(m, val, nnz, table, ids, idp);
    if (m->opts.table_updatable && !cb) return SM_OK;   // codebook form or none
    Band2Host bh;
    B2Geom g = dma3 ? (cb ? kB2Dma3Cb : kB2Dma3B2) : kB2Wide;
    // Bands are fixed slots of g.chunks() * 64 entries: where a slab's density leaves
    // them mostly dummies (wide or very sparse matrices), the padding would cost more HBM
    // bytes than the layout saves -- decline unless forced (SM_LAYOUT_BAND2 / CBAND).
    auto fits = [&](const B2Geom &gg) {
        if (!band2_build(rp, col, val, n_rows, n_cols, want, bh, cb ? idp : nullptr, gg, slab0_permille, upd))
            return false;
        return forced || bh.n_bands == 0 ||
               (double)bh.real_terms >= 0.7 * (double)bh.n_bands * gg.chunks() * 64;
    };
    bool ok = fits(g);
    if (!ok && g.nch != 0) {   // dma3 did not fit: wide
        g = kB2Wide;
        ok = fits(g);
    }
    if (!ok) return SM_OK;
    std::vector<uint8_t>().swap(ids);
    const int64_t band_words = (int64_t)(cb ? 64 : 128) * g.chunks();
    const int64_t ntile = (int64_t)bh.n_blocks * bh.n_slabs;
    SM_TRY_HIP(m->mem.alloc(&d.d_tile_band, ntile + 1));
    SM_TRY_HIP(m->mem.alloc(&d.d_band_clo, std::max<int64_t>(1, bh.n_bands)));
    SM_TRY_HIP(m->mem.alloc(&d.d_ent, std::max<int64_t>(1, bh.n_bands * band_words)));
    if (const sm_status sts = band2_finish(m, d, bh, table, n_rows)) return sts;
    SM_TRY_HIP(hipMemcpy(d.d_tile_band, bh.tile_band_start.data(), (size_t)(ntile + 1) * 4,
                         hipMemcpyHostToDevice));
    if (bh.n_bands > 0) {
        SM_TRY_HIP(hipMemcpy(d.d_band_clo, bh.band_clo.data(), (size_t)bh.n_bands * 4,
                             hipMemcpyHostToDevice));
        SM_TRY_HIP(hipMemcpy(d.d_ent, bh.ent.data(), (size_t)(bh.n_bands * band_words) * 4,
                             hipMemcpyHostToDevice));
    }
    if (const sm_status stm = upload_term_map(m, bh.term, &d.d_term)) return stm;
    d.n_term = (int64_t)bh.term.size() / 2;
    return SM_OK;
}

// Gathered chunk bands (gcb.h, kernels_gcb.hip): 32K-row tiles where the rows make at
// least 256 of them (one per CU), else 16K-row tiles; slabs so the tiles reach 256.
static void gcb_geometry(const sm_matrix *m, int &rows_log2, int32_t &slabs) {
    rows_log2 = m->n_rows >= ((int64_t)kXbTargetTiles << 15) ? 15 : 14;
    const int64_t nblk = (m->n_rows + ((int64_t)1 << rows_log2) - 1) >> rows_log2;
    slabs = (int32_t)std::max<int64_t>(1, std::min<int64_t>(16, (kXbTargetTiles + nblk - 1) / nblk));
    if (m->opts.band_slabs > 0) slabs = m->opts.band_slabs;
}

// The rest of a built gcb layout (its bands already in d_tile_band / d_band_clo / d_ent):
// the geometry, slab partials and hand-off words.
static sm_status gcb_finish(sm_matrix *m, const GcbHost &gh) {
    GcbDev &d = m->plan.gcb;
    d.kind = kXbGcb;
    d.block_rows = gh.block_rows;
    d.n_blocks = gh.n_blocks;
    d.n_bands = (int32_t)std::min<int64_t>(gh.n_bands, INT32_MAX);
    d.n_slabs = gh.n_slabs;
    d.window = gh.window;
    d.slab_cols = gh.slab_cols;
    return alloc_slab_scratch(m, d, m->n_rows, gh.n_slabs - 1);
}

static sm_status upload_gcb(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    int rows_log2 = 0;
    int32_t slabs = 1;
    gcb_geometry(m, rows_log2, slabs);
    GcbHost gh;
    if (!gcb_build(rp, col, val, m->n_rows, m->n_cols, rows_log2, slabs, kGcbMaxWindow, gh, m->opts.updatable != 0))
        return SM_OK;
    GcbDev &d = m->plan.gcb;
    const int64_t ntile = (int64_t)gh.n_blocks * gh.n_slabs;
    SM_TRY_HIP(m->mem.alloc(&d.d_tile_band, ntile + 1));
    SM_TRY_HIP(m->mem.alloc(&d.d_band_clo, std::max<int64_t>(1, gh.n_bands)));
    SM_TRY_HIP(m->mem.alloc(&d.d_ent, std::max<int64_t>(1, gh.n_bands * kGcbBandWords)));
    SM_TRY_HIP(hipMemcpy(d.d_tile_band, gh.tile_band_start.data(), (size_t)(ntile + 1) * 4,
                         hipMemcpyHostToDevice));
    if (gh.n_bands > 0) {
        SM_TRY_HIP(hipMemcpy(d.d_band_clo, gh.band_clo.data(), (size_t)gh.n_bands * 4, hipMemcpyHostToDevice));
        SM_TRY_HIP(hipMemcpy(d.d_ent, gh.ent.data(), (size_t)gh.n_bands * kGcbBandWords * 4,
                             hipMemcpyHostToDevice));
    }
    if (const sm_status stm = upload_term_map(m, gh.term, &d.d_term)) return stm;
    d.n_term = (int64_t)gh.term.size() / 2;
    return gcb_finish(m, gh);
}

sm_status upload_xband(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val,
                       XbKind kind) {
    if (kind == kXbGcb) return upload_gcb(m, rp, col, val);
    if (kind == kXbBand2 || kind == kXbCband) {
        // Geometry: band_tall (xband.h B2Geom, build_band2).
        // Slab 0's tile loads and scales y (64 KiB per 16K-row block from HBM) before its first
        // band: on config 2 its band loop ended 1.5-2.3 us after the other slabs' (per-tile
        // timeline, profiles/r05_dma3_tile_timeline_dump.txt).  Narrower slab-0 tiles did not
        // shorten the kernel (kB2Slab0Permille), so AUTO keeps even slabs; the option stays.
        const int32_t p0 = m->opts.band_slab0_permille > 0 ? m->opts.band_slab0_permille : kB2Slab0Permille;
        const sm_status st = build_band2(m, m->plan.b2, m->n_rows, m->n_cols, m->nnz, rp, col, val, kind,
                                         m->opts.band_tall, m->opts.band_slabs, kind_forced(m), p0);
        if (st == SM_OK && m->plan.b2.n_blocks == 0 && !kind_forced(m) && !m->opts.table_updatable)
            return upload_xband(m, rp, col, val, kXbBlocked);   // declined: blocked kind
        return st;
    }
    // Gather kind: AUTO takes it past kGatherCols (3M columns) with bands of 32K
    // columns -- fewer bands, hence fewer per-band barriers, for the same terms (8M
    // columns: 93 us with 32K bands vs 122 with 8K); the rank field shrinks to 3 bits,
    // ample at < 0.25 terms per row per band.  A forced gather kind on a narrower
    // matrix keeps 8K-column bands.  gather_band_log2 = 13|14|15 forces the band width
    // (16K: measured slower than the blocked kind at 2M).
    const int gb = m->opts.gather_band_log2;
    const int gband_log2 = gb == 15 ? kXbGatherWideBandLog2
                           : gb == 14 ? kXbGatherWideBandLog2 - 1
                           : gb == 13 ? kXbGatherBandLog2
                           : m->n_cols > kGatherCols ? kXbGatherWideBandLog2
                                                     : kXbGatherBandLog2;
    const XbBits bits = kind == kXbExact    ? xb_bits(kXbExactBandLog2, kXbExactRowsLog2)
                        : kind == kXbGather ? xb_bits(gband_log2, kXbGatherRowsLog2)
                                            : xb_bits(kXbBlockedBandLog2, kXbBlockedRowsLog2);
    XbandHost xh;
    // Register capacity from the waves that hold entries: 12 on the blocked kind
    // (4 loader waves stage x), all 16 on the exact and gather kinds.
    const int entry_waves = kind == kXbBlocked ? kXbComputeWaves : kXbThreads / 64;
    if (!xband_build(rp, col, val, m->n_rows, m->n_cols, bits, entry_waves, xh,
                     kind == kXbGather, 0, m->opts.updatable != 0)) {
        // The gather kind's wide bands leave 3-4 rank bits: a matrix with longer row
        // segments may still fit the blocked layout (5 bits, 8K-column bands).
        // Only where the blocked kind's own sweep cost still pays (its row blocks
        // differ from the gather kind's); otherwise the stream kernel serves it.
        if (kind == kXbGather && !kind_forced(m) &&
            (xband_cost_ok(m, kXbBlocked) || m->opts.layout == SM_LAYOUT_BANDS))
            return upload_xband(m, rp, col, val, kXbBlocked);
        return SM_OK;   // layout not applicable: the stream kernel serves this matrix
    }
    XbandDev &d = m->plan.xb;
    // Blocked: split the bands in slabs so there are >= kXbTargetTiles tiles.
    int32_t n_slabs = 1;
    if (kind != kXbExact) {
        // At most 64 slabs: the hand-off counts arrivals in 8 bits (kernels_xband.hip).
        const int64_t want = std::min<int64_t>(64, ((int64_t)kXbTargetTiles + xh.n_blocks - 1) / xh.n_blocks);
        n_slabs = (int32_t)std::max<int64_t>(1, std::min<int64_t>(want, xh.n_bands));
    }
    // Slabs of whole groups of 8 bands (the kernel steps bands 4 or 8 at a time).
    int32_t slab_bands = (xh.n_bands + n_slabs - 1) / n_slabs;
    slab_bands = (slab_bands + 7) & ~7;
    n_slabs = (xh.n_bands + slab_bands - 1) / slab_bands;
    std::vector<int32_t> cs32(xh.chunk_start.size());
    for (size_t i = 0; i < cs32.size(); i++) cs32[i] = (int32_t)xh.chunk_start[i];
    SM_TRY_HIP(dev_upload(m->mem, &d.d_chunk_start, cs32));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_word, xh.word));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_val, xh.val));
    d.kind = kind;
    d.block_rows = xh.block_rows;
    d.n_blocks = xh.n_blocks;
    d.n_bands = xh.n_bands;
    d.n_slabs = n_slabs;
    d.slab_bands = slab_bands;
    d.band_cols = xh.band_cols;
    d.max_chunks_per_band = xh.max_chunks_per_band;
    if (const sm_status sts = alloc_slab_scratch(m, d, m->n_rows, n_slabs - 1)) return sts;
    if (const sm_status stm = upload_term_map(m, xh.term, &d.d_term)) return stm;
    d.n_term = (int64_t)xh.term.size();
    return SM_OK;
}

// Column relabeling for the stream kernel.  relabel = 0 disables
// it, 1 forces it; otherwise it is built when x is larger than an XCD's
// L2 (>= 2^20 columns), no band layout serves the matrix, there are at least as many
// terms as columns (the per-SpMV permutation of x is then cheap next to the
// product), and the column degrees are skewed: the busiest 1/16 of the columns hold
// >= 40 % of the terms (power-law graphs: R-MAT scale 24 has 87 % there).
bool want_relabel_size(const sm_matrix *m) {
    if (m->opts.relabel == 0) return false;
    if (m->nnz == 0 || m->n_cols == 0) return false;
    if (m->opts.relabel == 1) return true;
    return m->n_cols >= (1 << 20) && m->nnz >= m->n_cols && !m->plan.band();
}

sm_status upload_relabel(sm_matrix *m, const int32_t *col) {
    const int64_t nc = m->n_cols, nnz = m->nnz;
    std::vector<int32_t> deg((size_t)nc, 0);
    for (int64_t e = 0; e < nnz; e++) deg[(size_t)col[e]]++;
    // new -> old, by descending degree; ties keep the original order (counting sort).
    int32_t dmax = 0;
    for (int32_t d : deg) dmax = std::max(dmax, d);
    std::vector<int64_t> start((size_t)dmax + 2, 0);
    for (int32_t d : deg) start[(size_t)(dmax - d) + 1]++;
    for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
    std::vector<int32_t> perm((size_t)nc), rank((size_t)nc);
    for (int64_t c = 0; c < nc; c++) {
        const int64_t j = start[(size_t)(dmax - deg[(size_t)c])]++;
        perm[(size_t)j] = (int32_t)c;
        rank[(size_t)c] = (int32_t)j;
    }
    if (m->opts.relabel != 1) {
        int64_t hot = 0;
        for (int64_t j = 0; j < nc / 16; j++) hot += deg[(size_t)perm[(size_t)j]];
        if ((double)hot < 0.4 * (double)nnz) return SM_OK;   // not skewed: no gain
    }
    std::vector<int32_t> rcol((size_t)nnz);
    for (int64_t e = 0; e < nnz; e++) rcol[(size_t)e] = rank[(size_t)col[e]];
    Plan &p = m->plan;
    SM_TRY_HIP(m->mem.alloc(&p.d_perm, nc + 4));
    SM_TRY_HIP(m->mem.alloc(&p.d_rcol, nnz + kPadElems));
    SM_TRY_HIP(m->mem.alloc(&p.d_xperm, nc + 4));
    // The SpMV permutes x by scattering it (coalesced reads, stores that never stall):
    // the device keeps the original -> new map.
    SM_TRY_HIP(hipMemcpy(p.d_perm, rank.data(), (size_t)nc * 4, hipMemcpyHostToDevice));
    SM_TRY_HIP(hipMemcpy(p.d_rcol, rcol.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
    SM_TRY_HIP(hipMemset(p.d_rcol + nnz, 0, kPadElems * sizeof(int32_t)));
    p.n_relabel = nc;
    return SM_OK;
}

// The merge path's column-sorted staging stream (kernels_merge.hip MergeStage), over the
// columns the merge kernel gathers with (the relabeled ones when the plan has them).
bool want_merge_stage(const sm_matrix *m) {
    return m->nnz > 0 && m->n_rows > 0 && m->opts.merge_stage == 1;
}

sm_status upload_merge_stage(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    std::vector<int32_t> rcol;
    if (m->plan.n_relabel > 0) {   // the relabeled columns (the plan keeps them on the device)
        rcol.resize((size_t)m->nnz);
        SM_TRY_HIP(hipMemcpy(rcol.data(), m->plan.d_rcol, (size_t)m->nnz * 4, hipMemcpyDeviceToHost));
        col = rcol.data();
    }
    std::vector<uint32_t> w;
    std::vector<uint16_t> z;
    std::vector<float> table;
    if (!merge_stage_build(rp, col, val, m->n_rows, m->n_cols, m->nnz, w, z, table)) return SM_OK;
    Plan &p = m->plan;
    SM_TRY_HIP(dev_upload(m->mem, &p.d_mstage_w, w));       // nnz words
    SM_TRY_HIP(dev_upload(m->mem, &p.d_mstage_z, z));       // nnz slots
    SM_TRY_HIP(dev_upload(m->mem, &p.d_mstage_tab, table)); // 256 values, zero past the codebook
    return SM_OK;
}

// Sorted sliced-ELL (sell.h, kernels_sell.hip) for every matrix no band layout
// serves (SM_SELL=0 disables it): faster than the stream kernel on uniform rows
// (config-2 shape without bands 100 vs 109 us, 2^17 rows 14.5 vs 15.8 us) and on
// R-MAT (1.91 vs 2.30 ms), and every row up to kSellMaxLen terms is summed in the
// reference's order (the stream kernel: rows up to 64).
bool want_sell(const sm_matrix *m) {
    if (m->opts.sell == 0) return false;
    return m->nnz > 0 && m->n_rows > 0 && !m->plan.band() && m->plan.cc.n_slices == 0 &&
           m->plan.sw.n_blocks == 0;
}

sm_status upload_sell(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val,
                      int64_t nnz = -1, bool cols_relabeled = false, SellDev *target = nullptr,
                      int32_t max_len_override = 0) {
    Plan &p = m->plan;
    if (nnz < 0) nnz = m->nnz;
    std::vector<int32_t> rcol;
    const int32_t *c = col;
    if (p.n_relabel > 0 && !cols_relabeled) {   // the layout stores relabeled columns (x is permuted per SpMV)
        rcol.resize((size_t)m->nnz);
        SM_TRY_HIP(hipMemcpy(rcol.data(), p.d_rcol, (size_t)m->nnz * 4, hipMemcpyDeviceToHost));
        c = rcol.data();
    }
    // Rows up to max_len terms go to the slices (one lane each, in stored order); the
    // longer ones as max_len-term segments.  sell_max_len overrides the cap.
    const int32_t max_len = max_len_override > 0       ? max_len_override
                            : m->opts.sell_max_len > 0 ? m->opts.sell_max_len
                                                       : kSellMaxLen;
    // sell_sigma: sort within windows of that many rows (0: one window),
    // sell_streams: XCD streams of windows (default 8 with windows).
    const int64_t sigma = std::max<int64_t>(0, m->opts.sell_sigma);
    const int streams = m->opts.sell_streams > 0 ? m->opts.sell_streams : sigma > 0 ? 8 : 1;
    // Codebook form (sell_codebook = 0 disables it): values of <= 255 distinct bit
    // patterns and columns < 2^24 -- one 4-byte word per slot instead of column + value.
    std::vector<float> table;
    std::vector<uint8_t> ids;
    const bool upd = m->opts.updatable != 0;   // the plain form: no decision reads the values
    const uint8_t *idp = nullptr;
    const bool cb = m->opts.sell_codebook != 0 && !upd && m->n_cols <= ((int64_t)1 << kSellCbColBits) &&
                    codebook_source(m, val, nnz, table, ids, idp);
    if (m->opts.table_updatable && !cb) return SM_OK;   // codebook form or none: the stream kernel serves
    if (!cb) std::vector<uint8_t>().swap(ids);
    SellHost sh;
    sell_build(rp, c, val, m->n_rows, max_len, sh, sigma, streams, cb ? idp : nullptr, upd);
    std::vector<int32_t>().swap(rcol);
    std::vector<uint8_t>().swap(ids);
    if (sh.n_slices == 0) return SM_OK;
    if (sh.padded >= ((int64_t)1 << 31) - kSellLanes * kSellUnroll) return SM_OK;
    SellDev &d = target ? *target : p.sell;
    d.max_len = max_len;
    d.n_long = (int32_t)sh.long_rows.size();
    const int32_t n_parts = sh.long_ptr.back();
    SM_TRY_HIP(dev_upload(m->mem, &d.d_long_rows, sh.long_rows));   // n_long
    SM_TRY_HIP(dev_upload(m->mem, &d.d_long_ptr, sh.long_ptr));     // n_long + 1
    SM_TRY_HIP(m->mem.alloc(&d.d_partials, n_parts));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_off, sh.off));               // n_slices
    SM_TRY_HIP(dev_upload(m->mem, &d.d_len, sh.len));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_row, sh.row));               // n_slices * kSellLanes
    SM_TRY_HIP(dev_upload(m->mem, &d.d_row_len, sh.row_len));
    // + a zeroed tail of 32 slots per lane: unrolls past kSellUnroll read up to it.
    const int64_t tail = 32 * kSellLanes;
    SM_TRY_HIP(m->mem.alloc(&d.d_col, sh.padded + tail));
    SM_TRY_HIP(hipMemset(d.d_col + sh.padded, 0, (size_t)tail * 4));
    if (cb) {
        SM_TRY_HIP(m->mem.alloc(&d.d_table, std::max<int64_t>((int64_t)table.size(), 1)));
        if (!table.empty())
            SM_TRY_HIP(hipMemcpy(d.d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice));
        d.table_size = (int32_t)table.size();
    } else {
        SM_TRY_HIP(m->mem.alloc(&d.d_val, sh.padded + tail));
        SM_TRY_HIP(hipMemset(d.d_val + sh.padded, 0, (size_t)tail * 4));
    }
    if (sh.padded) {
        SM_TRY_HIP(hipMemcpy(d.d_col, sh.col.data(), (size_t)sh.padded * 4, hipMemcpyHostToDevice));
        if (!cb) SM_TRY_HIP(hipMemcpy(d.d_val, sh.val.data(), (size_t)sh.padded * 4, hipMemcpyHostToDevice));
    }
    if (const sm_status stm = upload_term_map(m, sh.term, &d.d_term)) return stm;
    d.n_term = (int64_t)sh.term.size();
    d.n_slices = sh.n_slices;
    return SM_OK;
}

// SM_ALGO_EXACT: the fastest launch built for `m` that adds every output's terms in the
// reference's order (kernel.cc:780-796, sparse-matrix.cc:164-190) -- what the reference's
// C++ surface runs (sblas_shim.cpp).  The band kernels need x 16-byte aligned (`x16`).
// kAlgoExactSell: the unsegmented sliced ELL built for this (upload_exact_sell).
int exact_algo(const sm_matrix *m, bool x16) {
    const Plan &pl = m->plan;
    if (pl.sw.n_blocks > 0) return SM_ALGO_XBAND;                                  // column-swept blocks
    if (pl.band_slabs() == 1 && x16) return SM_ALGO_XBAND;                        // one slab of bands
    if (pl.cc.n_slices > 0) return SM_ALGO_SELL;                                    // column-chunked ELL
    if (pl.sell.n_slices > 0 && pl.sell.n_long == 0 && pl.hot.n_blocks == 0) return SM_ALGO_SELL;
    if (pl.max_row_nnz <= SM_SERIAL_ROW_MAX) return SM_ALGO_STREAM;                // serial rows only
    if (pl.xsell.n_slices > 0) return kAlgoExactSell;
    return SM_ALGO_PARITY;
}

// The unsegmented sliced ELL for SM_ALGO_EXACT (sm_build_opts.exact_sell): by default for
// matrices made by the CopyForm constructors -- the reference's own path, whose C++
// surface promises its results bit for bit -- when nothing else built keeps the order.
bool want_exact_sell(const sm_matrix *m) {
    if (m->nnz == 0 || m->n_rows == 0 || m->opts.exact_sell < 0) return false;
    if (m->opts.exact_sell == 0 && !m->from_index) return false;
    return exact_algo(m, true) == SM_ALGO_PARITY;
}

sm_status upload_exact_sell(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    // Rows never cut: the slice cap is the longest row (a lane walks its whole row).
    const int32_t cap = std::max<int32_t>(m->plan.max_row_nnz, 1);
    return upload_sell(m, rp, col, val, -1, false, &m->plan.xsell, cap);
}

// Column-chunked sorted sliced-ELL (ccsell.h, kernels_ccsell.hip):
// AUTO builds it instead of the sliced ELL when x is far larger than an XCD's L2
// (>= 2^23 columns = 32 MiB, 8 L2s' worth) and no band layout or relabeling serves
// the matrix -- a row-ordered ELL would gather every term's x from the Infinity Cache
// or HBM.  It declines (and the sliced ELL serves) when one row has more than 2048
// terms inside one column chunk.  ccsell = 0 / 1 never / always tries it.
// Column-swept row blocks (sweep.h, kernels_sweep.hip): forced by SM_LAYOUT_SWEEP.
bool want_sweep(const sm_matrix *m) {
    if (m->nnz == 0 || m->n_rows == 0 || m->plan.band()) return false;
    if (m->n_cols >= ((int64_t)1 << 30)) return false;   // 32-bit byte offsets into x
    return m->opts.layout == SM_LAYOUT_SWEEP;
}

sm_status upload_sweep(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    std::vector<float> table;
    std::vector<uint8_t> ids;
    const uint8_t *idp = nullptr;
    if (!codebook_source(m, val, m->nnz, table, ids, idp) || table.size() > 255) return SM_OK;   // not applicable
    SweepHost h;
    if (!sweep_build(rp, col, idp, m->n_rows, h)) return SM_OK;
    std::vector<uint8_t>().swap(ids);
    SweepDev &d = m->plan.sw;
    SM_TRY_HIP(dev_upload(m->mem, &d.d_block_chunk, h.block_chunk));
    SM_TRY_HIP(m->mem.alloc(&d.d_ent, std::max<int64_t>(1, h.n_chunks * 128)));
    SM_TRY_HIP(dev_upload_table(m->mem, &d.d_table, table.data(), (int32_t)table.size()));
    if (h.n_chunks)
        SM_TRY_HIP(hipMemcpy(d.d_ent, h.ent.data(), h.ent.size() * 4, hipMemcpyHostToDevice));
    d.table_size = (int32_t)table.size();
    d.n_chunks = h.n_chunks;
    d.n_blocks = h.n_blocks;
    return SM_OK;
}

bool want_ccsell(const sm_matrix *m) {
    if (m->opts.ccsell == 0 || m->opts.sell == 0) return false;
    if (m->nnz == 0 || m->n_rows == 0 || m->plan.band() || m->plan.n_relabel > 0 ||
        m->plan.sw.n_blocks > 0)
        return false;
    return m->opts.ccsell == 1 || m->n_cols >= ((int64_t)1 << 23);
}

sm_status upload_ccsell(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    const int32_t cl = m->opts.ccsell_chunk_log2 > 0 ? m->opts.ccsell_chunk_log2 : kCcDefaultChunkLog2;
    std::vector<float> table;
    std::vector<uint8_t> ids;
    const bool upd = m->opts.updatable != 0;   // the plain form: no decision reads the values
    const uint8_t *idp = nullptr;
    const bool cb = m->opts.sell_codebook != 0 && !upd && cl <= 24 && codebook_source(m, val, m->nnz, table, ids, idp);
    if (m->opts.table_updatable && !cb) return SM_OK;   // codebook form or none
    if (!cb) std::vector<uint8_t>().swap(ids);
    CcsellHost h;
    // SM_CCSELL_ROWORDER (development A/B): units in row order instead of by length.
    const char *ro = dev_env("SM_CCSELL_ROWORDER");
    const bool by_length = !(ro && atoi(ro) == 1);
    if (!ccsell_build(rp, col, val, cb ? idp : nullptr, m->n_rows, m->n_cols, cl, h, by_length, upd))
        return SM_OK;   // not applicable: the sliced ELL serves the matrix
    std::vector<uint8_t>().swap(ids);
    if (h.n_slices == 0) return SM_OK;
    CcsellDev &d = m->plan.cc;
    SM_TRY_HIP(dev_upload(m->mem, &d.d_off, h.off));           // n_slices
    SM_TRY_HIP(dev_upload(m->mem, &d.d_len, h.len));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_row, h.row));           // n_slices * kSellLanes
    SM_TRY_HIP(dev_upload(m->mem, &d.d_row_len, h.row_len));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_word, h.word));         // the padded slots
    if (cb) {
        SM_TRY_HIP(dev_upload_table(m->mem, &d.d_table, table.data(), (int32_t)table.size()));
        d.table_size = (int32_t)table.size();
    } else {
        SM_TRY_HIP(dev_upload(m->mem, &d.d_val, h.val));
    }
    if (const sm_status stm = upload_term_map(m, h.term, &d.d_term)) return stm;
    d.n_term = (int64_t)h.term.size();
    d.n_chunks = h.n_chunks;
    d.chunk_log2 = h.chunk_log2;
    d.chunk_slice = std::move(h.chunk_slice);
    d.n_slices = h.n_slices;
    return SM_OK;
}

// The reference's stream on the device (native.hip, SM_ALGO_NATIVE): each panel's run
// padded to start at a multiple of 16 bytes with (delta 0, id T) fillers, which the
// decode skips like the reference's own fillers -- so every 16-entry load is aligned.
sm_status upload_native(sm_matrix *m) {
    if (!m->has_ref || m->panel_col_off.empty() || m->table_size <= 0) return SM_OK;
    if (m->s_rows >= ((int64_t)1 << 23)) return SM_OK;   // in-panel offsets in int32
    const size_t P = m->panel_col_off.size();
    const size_t P_all = (size_t)((m->s_cols + 255) / 256);
    std::vector<uint8_t> pos, val;
    // Panels with entries first, then every 256-column block without one (an empty run):
    // a beta != 1 launch covers them all, since the kernel applies beta to the columns
    // it owns and the reference scales all of C (sparse-matrix.cc:149-151).
    std::vector<int64_t> beg(P, 0), end(P, 0);
    std::vector<int32_t> cols(m->panel_col_off.begin(), m->panel_col_off.end());
    {
        std::vector<char> has(P_all, 0);
        for (size_t p = 0; p < P; p++) has[(size_t)m->panel_col_off[p] / 256] = 1;
        for (size_t q = 0; q < P_all; q++)
            if (!has[q]) cols.push_back((int32_t)(q * 256));
        beg.resize(cols.size(), 0);
        end.resize(cols.size(), 0);
    }
    pos.reserve(m->pos.size() + 16 * P);
    val.reserve(m->pos.size() + 16 * P);
    for (size_t p = 0; p < P; p++) {
        while (pos.size() % 16) { pos.push_back(0); val.push_back((uint8_t)m->table_size); }
        beg[p] = (int64_t)pos.size();
        pos.insert(pos.end(), m->pos.begin() + m->panel_begin[p], m->pos.begin() + m->panel_end[p]);
        val.insert(val.end(), m->val.begin() + m->panel_begin[p], m->val.begin() + m->panel_end[p]);
        end[p] = (int64_t)pos.size();
    }
    NativeDev &d = m->plan.nat;
    SM_TRY_HIP(m->mem.alloc(&d.d_pos, (int64_t)pos.size() + 16));
    SM_TRY_HIP(m->mem.alloc(&d.d_val, (int64_t)val.size() + 16));
    const size_t Pc = cols.size();
    SM_TRY_HIP(dev_upload(m->mem, &d.d_beg, beg));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_end, end));
    SM_TRY_HIP(dev_upload(m->mem, &d.d_col, cols));
    SM_TRY_HIP(dev_upload_table(m->mem, &d.d_table, m->table.data(), m->table_size));
    SM_TRY_HIP(hipMemcpy(d.d_pos, pos.data(), pos.size(), hipMemcpyHostToDevice));
    SM_TRY_HIP(hipMemcpy(d.d_val, val.data(), val.size(), hipMemcpyHostToDevice));
    d.table_size = m->table_size;
    d.s_rows = m->s_rows;
    d.s_cols = m->s_cols;
    d.n_panels = (int32_t)P;
    d.n_all = (int32_t)Pc;
    // Batch metadata of the two-kernel form: the carry before each batch and the live
    // entries of each (batch, group) -- derived from the stream once, as the panel bounds are.
    std::vector<int32_t> pbatch(Pc + 1, 0), boff;
    std::vector<NatBatch> bmeta;
    int64_t live_total = 0;
    for (size_t p = 0; p < Pc; p++) {
        pbatch[p] = (int32_t)bmeta.size();
        int32_t carry = 0;
        for (int64_t e0 = beg[p]; e0 < end[p]; e0 += kNatBatchEntries) {
            const int64_t e1 = std::min<int64_t>(end[p], e0 + kNatBatchEntries);
            bmeta.push_back(NatBatch{e0, (int32_t)(e1 - e0), carry});
            int64_t live[4] = {0, 0, 0, 0};
            for (int64_t e = e0; e < e1; e++) {
                carry += pos[(size_t)e];
                if (val[(size_t)e] < m->table_size) live[(carry & 255) >> 6]++;
            }
            for (int g = 0; g < 4; g++) {
                boff.push_back((int32_t)live_total);
                live_total += live[g];
            }
        }
        d.max_panel_batches = std::max<int32_t>(d.max_panel_batches, (int32_t)bmeta.size() - pbatch[p]);
    }
    pbatch[Pc] = (int32_t)bmeta.size();
    d.n_batches = (int32_t)bmeta.size();
    if (live_total >= ((int64_t)1 << 31)) return SM_OK;   // fused kernel only
    if (d.n_batches > 0 && d.max_panel_batches > kNatFusedBatches) {
        SM_TRY_HIP(dev_upload(m->mem, &d.d_pbatch, pbatch));   // Pc + 1
        SM_TRY_HIP(dev_upload(m->mem, &d.d_bmeta, bmeta));     // n_batches
        SM_TRY_HIP(dev_upload(m->mem, &d.d_boff, boff));       // n_batches * 4
        SM_TRY_HIP(m->mem.alloc(&d.d_lists, std::max<int64_t>(live_total, 1)));
        SM_TRY_HIP(m->mem.alloc(&d.d_hdr, (int64_t)d.n_batches * 256));
    }
    return SM_OK;
}

// Skewed graphs (column relabeling built, e.g. R-MAT): the hottest
// relabeled columns [0, H) hold a large share of the terms in few columns, so they go
// through the codebook band kernel with their x staged in LDS (kernels_band2.hip) --
// no gathers -- and the sliced ELL gathers only the rest.  A row then adds its hot
// terms (in relabeled column order) before its cold ones (stored order): within the
// Sum|terms| bound, deterministic.  Opt-in only (hot_cols > 0 sets H; 0 and -1 never):
// measured on R-MAT scale 24 the split loses -- 2.71 ms at H = 32768, 2.16 ms at 8192,
// 4.55 ms at 131072 against 1.66 ms for the codebook sliced ELL alone (the band pass
// over 2^24 rows costs ~1.4 ms by itself; profiles/r03_rmat24_layout_ab.txt).
sm_status upload_sell_layouts(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val) {
    Plan &p = m->plan;
    const int64_t H0 = m->opts.hot_cols > 0 ? m->opts.hot_cols : 0;
    const bool try_hot = p.n_relabel > 0 && H0 > 0 && H0 < m->n_cols;
    if (!try_hot) return upload_sell(m, rp, col, val);
    const int64_t nnz = m->nnz, nr = m->n_rows;
    std::vector<int32_t> rcol((size_t)nnz);
    SM_TRY_HIP(hipMemcpy(rcol.data(), p.d_rcol, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    int64_t hot = 0;
    for (int64_t e = 0; e < nnz; e++) hot += rcol[(size_t)e] < H0;
    // Split every row into its hot part (sorted by relabeled column: the bands need
    // ascending columns) and its cold part (stored order).
    std::vector<int32_t> rph((size_t)nr + 1, 0), rpc((size_t)nr + 1, 0);
    std::vector<int32_t> ch((size_t)hot), cc((size_t)(nnz - hot));
    std::vector<float> vh((size_t)hot), vc((size_t)(nnz - hot));
    std::vector<std::pair<int32_t, float>> tmp;
    int64_t oh = 0, oc = 0;
    for (int64_t r = 0; r < nr; r++) {
        tmp.clear();
        for (int32_t e = rp[r]; e < rp[r + 1]; e++) {
            if (rcol[(size_t)e] < H0) {
                tmp.push_back({rcol[(size_t)e], val[e]});
            } else {
                cc[(size_t)oc] = rcol[(size_t)e];
                vc[(size_t)oc++] = val[e];
            }
        }
        std::sort(tmp.begin(), tmp.end(),
                  [](const std::pair<int32_t, float> &a, const std::pair<int32_t, float> &b) { return a.first < b.first; });
        for (const auto &t : tmp) {
            ch[(size_t)oh] = t.first;
            vh[(size_t)oh++] = t.second;
        }
        rph[(size_t)r + 1] = (int32_t)oh;
        rpc[(size_t)r + 1] = (int32_t)oc;
    }
    std::vector<int32_t>().swap(rcol);
    const size_t mark = m->mem.mark();
    if (const sm_status st = build_band2(m, p.hot, nr, H0, hot, rph.data(), ch.data(), vh.data(), kXbCband, 0, 0, true))
        return st;
    if (p.hot.n_blocks == 0 || p.hot.kind != kXbCband) {   // not applicable: sell serves all terms
        m->mem.release_since(mark);   // the matrix is as if the split was never tried
        p.hot = Band2Dev();
        return upload_sell(m, rp, col, val);
    }
    p.hot_cols = (int32_t)H0;
    std::vector<int32_t>().swap(ch);
    std::vector<float>().swap(vh);
    return upload_sell(m, rpc.data(), cc.data(), vc.data(), nnz - hot, true);
}

sm_status upload_plan(sm_matrix *m, const int32_t *rp_host) {
    PlanHost ph;
    int32_t tile = tile_nnz_setting(m);
    // Power-law rows (longest row > 64x the mean, e.g. R-MAT): 2048-term tiles
    // balance the workgroups better -- R-MAT scale 24: 2.34 ms vs 2.43 ms at 4096
    // (profiles/r01_rmat24_sweep.txt).  tile_nnz overrides.
    if (m->opts.tile_nnz == 0 && m->n_rows > 0) {
        int64_t longest = 0;
        for (int64_t r = 0; r < m->n_rows; r++)
            longest = std::max<int64_t>(longest, (int64_t)rp_host[r + 1] - rp_host[r]);
        if ((double)longest > 64.0 * (double)m->nnz / (double)m->n_rows) tile = 2048;
    }
    plan_rows(rp_host, m->n_rows, tile, kTileRows, kLongChunk, kSerialRowMax, ph);
    std::vector<Tile> tiles(ph.tiles.size());
    for (size_t i = 0; i < tiles.size(); i++)
        tiles[i] = Tile{ph.tiles[i].r0, ph.tiles[i].r1, ph.tiles[i].flags, 0};
    std::vector<Chunk> chunks(ph.chunks.size());
    for (size_t i = 0; i < chunks.size(); i++)
        chunks[i] = Chunk{ph.chunks[i].lr, ph.chunks[i].begin, ph.chunks[i].end, 0};
    Plan &p = m->plan;
    p.tile_nnz = tile;
    p.n_tiles = (int32_t)tiles.size();
    p.n_long = (int32_t)ph.long_rows.size();
    p.n_chunks = (int32_t)chunks.size();
    p.max_row_nnz = ph.max_row_nnz;
    p.avg_row_nnz = ph.avg_row_nnz;
    SM_TRY_HIP(dev_upload(m->mem, &p.d_tiles, tiles));
    if (m->n_rows > 0 && m->nnz > 0) {   // merge path (SM_ALGO_MERGE): slice corners, 32 B records
        const int64_t nb = merge_blocks(m->n_rows, m->nnz);
        std::vector<int32_t> corners;
        merge_corners(rp_host, m->n_rows, m->nnz, corners);
        SM_TRY_HIP(m->mem.alloc(&p.d_merge, nb));
        SM_TRY_HIP(m->mem.alloc(&p.d_merge_corner, nb + 1));
        SM_TRY_HIP(hipMemcpy(p.d_merge_corner, corners.data(), corners.size() * 4, hipMemcpyHostToDevice));
    }
    SM_TRY_HIP(dev_upload(m->mem, &p.d_chunks, chunks));
    SM_TRY_HIP(m->mem.alloc(&p.d_partials, p.n_chunks));
    SM_TRY_HIP(dev_upload(m->mem, &p.d_long_rows, ph.long_rows));   // n_long
    SM_TRY_HIP(dev_upload(m->mem, &p.d_long_ptr, ph.long_ptr));     // n_long + 1
    return SM_OK;
}

// Allocate the CSR arrays (col/val carry a zeroed tail of kPadElems for the
// aligned 16-byte loads of the stream kernel).
sm_status alloc_csr(sm_matrix *m) {
    SM_TRY_HIP(m->mem.alloc(&m->d_row_ptr, m->n_rows + 1));
    SM_TRY_HIP(m->mem.alloc(&m->d_col, m->nnz + kPadElems));
    SM_TRY_HIP(m->mem.alloc(&m->d_val, m->nnz + kPadElems));
    SM_TRY_HIP(hipMemset(m->d_col + m->nnz, 0, kPadElems * sizeof(int32_t)));
    SM_TRY_HIP(hipMemset(m->d_val + m->nnz, 0, kPadElems * sizeof(float)));
    return SM_OK;
}

// The host builders, in the one order both constructor tails run them: each want_* reads what
// was built before it.  `values(val)` makes the CSR values readable on the host at `val` before
// the first builder that stores them (the device tail fetches them then, once).  `ids` / `table`:
// a table matrix's own, on the host, which codebook_source hands a table_updatable matrix's
// builders; the matrix points at them for this call only.
template <class V>
static sm_status build_host_layouts(sm_matrix *m, const int32_t *rp, const int32_t *col, V &&values, bool exact_sell,
                                    const uint8_t *ids, const float *table) {
    sm_status st = SM_OK;
    const float *val = nullptr;
    m->build_ids = ids;
    m->build_table = table;
    if (st == SM_OK && want_xband(m)) st = values(val);
    if (st == SM_OK && want_xband(m)) st = upload_xband(m, rp, col, val, xband_kind_setting(m));
    if (st == SM_OK && want_sweep(m)) st = values(val);
    if (st == SM_OK && want_sweep(m)) st = upload_sweep(m, rp, col, val);
    if (st == SM_OK && want_relabel_size(m)) st = upload_relabel(m, col);
    if (st == SM_OK && want_ccsell(m)) st = values(val);
    if (st == SM_OK && want_ccsell(m)) st = upload_ccsell(m, rp, col, val);
    if (st == SM_OK && want_sell(m)) st = values(val);
    if (st == SM_OK && want_sell(m)) st = upload_sell_layouts(m, rp, col, val);
    if (st == SM_OK && want_merge_stage(m)) st = values(val);
    if (st == SM_OK && want_merge_stage(m)) st = upload_merge_stage(m, rp, col, val);
    if (st == SM_OK && exact_sell && want_exact_sell(m)) st = values(val);
    if (st == SM_OK && exact_sell && want_exact_sell(m)) st = upload_exact_sell(m, rp, col, val);
    m->build_ids = nullptr;
    m->build_table = nullptr;
    return st;
}

sm_status finish_from_host_csr(sm_matrix *m, const int32_t *rp, const int32_t *col, const float *val, const uint8_t *ids,
                               const float *table) {
    sm_status st = alloc_csr(m);
    if (st != SM_OK) return st;
    SM_TRY_HIP(hipMemcpy(m->d_row_ptr, rp, (size_t)(m->n_rows + 1) * 4, hipMemcpyHostToDevice));
    if (m->nnz) {
        SM_TRY_HIP(hipMemcpy(m->d_col, col, (size_t)m->nnz * 4, hipMemcpyHostToDevice));
        SM_TRY_HIP(hipMemcpy(m->d_val, val, (size_t)m->nnz * 4, hipMemcpyHostToDevice));
    }
    m->rows_ascend = true;
    for (int64_t r = 0; r < m->n_rows && m->rows_ascend; r++)
        for (int32_t e = rp[r] + 1; e < rp[r + 1]; e++)
            if (col[e - 1] >= col[e]) {
                m->rows_ascend = false;
                break;
            }
    st = upload_plan(m, rp);
    if (st != SM_OK) return st;
    return build_host_layouts(m, rp, col, [val](const float *&v) { v = val; return SM_OK; }, true, ids, table);
}

sm_status finish_from_device_csr(sm_matrix *m, hipStream_t s, bool exact_sell) {
    const int64_t n_rows = m->n_rows, n_cols = m->n_cols, nnz = m->nnz;
    sm_status st = SM_OK;
    int32_t flag = 0;
    std::vector<int32_t> rp((size_t)n_rows + 1);
    hipError_t e = hipSuccess;
    {
        DevScratch tmp;
        int32_t *d_flag = nullptr;
        e = tmp.alloc(&d_flag, 1);
        if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int32_t), s);
        if (e == hipSuccess)
            e = launch_validate((int32_t)n_rows, (int32_t)n_cols, (int32_t)nnz, m->d_row_ptr,
                                m->d_col, d_flag, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(rp.data(), m->d_row_ptr, rp.size() * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return hip_fail(e, "sm_create_from_csr_device");
    if (flag & kCsrInvalid) return fail(SM_ERR_INVALID_MATRIX, "device CSR failed validation (flags 0x%x)", flag & kCsrInvalid);
    m->rows_ascend = !(flag & kCsrNotAscending);
    st = upload_plan(m, rp.data());
    const bool xband = want_xband(m);
    // The column relabeling and the sorted sliced ELL on the device (builddev.hip) where they
    // are all this matrix wants: no band layout, sweep, hot split, windowed sort or exact sliced
    // ELL, and no column-chunked ELL once the relabeling is decided (its builder runs on the
    // host).  R-MAT 24: the host path took 5.4 s.
    bool dev_done = false;
    // An updatable matrix is built as host_build = 1: only the host builders emit the slot -> term maps.
    const bool dev_ok = st == SM_OK && m->opts.host_build == 0 && m->opts.updatable == 0 && m->opts.table_updatable == 0 &&
                        !want_sweep(m) &&
                        m->opts.hot_cols <= 0 &&
                        m->opts.sell_sigma == 0 && m->opts.sell_streams <= 1 && m->opts.exact_sell != 1;
    // The gathered chunk bands on the device (builddev_gcb.hip; config 5: 15 s on the host path).
    // Declined (a row's columns not ascending, size limits): the host path below decides.
    // A forced column relabeling (relabel = 1) is built beside the bands by the host path
    // only, so the device path is declined there too: the same bytes either way.
    if (dev_ok && xband && xband_kind_setting(m) == kXbGcb && m->opts.relabel != 1) {
        hipError_t eb = hipSuccess;
        int rows_log2 = 0;
        int32_t slabs = 1;
        gcb_geometry(m, rows_log2, slabs);
        GcbHost meta;
        const size_t mark = m->mem.mark();
        const int rc = devbuild_gcb(m, rows_log2, slabs, kGcbMaxWindow, meta, s, eb);
        if (rc < 0) st = hip_fail(eb, "device gcb builder");
        else if (rc == 0) {
            st = gcb_finish(m, meta);
            dev_done = st == SM_OK;
            if (dev_done) m->built_on_device |= SM_BUILT_DEV_GCB;
        } else {   // declined: nothing of the attempt stays
            m->mem.release_since(mark);
            m->plan.gcb = GcbDev();
        }
    }
    // The balanced bands on the device (builddev_band2.hip; config 2: 0.41 s on the host path),
    // with upload_xband's arguments.  Declined (a row's columns not strictly ascending, size
    // limits, bands under 70 % full, scratch out of memory): the host path below decides -- the
    // blocked kind or none, as before.  A band matrix wants no sliced ELL; one that wants the
    // unsegmented sliced ELL beside its bands keeps the host path.
    const XbKind b2kind = xband ? xband_kind_setting(m) : kXbExact;
    if (dev_ok && xband && (b2kind == kXbBand2 || b2kind == kXbCband) && m->opts.relabel != 1 &&
        (m->opts.band_tall == 0 || m->opts.band_tall == 4 || m->opts.band_tall == 6) &&
        !(exact_sell && want_exact_sell(m))) {
        hipError_t eb = hipSuccess;
        const int32_t p0 = m->opts.band_slab0_permille > 0 ? m->opts.band_slab0_permille : kB2Slab0Permille;
        Band2Host meta;
        std::vector<float> table;
        const size_t mark = m->mem.mark();
        const int rc = devbuild_band2(m, b2kind, m->opts.band_tall, band2_want_slabs(n_rows, m->opts.band_slabs),
                                      kind_forced(m), p0, meta, table, s, eb);
        if (rc < 0) st = hip_fail(eb, "device band2 builder");
        else if (rc == 0) {
            st = band2_finish(m, m->plan.b2, meta, table, n_rows);
            dev_done = st == SM_OK;
            if (dev_done) m->built_on_device |= SM_BUILT_DEV_BANDS;
        } else {   // declined: nothing of the attempt stays
            m->mem.release_since(mark);
            m->plan.b2 = Band2Dev();
        }
    }
    if (dev_ok && !xband) {
        hipError_t eb = hipSuccess;
        int rc = 0;
        if (want_relabel_size(m)) rc = devbuild_relabel(m, m->opts.relabel != 1, s, eb);
        uint32_t built = rc == 0 && m->plan.n_relabel > 0 ? SM_BUILT_DEV_RELABEL : 0;
        if (rc == 0 && !want_ccsell(m)) {
            if (want_sell(m)) {
                const int32_t max_len = m->opts.sell_max_len > 0 ? m->opts.sell_max_len : kSellMaxLen;
                rc = devbuild_sell(m, max_len, m->opts.sell_codebook != 0, s, eb);
                if (rc == 0 && m->plan.sell.n_slices > 0) built |= SM_BUILT_DEV_SELL;
            }
            dev_done = rc == 0;
        }
        if (dev_done) m->built_on_device |= built;
        if (rc != 0) st = hip_fail(eb, "device layout builder");
    }
    // The merge path's staging copy (sm_build_opts.merge_stage) after a device build too
    // (R-MAT 24: 7.7 s on the host path).
    if (st == SM_OK && dev_done && want_merge_stage(m)) {
        hipError_t eb = hipSuccess;
        if (devbuild_merge_stage(m, s, eb) < 0) st = hip_fail(eb, "device merge staging builder");
        else if (m->plan.d_mstage_w) m->built_on_device |= SM_BUILT_DEV_MERGE_STAGE;
    }
    const bool maybe_sell = m->opts.sell != 0 && nnz > 0;
    const bool maybe_xsell = exact_sell && nnz > 0 && n_rows > 0 && (m->opts.exact_sell == 1 || (m->opts.exact_sell == 0 && m->from_index));
    // The other band kinds, and whatever the device builders declined or the options keep from
    // them, are built on the host (band2.cpp, xband.cpp, sell.cpp): the
    // columns come down for any of them, the values only for the layout that stores
    // them (4 + 4 bytes per term over PCIe once, at creation).
    if (st == SM_OK && !dev_done &&
        (xband || want_relabel_size(m) || maybe_sell || maybe_xsell || want_sweep(m) || want_merge_stage(m))) {
        std::vector<int32_t> ch((size_t)nnz);
        std::vector<float> vh;
        auto values = [&](const float *&v) -> sm_status {
            if (vh.size() != (size_t)nnz) {
                vh.resize((size_t)nnz);
                const hipError_t ev = hipMemcpy(vh.data(), m->d_val, (size_t)nnz * 4, hipMemcpyDeviceToHost);
                if (ev != hipSuccess) return hip_fail(ev, "copy CSR values for the layout builder");
            }
            v = vh.data();
            return SM_OK;
        };
        hipError_t e3 = hipSuccess;
        if (nnz) e3 = hipMemcpy(ch.data(), m->d_col, (size_t)nnz * 4, hipMemcpyDeviceToHost);
        st = e3 == hipSuccess ? SM_OK : hip_fail(e3, "copy CSR columns for the layout builder");
        // A table_updatable matrix's builders take its own ids and table (codebook_source): 1 byte
        // per term and the table come down once; `s` is synchronised above.
        std::vector<uint8_t> h_ids;
        std::vector<float> h_tab;
        if (st == SM_OK && m->is_table && m->opts.table_updatable) {
            h_ids.resize((size_t)nnz);
            h_tab.resize(256);
            if (nnz) e3 = hipMemcpy(h_ids.data(), m->d_tab_ids, (size_t)nnz, hipMemcpyDeviceToHost);
            if (e3 == hipSuccess) e3 = hipMemcpy(h_tab.data(), m->d_tab, 256 * sizeof(float), hipMemcpyDeviceToHost);
            if (e3 != hipSuccess) st = hip_fail(e3, "copy the table and its ids for the layout builder");
        }
        if (st == SM_OK) st = build_host_layouts(m, rp.data(), ch.data(), values, exact_sell, h_ids.data(), h_tab.data());
    }
    return st;
}

}  // namespace smamd
