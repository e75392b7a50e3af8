// capi.cpp -- the extern "C" boundary of libsparsematrix_amd.so
// (include/sparsematrix.h), but for the constructors (create.cpp).  Host-side C++: error
// reporting, what a matrix tells about itself, copies, and the argument checks and kernel
// dispatch of the products and updates; what decides and builds a matrix's layouts is
// layouts.cpp.  All arithmetic runs in the HIP kernels of kernels.hip; there is no CPU compute path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "capi_util.h"
#include "gcb.h"
#include "sm_internal.h"
#include "sell.h"
#include "xband.h"

using namespace smamd;

namespace {
thread_local std::string g_err;   // sm_last_error
}

namespace smamd {

sm_status fail(sm_status s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return s;
}

hipError_t after_launch(hipError_t e, hipStream_t s, const char *what) {
    static const bool debug_sync = [] {
        const char *v = getenv("SM_DEBUG_SYNC");
        return v && atoi(v) != 0;
    }();
    if (e != hipSuccess || !debug_sync) return e;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) fprintf(stderr, "[sparsematrix_amd] %s failed: %s\n", what, hipGetErrorString(e));
    return e;
}

}  // namespace smamd

// Everything the matrix owns on its device: the recorded buffers, the AddMatMat workspace and
// the events.
sm_matrix::~sm_matrix() {
    DeviceGuard g(device);
    mem.release_all();
    dev_free_uncounted(d_ws);
    for (hipEvent_t ev : {ws_ready, scratch_turn.ready, table_turn.ready})
        if (ev) (void)hipEventDestroy(ev);
}

namespace {

const char *kNotTable = "not a table matrix (sm_create_from_csr_ids)";
const char *kIndexHint = "a dense-index matrix is not a table matrix: build it with sm_create_from_csr_ids from "
                         "(row_ptr, col_idx, ids, table), see INTEGRATION.md";
sm_status need_table(const sm_matrix *m, const char *what) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (!m->is_table) return fail(SM_ERR_NOT_SUPPORTED, "%s: %s", what, m->from_index ? kIndexHint : kNotTable);
    return SM_OK;
}

// The native form's two-kernel path keeps its column lists in the matrix (scratch_turn).
bool native_scratch(const NativeDev &nd) { return nd.d_lists && nd.max_panel_batches > kNatFusedBatches; }

// FNV-1a over device arrays (sm_layout_digest).
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void *p, size_t n) {
        const uint8_t *b = static_cast<const uint8_t *>(p);
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    }
};
template <class T>
sm_status fnv_dev(Fnv &f, const T *d, int64_t n) {
    if (!d || n <= 0) return SM_OK;
    std::vector<T> h((size_t)n);
    const hipError_t e = hipMemcpy(h.data(), d, (size_t)n * sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "sm_layout_digest");
    f.add(h.data(), h.size() * sizeof(T));
    return SM_OK;
}
}  // namespace

extern "C" {

const char *sm_version(void) { return "sparsematrix_amd 0.2 (gfx950)"; }

const char *sm_status_string(sm_status s) {
    switch (s) {
    case SM_OK: return "ok";
    case SM_ERR_INVALID_ARG: return "invalid argument";
    case SM_ERR_OUT_OF_MEMORY: return "out of memory";
    case SM_ERR_HIP: return "HIP runtime error";
    case SM_ERR_NOT_SUPPORTED: return "not supported";
    case SM_ERR_TOO_LARGE: return "too large for int32 indexing";
    case SM_ERR_INVALID_MATRIX: return "invalid matrix";
    case SM_ERR_NO_DEVICE: return "no HIP device";
    }
    return "unknown status";
}

const char *sm_last_error(void) { return g_err.c_str(); }

sm_status sm_device_count(int32_t *count) {
    if (!count) return fail(SM_ERR_INVALID_ARG, "count is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n ? SM_OK : fail(SM_ERR_NO_DEVICE, "no HIP device visible");
}

void sm_destroy(sm_matrix *m) { delete m; }

sm_status sm_get_info(const sm_matrix *m, sm_info *info) {
    return sm_get_info_ex(m, info, sizeof(sm_info));
}

sm_status sm_debug_seed_handoff(sm_matrix *m, uint64_t started) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    const Band2Dev &xb = m->plan.b2;
    if (xb.n_blocks <= 0 || xb.n_slabs < 2 || !xb.d_tickets)
        return fail(SM_ERR_NOT_SUPPORTED, "no multi-slab band2/cband layout");
    if (started % (uint64_t)xb.n_slabs != 0)
        return fail(SM_ERR_NOT_SUPPORTED, "started must be a multiple of the slab count");
    DeviceGuard g(m->device);
    // Control words per block (xband_dev.h slab_handoff_epoch): [0..1] started, [2..3] arrive.
    std::vector<int32_t> h((size_t)xb.n_blocks * 4, 0);
    for (int32_t b = 0; b < xb.n_blocks; ++b) memcpy(&h[(size_t)b * 4], &started, 8);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(xb.d_tickets, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_debug_seed_handoff");
}

sm_status sm_get_info_ex(const sm_matrix *m, sm_info *out, size_t info_bytes) {
    if (!m || !out) return fail(SM_ERR_INVALID_ARG, "null argument");
    sm_info full;
    memset(&full, 0, sizeof(full));
    sm_info *info = &full;
    info->s_rows = m->s_rows;
    info->s_cols = m->s_cols;
    info->n_rows = m->n_rows;
    info->n_cols = m->n_cols;
    info->nnz = m->nnz;
    info->table_size = m->is_table ? m->tab_size : m->table_size;
    info->has_ref_stream = m->has_ref ? 1 : 0;
    info->n_entries = (int64_t)m->pos.size();
    info->n_panels = (int64_t)m->panel_col_off.size();
    info->device = m->device;
    info->n_tiles = m->plan.n_tiles;
    info->n_long_rows = m->plan.n_long;
    info->max_row_nnz = m->plan.max_row_nnz;
    if (const BandTiles *b = m->plan.band()) {
        info->has_xband = b->kind;
        info->xband_blocks = b->n_blocks;
        info->xband_bands = b->n_bands;
        info->xband_slabs = b->n_slabs;
        info->xband_block_rows = b->block_rows;
    }
    info->xband_slab_cols = m->plan.band_slab_cols();
    info->xband_slab0_cols = m->plan.band_slab0_cols();
    info->merge_stage = m->plan.d_mstage_w ? 1 : 0;
    info->xband_beta_last = SM_B2_BL && m->plan.b2.n_blocks > 0 && m->plan.b2.n_slabs > 1;
    info->device_bytes = m->mem.bytes;
    info->updatable = m->opts.updatable ? 1 : 0;
    info->table_updatable = m->opts.table_updatable ? 1 : 0;
    info->col_relabel = m->plan.n_relabel > 0 ? 1 : 0;
    info->sell_slices = m->plan.sell.n_slices;
    info->sell_codebook = m->plan.sell.d_table != nullptr || m->plan.cc.d_table != nullptr;
    info->ccsell_chunks = m->plan.cc.n_slices > 0 ? m->plan.cc.n_chunks : 0;
    info->hot_cols = m->plan.hot.n_blocks > 0 ? m->plan.hot_cols : 0;
    info->sweep_blocks = (int32_t)std::min<int64_t>(m->plan.sw.n_blocks, INT32_MAX);
    info->exact_sell_slices = m->plan.xsell.n_slices;
    {
        const int a = exact_algo(m, true);
        info->exact_algo = a == kAlgoExactSell ? (int32_t)SM_ALGO_SELL : a;
    }
    // Only the bytes the caller's struct has (an older, shorter sm_info stays valid).
    memcpy(out, &full, std::min(info_bytes, sizeof(full)));
    return SM_OK;
}

sm_status sm_layout_digest(const sm_matrix *m, uint64_t digest[4]) {
    if (!m || !digest) return fail(SM_ERR_INVALID_ARG, "null argument");
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    for (int k = 0; k < 4; k++) digest[k] = 0;
    const Plan &p = m->plan;
    sm_status st = SM_OK;
    if (p.n_relabel > 0) {
        Fnv f;
        if ((st = fnv_dev(f, p.d_perm, p.n_relabel)) != SM_OK) return st;
        if ((st = fnv_dev(f, p.d_rcol, m->nnz)) != SM_OK) return st;
        digest[0] = f.h;
    }
    const GcbDev &gb = p.gcb;
    if (gb.n_blocks > 0) {   // gathered chunk bands (gcb.h)
        const int64_t ntile = (int64_t)gb.n_blocks * gb.n_slabs;
        Fnv f;
        const int32_t geo[5] = {gb.block_rows, gb.window, gb.n_blocks, gb.n_slabs, gb.slab_cols};
        f.add(geo, sizeof(geo));
        if ((st = fnv_dev(f, gb.d_tile_band, ntile + 1)) != SM_OK) return st;
        if ((st = fnv_dev(f, gb.d_band_clo, gb.n_bands)) != SM_OK) return st;
        digest[1] = f.h;
        Fnv w;
        if ((st = fnv_dev(w, gb.d_ent, (int64_t)gb.n_bands * kGcbBandWords)) != SM_OK) return st;
        digest[2] = w.h;
    }
    const SellDev &d = p.sell;
    const Band2Dev &b2 = p.b2;
    bool b2_table = false;
    if (b2.n_blocks > 0 && d.n_slices == 0) {   // balanced bands (xband.h Band2Host), no sliced ELL beside them
        const int64_t ntile = (int64_t)b2.n_blocks * b2.n_slabs;
        const bool cb = b2.kind == kXbCband;
        Fnv f;
        const int32_t geo[7] = {b2.kind, b2.block_rows, b2.window, b2.n_blocks, b2.n_slabs, b2.slab_cols, b2.slab0_cols};
        f.add(geo, sizeof(geo));
        if ((st = fnv_dev(f, b2.d_tile_band, ntile + 1)) != SM_OK) return st;
        if ((st = fnv_dev(f, b2.d_band_clo, b2.n_bands)) != SM_OK) return st;
        digest[1] = f.h;
        // entry words per band: the window tells the geometry (dma3: 30 chunks, wide: 32)
        const int64_t chunks = b2.window == kB2Wide.window ? kB2Wide.chunks() : kB2Dma3Cb.chunks();
        Fnv w;
        if ((st = fnv_dev(w, b2.d_ent, (int64_t)b2.n_bands * chunks * (cb ? 64 : 128))) != SM_OK) return st;
        digest[2] = w.h;
        b2_table = cb && b2.d_table;
    }
    if (d.n_slices > 0) {
        std::vector<int64_t> off((size_t)d.n_slices);
        std::vector<int32_t> len((size_t)d.n_slices);
        SM_TRY_HIP(hipMemcpy(off.data(), d.d_off, off.size() * 8, hipMemcpyDeviceToHost));
        SM_TRY_HIP(hipMemcpy(len.data(), d.d_len, len.size() * 4, hipMemcpyDeviceToHost));
        const int64_t padded = off.back() + (int64_t)len.back() * kSellLanes;
        Fnv f;
        f.add(off.data(), off.size() * 8);
        f.add(len.data(), len.size() * 4);
        if ((st = fnv_dev(f, d.d_row, d.n_slices * kSellLanes)) != SM_OK) return st;
        if ((st = fnv_dev(f, d.d_row_len, d.n_slices * kSellLanes)) != SM_OK) return st;
        f.add(&d.n_long, 4);
        f.add(&d.max_len, 4);
        if ((st = fnv_dev(f, d.d_long_rows, d.n_long)) != SM_OK) return st;
        if ((st = fnv_dev(f, d.d_long_ptr, d.n_long > 0 ? d.n_long + 1 : 0)) != SM_OK) return st;
        digest[1] = f.h;
        Fnv c;
        if ((st = fnv_dev(c, d.d_col, padded + 32 * kSellLanes)) != SM_OK) return st;
        if ((st = fnv_dev(c, d.d_val, d.d_val ? padded + 32 * kSellLanes : 0)) != SM_OK) return st;
        digest[2] = c.h;
    }
    Fnv t;   // [3]: the sliced ELL's codebook, then the merge staging copy
    bool any = false;
    if (d.n_slices > 0 && d.d_table) {
        if ((st = fnv_dev(t, d.d_table, d.table_size)) != SM_OK) return st;
        t.add(&d.table_size, 4);
        any = true;
    }
    if (b2_table) {
        if ((st = fnv_dev(t, b2.d_table, 256)) != SM_OK) return st;
        t.add(&b2.table_size, 4);
        any = true;
    }
    if (p.d_mstage_w) {
        if ((st = fnv_dev(t, p.d_mstage_w, m->nnz)) != SM_OK) return st;
        if ((st = fnv_dev(t, p.d_mstage_z, m->nnz)) != SM_OK) return st;
        if ((st = fnv_dev(t, p.d_mstage_tab, 256)) != SM_OK) return st;
        any = true;
    }
    if (any) digest[3] = t.h;
    return SM_OK;
}

sm_status sm_built_on_device(const sm_matrix *m, uint32_t *mask) {
    if (!m || !mask) return fail(SM_ERR_INVALID_ARG, "null argument");
    *mask = m->built_on_device;
    return SM_OK;
}

int32_t sm_num_rows(const sm_matrix *m) { return m ? (int32_t)m->s_rows : 0; }
int32_t sm_num_cols(const sm_matrix *m) { return m ? (int32_t)m->s_cols : 0; }

sm_status sm_copy_ref_stream(const sm_matrix *m, uint8_t *pos, uint8_t *val, int32_t *pro,
                             int32_t *pco, int64_t *pb, int64_t *pe) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (!m->has_ref) return fail(SM_ERR_NOT_SUPPORTED, "matrix holds no reference encoding");
    if (pos && !m->pos.empty()) memcpy(pos, m->pos.data(), m->pos.size());
    if (val && !m->val.empty()) memcpy(val, m->val.data(), m->val.size());
    const size_t P = m->panel_col_off.size();
    if (pro && P) memcpy(pro, m->panel_row_off.data(), P * 4);
    if (pco && P) memcpy(pco, m->panel_col_off.data(), P * 4);
    if (pb && P) memcpy(pb, m->panel_begin.data(), P * 8);
    if (pe && P) memcpy(pe, m->panel_end.data(), P * 8);
    return SM_OK;
}

sm_status sm_copy_csr(const sm_matrix *m, int32_t *row_ptr, int32_t *col_idx, float *val) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    DeviceGuard g(m->device);
    if (row_ptr)
        SM_TRY_HIP(hipMemcpy(row_ptr, m->d_row_ptr, (size_t)(m->n_rows + 1) * 4, hipMemcpyDeviceToHost));
    if (col_idx && m->nnz)
        SM_TRY_HIP(hipMemcpy(col_idx, m->d_col, (size_t)m->nnz * 4, hipMemcpyDeviceToHost));
    if (val && m->nnz)
        SM_TRY_HIP(hipMemcpy(val, m->d_val, (size_t)m->nnz * 4, hipMemcpyDeviceToHost));
    return SM_OK;
}

sm_status sm_to_dense(const sm_matrix *m, float *out, int32_t stride, sm_trans trans) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (trans != SM_NO_TRANS && trans != SM_TRANS) return fail(SM_ERR_INVALID_ARG, "bad trans");
    // NoTrans: S, s_rows x stride (s_cols used); Trans: S^T = B, s_cols x stride (s_rows used)
    const int64_t out_rows = trans == SM_TRANS ? m->s_cols : m->s_rows;
    const int64_t width = trans == SM_TRANS ? m->s_rows : m->s_cols;
    if (out_rows == 0) return SM_OK;
    if (!out || stride < width) return fail(SM_ERR_INVALID_ARG, "null out or stride < %lld", (long long)width);
    DeviceGuard g(m->device);
    const size_t bytes = (size_t)out_rows * stride * sizeof(float);
    DevScratch tmp;
    float *d = nullptr;
    SM_TRY_HIP(tmp.alloc(&d, (int64_t)out_rows * stride));
    hipError_t e = hipMemsetAsync(d, 0, bytes, 0);
    if (e == hipSuccess)
        e = launch_scatter_dense((int32_t)m->n_rows, m->d_row_ptr, m->d_col, m->d_val, d, stride,
                                 trans == SM_TRANS, 0);
    if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "sm_to_dense");
    return SM_OK;
}

// The exit of the pipeline: sm_to_dense's orientations into a device buffer, asynchronously, the
// matrix only read and nothing allocated.
sm_status sm_to_dense_device(const sm_matrix *m, float *d_out, int64_t ld, sm_trans trans, sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (trans != SM_NO_TRANS && trans != SM_TRANS) return fail(SM_ERR_INVALID_ARG, "bad trans");
    const int64_t out_rows = trans == SM_TRANS ? m->s_cols : m->s_rows;
    const int64_t width = trans == SM_TRANS ? m->s_rows : m->s_cols;
    if (out_rows == 0 || width == 0) return SM_OK;
    if (!d_out) return fail(SM_ERR_INVALID_ARG, "sm_to_dense_device: null output");
    if (ld < width) return fail(SM_ERR_INVALID_ARG, "sm_to_dense_device: ld %lld < %lld", (long long)ld, (long long)width);
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_dense_zero(d_out, out_rows, width, ld, s);
    if (e == hipSuccess && m->nnz > 0)
        e = m->rows_ascend ? launch_scatter_terms((int32_t)m->n_rows, m->nnz, m->d_row_ptr, m->d_col, m->d_val, d_out, ld,
                                                  trans == SM_TRANS, s)
                           : launch_scatter_dense((int32_t)m->n_rows, m->d_row_ptr, m->d_col, m->d_val, d_out, ld,
                                                  trans == SM_TRANS, s);
    if (e != hipSuccess) return hip_fail(e, "sm_to_dense_device");
    return SM_OK;
}

int32_t sm_equal(const sm_matrix *a, const sm_matrix *b) {
    if (!a || !b) return 0;
    if (a == b) return 1;
    if (a->s_rows != b->s_rows || a->s_cols != b->s_cols || a->nnz != b->nnz) return 0;
    if (a->has_ref && b->has_ref) {
        // the reference's own member-wise comparison (sparse-matrix.cc:197-207)
        if (a->table.size() != b->table.size() ||
            memcmp(a->table.data(), b->table.data(), a->table.size() * 4) != 0)
            return 0;
        return a->pos == b->pos && a->val == b->val && a->panel_row_off == b->panel_row_off &&
               a->panel_col_off == b->panel_col_off && a->panel_begin == b->panel_begin &&
               a->panel_end == b->panel_end;
    }
    std::vector<int32_t> ra((size_t)a->n_rows + 1), rb((size_t)b->n_rows + 1);
    std::vector<int32_t> ca((size_t)a->nnz), cb((size_t)b->nnz);
    std::vector<float> va((size_t)a->nnz), vb((size_t)b->nnz);
    if (sm_copy_csr(a, ra.data(), ca.data(), va.data()) != SM_OK) return 0;
    if (sm_copy_csr(b, rb.data(), cb.data(), vb.data()) != SM_OK) return 0;
    return ra == rb && ca == cb &&
           (va.empty() || memcmp(va.data(), vb.data(), va.size() * 4) == 0);
}

// ---------------------------------------------------------------------------

// The launches of one SpMV by the algorithm `ai` (an sm_algo other than NATIVE / EXACT / MFMA,
// or kAlgoExactSell), alpha != 0.
static hipError_t launch_spmv_algo(const sm_matrix *m, int ai, float alpha, const float *x, float beta, float *y,
                                   hipStream_t s) {
    const int32_t n = (int32_t)m->n_rows;
    hipError_t e = hipSuccess;
    switch (ai) {
    case SM_ALGO_PARITY:
        e = launch_spmv_parity(n, m->d_row_ptr, m->d_col, m->d_val, x, y, alpha, beta, s);
        break;
    case SM_ALGO_VECTOR:
        e = launch_spmv_vector(n, m->plan.avg_row_nnz, m->d_row_ptr, m->d_col, m->d_val, x, y,
                               alpha, beta, s);
        break;
    case SM_ALGO_AUTO:
    case SM_ALGO_XBAND:
        if (m->plan.sw.n_blocks > 0) {   // column-swept row blocks: no scratch, bit-identical
            e = launch_spmv_sweep(m->plan.sw, n, (int32_t)m->n_cols, x, y, alpha, beta, s);
            break;
        }
        if (m->plan.band() && ((uintptr_t)x % 16) == 0) {
            e = launch_spmv_band(m->plan, n, (int32_t)m->n_cols, x, y, alpha, beta, s);
            break;
        }
        // fall through: no band layout (or unaligned x) -> sell or stream kernel
        [[fallthrough]];
    case SM_ALGO_SELL:
        if (m->plan.cc.n_slices > 0) {   // column-chunked: no scratch, y read and written per chunk
            e = launch_spmv_ccsell(m->plan.cc, x, y, alpha, beta, s);
            break;
        }
        if (m->plan.sell.n_slices > 0) {
            const float *xs = x;
            if (m->plan.n_relabel > 0) {   // the slices hold relabeled columns
                e = launch_x_relabel(m->plan.n_relabel, m->plan.d_perm, x, m->plan.d_xperm, s);
                xs = m->plan.d_xperm;
            }
            float b = beta;
            if (e == hipSuccess && m->plan.hot.n_blocks > 0) {   // hot columns first, then the rest
                e = launch_spmv_band2(m->plan.hot, n, m->plan.hot_cols, xs, y, alpha, beta, s);
                b = 1.0f;
            }
            if (e == hipSuccess) e = launch_spmv_sell(m->plan.sell, xs, y, alpha, b, s);
            break;
        }
        [[fallthrough]];   // no sell layout -> stream kernel
    case SM_ALGO_STREAM:
        // Long-row partial sums (and the relabeled x) live in the matrix (allocated at
        // creation): SpMVs on one matrix must not run concurrently on different streams.
        if (m->plan.n_relabel > 0) {
            e = launch_x_relabel(m->plan.n_relabel, m->plan.d_perm, x, m->plan.d_xperm, s);
            if (e == hipSuccess)
                e = launch_spmv_stream(m->plan, m->d_row_ptr, m->plan.d_rcol, m->d_val,
                                       m->plan.d_xperm, y, alpha, beta, m->plan.d_partials, s);
            break;
        }
        e = launch_spmv_stream(m->plan, m->d_row_ptr, m->d_col, m->d_val, x, y, alpha, beta,
                               m->plan.d_partials, s);
        break;
    case SM_ALGO_MERGE: {   // merge path over the CSR arrays (kernels_merge.hip)
        const MergeStage mstage{m->plan.d_mstage_w, m->plan.d_mstage_z, m->plan.d_mstage_tab};
        if (m->plan.n_relabel > 0) {   // skewed columns: the relabeled copy, hot x in L2 (as stream)
            e = launch_x_relabel(m->plan.n_relabel, m->plan.d_perm, x, m->plan.d_xperm, s);
            if (e == hipSuccess)
                e = launch_spmv_merge(n, (int32_t)m->nnz, m->d_row_ptr, m->plan.d_rcol, m->d_val, m->plan.d_xperm, y,
                                      alpha, beta, m->plan.d_merge_corner, m->plan.d_merge, s, &mstage);
            break;
        }
        e = launch_spmv_merge(n, (int32_t)m->nnz, m->d_row_ptr, m->d_col, m->d_val, x, y, alpha, beta,
                              m->plan.d_merge_corner, m->plan.d_merge, s, &mstage);
        break;
    }
    case kAlgoExactSell: {   // unsegmented slices: every row in stored order, one lane each
        const float *xs = x;
        if (m->plan.n_relabel > 0) {   // the slices hold relabeled columns
            e = launch_x_relabel(m->plan.n_relabel, m->plan.d_perm, x, m->plan.d_xperm, s);
            xs = m->plan.d_xperm;
        }
        if (e == hipSuccess) e = launch_spmv_sell(m->plan.xsell, xs, y, alpha, beta, s);
        break;
    }
    default:   // (not reached: `ai` was checked above)
        e = hipErrorInvalidValue;
    }
    return e;
}

// Whether launch_spmv_algo(m, ai, ...) takes a turn on the matrix's SpMV scratch (sm_internal.h):
// SpMVs that do run one after the other on the device, whatever stream or thread issues them.
// Deliberately a superset of what the route launches: any built layout that has scratch owned
// by the matrix counts (slab partials, the relabeled x, long-row partials), used by `ai` or not.
static bool spmv_takes_turn(const Plan &pl, int ai) {
    if (ai == SM_ALGO_MERGE) return true;
    if (ai == SM_ALGO_PARITY || ai == SM_ALGO_VECTOR) return false;
    return pl.band_slabs() > 1 || pl.n_relabel > 0 || (pl.hot.n_blocks > 0 && pl.hot.n_slabs > 1) ||
           pl.sell.n_long > 0 || pl.n_long > 0;
}

sm_status sm_spmv(const sm_matrix *m, float alpha, const float *x, float beta, float *y,
                  sm_algo algo, sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (m->n_rows == 0) return SM_OK;
    if (!y || (alpha != 0.0f && m->n_cols > 0 && !x)) return fail(SM_ERR_INVALID_ARG, "null x/y");
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    const int32_t n = (int32_t)m->n_rows;
    hipError_t e = hipSuccess;
    if (alpha == 0.0f) {   // sparse-matrix.cc:149-152: only the beta pass
        if (beta != 1.0f) e = launch_beta(y, 1, n, n, beta, s);
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmv beta");
    }
    if (algo == SM_ALGO_NATIVE) {   // the reference stream: y = x * S (a = x, c = y, m = 1)
        if (!m->has_ref || (m->plan.nat.n_panels == 0 && m->nnz > 0))
            return fail(SM_ERR_NOT_SUPPORTED, "SM_ALGO_NATIVE needs a matrix built from the dense index");
        e = m->plan.nat.n_panels == 0
                ? (beta != 1.0f ? launch_beta(y, 1, n, n, beta, s) : hipSuccess)
                : with_turn(m->scratch_turn, s, native_scratch(m->plan.nat), [&] {
                      return launch_native_addmatmat(m->plan.nat, 1, x, (int32_t)m->n_cols, y, n, alpha,
                                                     beta, s);
                  });
        e = after_launch(e, s, "sm_spmv native");
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmv native");
    }
    if (algo == SM_ALGO_MFMA) return fail(SM_ERR_NOT_SUPPORTED, "SM_ALGO_MFMA is an SpMM algorithm (n_rhs = 32)");
    const int ai = algo == SM_ALGO_EXACT ? exact_algo(m, ((uintptr_t)x % 16) == 0) : (int)algo;
    if ((ai < SM_ALGO_AUTO || ai > SM_ALGO_SELL) && ai != kAlgoExactSell && ai != SM_ALGO_MERGE)
        return fail(SM_ERR_INVALID_ARG, "unknown algo %d", (int)algo);
    e = with_turn(m->scratch_turn, s, spmv_takes_turn(m->plan, ai),
                  [&] { return launch_spmv_algo(m, ai, alpha, x, beta, y, s); });
    e = after_launch(e, s, "sm_spmv");
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmv launch");
}

sm_status sm_spmm(const sm_matrix *m, int32_t n_rhs, float alpha, const float *X, int64_t ldx,
                  float beta, float *Y, int64_t ldy, sm_algo algo, sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (n_rhs < 0) return fail(SM_ERR_INVALID_ARG, "n_rhs < 0");
    if (m->n_rows == 0 || n_rhs == 0) return SM_OK;
    if (ldy < n_rhs || ldx < n_rhs) return fail(SM_ERR_INVALID_ARG, "ldx/ldy < n_rhs");
    if (!Y || (alpha != 0.0f && m->n_cols > 0 && !X)) return fail(SM_ERR_INVALID_ARG, "null X/Y");
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    const int32_t n = (int32_t)m->n_rows;
    hipError_t e;
    if (alpha == 0.0f) {
        e = beta != 1.0f ? launch_beta(Y, n, n_rhs, ldy, beta, s) : hipSuccess;
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmm beta");
    }
    if (algo == SM_ALGO_MFMA) {   // the matrix-core SpMM (spmm_mfma.hip)
        if (n_rhs != 32 || ldx % 2 || ldy % 2 || ((uintptr_t)X % 8) || ((uintptr_t)Y % 8) ||
            (uint64_t)m->n_cols * (uint64_t)ldx * 4u >= 0xFFFFFFF0ull ||
            (uint64_t)m->nnz * 4u >= 0xFFFFFFF0ull)
            return fail(SM_ERR_NOT_SUPPORTED, "SM_ALGO_MFMA needs n_rhs = 32, even ldx/ldy, 8-byte "
                        "aligned X/Y, and X and the term arrays under 4 GiB");
        e = launch_spmm_mfma(n, m->d_row_ptr, m->d_col, m->d_val, (int32_t)m->nnz, X, ldx, m->n_cols,
                             Y, ldy, alpha, beta, s);
        e = after_launch(e, s, "sm_spmm mfma");
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmm mfma");
    }
    const bool vec_ok = n_rhs % 4 == 0 && n_rhs <= 128 && ldx % 4 == 0 && ldy % 4 == 0 &&
                        ((uintptr_t)X % 16) == 0 && ((uintptr_t)Y % 16) == 0;
    if (algo == SM_ALGO_SELL || algo == SM_ALGO_XBAND || algo == SM_ALGO_EXACT || algo == SM_ALGO_MERGE)
        algo = SM_ALGO_AUTO;   // SpMV layouts; the SpMM kernels keep every row's order
    if ((algo == SM_ALGO_AUTO || algo == SM_ALGO_STREAM || algo == SM_ALGO_VECTOR) && vec_ok)
        e = launch_spmm_rowpanel(n, n_rhs, m->d_row_ptr, m->d_col, m->d_val, (int32_t)m->nnz, X,
                                 ldx, m->n_cols, Y, ldy, alpha, beta, algo != SM_ALGO_VECTOR, s);
    else if (algo >= SM_ALGO_AUTO && algo <= SM_ALGO_VECTOR)
        e = launch_spmm_generic(n, n_rhs, m->d_row_ptr, m->d_col, m->d_val, X, ldx, 1, Y, ldy, 1,
                                alpha, beta, true, s);
    else
        return fail(SM_ERR_INVALID_ARG, "unknown algo %d", (int)algo);
    e = after_launch(e, s, "sm_spmm");
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_spmm launch");
}

sm_status sm_sddmm(const sm_matrix *m, int32_t n_rhs, float alpha, const float *G, int64_t ldg,
                   const float *X, int64_t ldx, float beta, float *out, sm_algo algo, sm_stream stream) {
    if (n_rhs < 1) return fail(SM_ERR_INVALID_ARG, "n_rhs < 1");   // before the matrix is looked at
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (ldg < n_rhs || ldx < n_rhs) return fail(SM_ERR_INVALID_ARG, "ldg/ldx < n_rhs");
    if (algo < SM_ALGO_AUTO || algo > SM_ALGO_MERGE) return fail(SM_ERR_INVALID_ARG, "unknown algo %d", (int)algo);
    if (m->nnz == 0) return SM_OK;
    if (!out || (alpha != 0.0f && (!G || !X))) return fail(SM_ERR_INVALID_ARG, "null G/X/out");
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    const int32_t nnz = (int32_t)m->nnz;
    hipError_t e;
    if (alpha == 0.0f) {
        e = beta != 1.0f ? launch_beta(out, 1, nnz, nnz, beta, s) : hipSuccess;
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_sddmm beta");
    }
    // Every algo but PARITY is AUTO (the SpMV layouts do not matter here).  n_rhs <= 3 runs the
    // one-lane-per-term kernel: nothing to share between lanes, and n_rhs = 1 stays bit-identical.
    if (algo != SM_ALGO_PARITY && sddmm_panel_ok(m->n_rows, m->n_cols, n_rhs, G, ldg, X, ldx))
        e = launch_sddmm_panel((int32_t)m->n_rows, (int32_t)m->n_cols, nnz, n_rhs, m->d_row_ptr, m->d_col, G, ldg,
                               X, ldx, out, alpha, beta, s);
    else
        e = launch_sddmm_term((int32_t)m->n_rows, nnz, n_rhs, m->d_row_ptr, m->d_col, G, ldg, X, ldx, out, alpha,
                              beta, s);
    e = after_launch(e, s, "sm_sddmm");
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_sddmm launch");
}

// The CSR step, then one refresh per layout that holds its own copy of the values
// (kernels_values.hip): launches only, so the call can be captured.
static sm_status update_values(sm_matrix *m, bool axpy, float a, const float *d_in, sm_values_order order,
                               sm_stream stream, const char *what) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (order != SM_VALUES_OWN && order != SM_VALUES_SOURCE) return fail(SM_ERR_INVALID_ARG, "bad sm_values_order");
    if (!m->opts.updatable)
        return fail(SM_ERR_NOT_SUPPORTED, "%s: the matrix was not built with sm_build_opts.updatable", what);
    if (order == SM_VALUES_SOURCE && !m->has_src_term)
        return fail(SM_ERR_NOT_SUPPORTED,
                    "%s: SM_VALUES_SOURCE needs a matrix made by sm_create_transpose, sm_create_masked or sm_create_pruned",
                    what);
    if (m->nnz == 0 || (axpy && a == 0.0f)) return SM_OK;
    if (!d_in) return fail(SM_ERR_INVALID_ARG, "%s: null array", what);
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    const Plan &p = m->plan;
    hipError_t e = launch_values_csr(m->nnz, axpy, a, d_in, order == SM_VALUES_SOURCE ? m->d_src_term : nullptr,
                                     m->d_val, s);
    if (e == hipSuccess && p.xb.d_term) e = launch_refresh_plain(p.xb.n_term, p.xb.d_term, m->d_val, p.xb.d_val, s);
    if (e == hipSuccess && p.b2.d_term) e = launch_refresh_entry(p.b2.n_term, p.b2.d_term, m->d_val, p.b2.d_ent, s);
    if (e == hipSuccess && p.gcb.d_term) e = launch_refresh_entry(p.gcb.n_term, p.gcb.d_term, m->d_val, p.gcb.d_ent, s);
    for (const SellDev *d : {&p.sell, &p.xsell})
        if (e == hipSuccess && d->d_term) e = launch_refresh_plain(d->n_term, d->d_term, m->d_val, d->d_val, s);
    if (e == hipSuccess && p.cc.d_term) e = launch_refresh_plain(p.cc.n_term, p.cc.d_term, m->d_val, p.cc.d_val, s);
    e = after_launch(e, s, what);
    if (e != hipSuccess) return hip_fail(e, what);
    return SM_OK;
}

sm_status sm_set_values(sm_matrix *m, const float *d_v, sm_values_order order, sm_stream stream) {
    return update_values(m, false, 0.0f, d_v, order, stream, "sm_set_values");
}

sm_status sm_axpy_values(sm_matrix *m, float a, const float *d_delta, sm_values_order order, sm_stream stream) {
    return update_values(m, true, a, d_delta, order, stream, "sm_axpy_values");
}

sm_status sm_copy_table_device(const sm_matrix *m, float *d_table, sm_stream stream) {
    if (const sm_status st = need_table(m, "sm_copy_table_device")) return st;
    if (m->tab_size == 0) return SM_OK;
    if (!d_table) return fail(SM_ERR_INVALID_ARG, "sm_copy_table_device: null array");
    DeviceGuard g(m->device);
    SM_TRY_HIP(hipMemcpyAsync(d_table, m->d_tab, (size_t)m->tab_size * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SM_OK;
}

sm_status sm_copy_term_ids_device(const sm_matrix *m, uint8_t *d_ids, sm_stream stream) {
    if (const sm_status st = need_table(m, "sm_copy_term_ids_device")) return st;
    if (m->nnz == 0) return SM_OK;
    if (!d_ids) return fail(SM_ERR_INVALID_ARG, "sm_copy_term_ids_device: null array");
    DeviceGuard g(m->device);
    SM_TRY_HIP(hipMemcpyAsync(d_ids, m->d_tab_ids, (size_t)m->nnz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SM_OK;
}

sm_status sm_sddmm_table(const sm_matrix *m, int32_t n_rhs, float alpha, const float *G, int64_t ldg,
                         const float *X, int64_t ldx, float beta, float *d_out, sm_algo algo, sm_stream stream) {
    if (n_rhs < 1) return fail(SM_ERR_INVALID_ARG, "n_rhs < 1");   // before the matrix is looked at
    if (const sm_status st = need_table(m, "sm_sddmm_table")) return st;
    if (ldg < n_rhs || ldx < n_rhs) return fail(SM_ERR_INVALID_ARG, "ldg/ldx < n_rhs");
    if (algo < SM_ALGO_AUTO || algo > SM_ALGO_MERGE) return fail(SM_ERR_INVALID_ARG, "unknown algo %d", (int)algo);
    const int32_t T = m->tab_size;
    if (T == 0) return SM_OK;
    if (!d_out || (alpha != 0.0f && m->nnz > 0 && (!G || !X))) return fail(SM_ERR_INVALID_ARG, "null G/X/out");
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (alpha == 0.0f) {
        e = beta != 1.0f ? launch_beta(d_out, 1, T, T, beta, s) : hipSuccess;
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_sddmm_table beta");
    }
    const int32_t nnz = (int32_t)m->nnz;
    const bool panel = algo != SM_ALGO_PARITY && nnz > 0 && sddmm_panel_ok(m->n_rows, m->n_cols, n_rhs, G, ldg, X, ldx);
    // The partials belong to the matrix: calls take turns on the device.
    e = with_turn(m->table_turn, s, true, [&] {
        hipError_t el = launch_sddmm_table(panel, (int32_t)m->n_rows, (int32_t)m->n_cols, nnz, n_rhs, m->d_row_ptr,
                                           m->d_col, m->d_tab_ids, T, G, ldg, X, ldx, m->d_tab_partials, s);
        if (el == hipSuccess) el = launch_table_finish(m->tab_chunks, T, m->d_tab_partials, d_out, alpha, beta, s);
        return el;
    });
    e = after_launch(e, s, "sm_sddmm_table");
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_sddmm_table launch");
}

// The table step (the authoritative table and every layout's copy), then the CSR values
// (kernels_values.hip): launches only, so the call can be captured.
static sm_status update_table(sm_matrix *m, bool axpy, float a, const float *d_in, sm_stream stream,
                              const char *what) {
    if (const sm_status st = need_table(m, what)) return st;
    if (!m->opts.table_updatable)
        return fail(SM_ERR_NOT_SUPPORTED, "%s: the matrix was not built with sm_build_opts.table_updatable", what);
    if (m->tab_size == 0 || (axpy && a == 0.0f)) return SM_OK;
    if (!d_in) return fail(SM_ERR_INVALID_ARG, "%s: null array", what);
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    const Plan &p = m->plan;
    TableDst dst{};
    auto add = [&](float *tab, int32_t n) {
        if (!tab) return;
        dst.p[dst.count] = tab;
        dst.n[dst.count++] = n;
    };
    if (p.b2.n_blocks > 0) add(p.b2.d_table, 256);
    if (p.sell.n_slices > 0) add(p.sell.d_table, p.sell.table_size);
    if (p.xsell.n_slices > 0) add(p.xsell.d_table, p.xsell.table_size);
    if (p.cc.n_slices > 0) add(p.cc.d_table, 256);
    if (p.sw.n_blocks > 0) add(p.sw.d_table, 256);
    hipError_t e = launch_table_step(m->tab_size, axpy, a, d_in, m->d_tab, dst, s);
    if (e == hipSuccess) e = launch_values_from_table(m->nnz, m->d_tab_ids, m->d_tab, m->d_val, s);
    e = after_launch(e, s, what);
    if (e != hipSuccess) return hip_fail(e, what);
    return SM_OK;
}

sm_status sm_set_table(sm_matrix *m, const float *d_table, sm_stream stream) {
    return update_table(m, false, 0.0f, d_table, stream, "sm_set_table");
}

sm_status sm_axpy_table(sm_matrix *m, float a, const float *d_delta, sm_stream stream) {
    return update_table(m, true, a, d_delta, stream, "sm_axpy_table");
}

sm_status sm_copy_csr_device(const sm_matrix *m, int32_t *d_row_ptr, int32_t *d_col_idx, float *d_val,
                             sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    if (d_row_ptr)
        SM_TRY_HIP(hipMemcpyAsync(d_row_ptr, m->d_row_ptr, (size_t)(m->n_rows + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (d_col_idx && m->nnz)
        SM_TRY_HIP(hipMemcpyAsync(d_col_idx, m->d_col, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, s));
    if (d_val && m->nnz)
        SM_TRY_HIP(hipMemcpyAsync(d_val, m->d_val, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, s));
    return SM_OK;
}

sm_status sm_addmatmat(const sm_matrix *mat, const float *a, int32_t m, int32_t lda, float *c,
                       int32_t ldc, float alpha, float beta, sm_algo algo, sm_stream stream) {
    if (!mat) return fail(SM_ERR_INVALID_ARG, "null matrix");
    const int64_t k = mat->s_rows, n = mat->s_cols;
    if (m < 0) return fail(SM_ERR_INVALID_ARG, "m < 0");
    if (m == 0 || n == 0) return SM_OK;
    if (ldc < n || (alpha != 0.0f && lda < k)) return fail(SM_ERR_INVALID_ARG, "lda/ldc too small");
    if (!c || (alpha != 0.0f && k > 0 && !a)) return fail(SM_ERR_INVALID_ARG, "null a/c");
    if (m == 1 && algo != SM_ALGO_NATIVE) return sm_spmv(mat, alpha, a, beta, c, algo, stream);
    DeviceGuard g(mat->device);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (alpha == 0.0f) {
        e = beta != 1.0f ? launch_beta(c, m, (int32_t)n, ldc, beta, s) : hipSuccess;
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_addmatmat beta");
    }
    if (algo == SM_ALGO_NATIVE) {   // the reference stream, A and C read in place
        if (!mat->has_ref || (mat->plan.nat.n_panels == 0 && mat->nnz > 0))
            return fail(SM_ERR_NOT_SUPPORTED, "SM_ALGO_NATIVE needs a matrix built from the dense index");
        e = mat->plan.nat.n_panels == 0
                ? (beta != 1.0f ? launch_beta(c, m, (int32_t)n, ldc, beta, s) : hipSuccess)
                : with_turn(mat->scratch_turn, s, native_scratch(mat->plan.nat), [&] {
                      return launch_native_addmatmat(mat->plan.nat, m, a, lda, c, ldc, alpha, beta, s);
                  });
        e = after_launch(e, s, "sm_addmatmat native");
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_addmatmat native");
    }
    // Few right-hand sides on a matrix of few B rows: the row-panel kernel gives each B row
    // mp / 4 lanes, so at m <= 4 and n = 16384 it runs 16384 lanes, each a serial chain over
    // its whole row.  Two remedies, both keeping every output's terms in stored order:
    //  - short rows (<= 64 terms on average) and m <= 2: m SpMVs on A's and C's rows (x = A
    //    row i, y = C row i, contiguous, no transposes), each with a reference-order kernel
    //    (EXACT) so the result equals the row panel's bit for bit whatever m is;
    //  - otherwise the row panel on a workspace padded to 16 columns (4 lanes per B row; the
    //    padding columns are computed and never copied back).
    // blas_test 16384^2 at 25 % (rows of ~4096 terms), AUTO, round 4: m = 4 0.957 ms as four
    // SpMVs, m = 16 0.425 ms (profiles/r04_blas_test_16384_fewrhs.txt).
    const bool few_rows = n < ((int64_t)1 << 18) && k > 0 && algo != SM_ALGO_PARITY;
    if (few_rows && m <= 2 && mat->nnz <= 64 * n) {
        const sm_algo sa = (algo == SM_ALGO_AUTO || algo == SM_ALGO_EXACT) ? SM_ALGO_EXACT : algo;
        for (int32_t i = 0; i < m; i++) {
            const sm_status st = sm_spmv(mat, alpha, a + (int64_t)i * lda, beta, c + (int64_t)i * ldc, sa, stream);
            if (st != SM_OK) return st;
        }
        return SM_OK;
    }
    if (algo != SM_ALGO_PARITY && m > 128 && k > 0) {
        // Rows of A and C are independent products: row-panel calls of <= 128 rows each.
        for (int32_t i0 = 0; i0 < m; i0 += 128) {
            const sm_status st = sm_addmatmat(mat, a + (int64_t)i0 * lda, std::min<int32_t>(128, m - i0),
                                              lda, c + (int64_t)i0 * ldc, ldc, alpha, beta, algo, stream);
            if (st != SM_OK) return st;
        }
        return SM_OK;
    }
    if (algo != SM_ALGO_PARITY && m <= 128 && k > 0) {
        // C^T = B A^T through the row-panel SpMM (the reference transposes too,
        // kernel.cc:31-187): X = A^T (k x mp), Y = C^T (n x mp) in a stream-ordered
        // workspace, mp = m rounded up to 4 (the padding columns are never copied
        // back), then C = Y^T.  Same terms in the same order as the in-place kernel
        // below (bit-identical); the matrix is streamed once instead of m times.
        const int64_t mp = few_rows && m < 16 ? 16 : (m + 3) & ~3;
        // The matrix's workspace (sm_internal.h), where the reference allocates a temp
        // buffer per call (sparse-matrix.cc:155-161): stream-ordered behind the previous
        // call's kernels, so back-to-back calls neither block the host nor share bytes.
        const size_t ws_bytes = (size_t)(k + n) * mp * sizeof(float);
        std::lock_guard<std::mutex> lk(mat->ws_mu);
        e = hipSuccess;
        if (!mat->ws_ready) e = hipEventCreateWithFlags(&mat->ws_ready, hipEventDisableTiming);
        else e = hipStreamWaitEvent(s, mat->ws_ready, 0);
        if (e == hipSuccess && mat->ws_bytes < ws_bytes) {
            // Grow: the old buffer is released once its last user has finished.
            e = hipEventSynchronize(mat->ws_ready);
            if (e == hipSuccess) e = hipFree(mat->d_ws);
            mat->d_ws = nullptr;
            mat->ws_bytes = 0;
            if (e == hipSuccess) e = hipMalloc((void **)&mat->d_ws, ws_bytes);
            if (e == hipSuccess) mat->ws_bytes = ws_bytes;
            else mat->d_ws = nullptr;
        }
        float *X = mat->d_ws, *Y = mat->d_ws + k * mp;
        bool queued = false;   // any kernel on the workspace: the next user must wait for it
        if (e == hipSuccess) e = launch_transpose(a, m, (int32_t)k, lda, X, mp, s);
        queued = queued || e == hipSuccess;
        if (e == hipSuccess) e = launch_transpose(c, m, (int32_t)n, ldc, Y, mp, s);
        if (e == hipSuccess)
            e = launch_spmm_rowpanel((int32_t)n, mp == 16 && m < 16 ? 16 : m, mat->d_row_ptr, mat->d_col,
                                     mat->d_val, (int32_t)mat->nnz, X, mp, k, Y, mp, alpha, beta, true, s);
        if (e == hipSuccess) e = launch_transpose(Y, (int32_t)n, m, mp, c, ldc, s);
        if (queued) {   // recorded on the error path too: kernels may be queued
            const hipError_t er = hipEventRecord(mat->ws_ready, s);
            if (e == hipSuccess) e = er;
        }
        e = after_launch(e, s, "sm_addmatmat");
        return e == hipSuccess ? SM_OK : hip_fail(e, "sm_addmatmat (row panels)");
    }
    // Parity (or m > 128): C^T = B A^T read in place, one thread per output:
    // X(kk, i) = a[i*lda + kk], Y(j, i) = c[i*ldc + j].
    e = launch_spmm_generic((int32_t)n, m, mat->d_row_ptr, mat->d_col, mat->d_val, a, 1, lda, c,
                            1, ldc, alpha, beta, false, s);
    e = after_launch(e, s, "sm_addmatmat");
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_addmatmat launch");
}

sm_status sm_addmatmat_host(const sm_matrix *mat, const float *a, int32_t m, int32_t lda, float *c,
                            int32_t ldc, float alpha, float beta) {
    if (!mat) return fail(SM_ERR_INVALID_ARG, "null matrix");
    const int64_t k = mat->s_rows, n = mat->s_cols;
    if (m < 0) return fail(SM_ERR_INVALID_ARG, "m < 0");
    if (m == 0 || n == 0) return SM_OK;
    if (ldc < n || (alpha != 0.0f && lda < k)) return fail(SM_ERR_INVALID_ARG, "lda/ldc too small");
    if (!c || (alpha != 0.0f && k > 0 && !a)) return fail(SM_ERR_INVALID_ARG, "null a/c");
    DeviceGuard g(mat->device);
    const int64_t a_elems = (alpha != 0.0f && k > 0) ? (int64_t)(m - 1) * lda + k : 0;
    const int64_t c_elems = (int64_t)(m - 1) * ldc + n;
    DevScratch tmp;
    float *da = nullptr, *dc = nullptr;
    hipError_t e = hipSuccess;
    if (a_elems) e = tmp.alloc(&da, a_elems);
    if (e == hipSuccess) e = tmp.alloc(&dc, c_elems);
    if (e == hipSuccess && a_elems) e = hipMemcpy(da, a, (size_t)a_elems * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dc, c, (size_t)c_elems * 4, hipMemcpyHostToDevice);
    sm_status st = SM_OK;
    if (e == hipSuccess) {
        // Bit-exact: the fastest reference-order kernels (SM_ALGO_EXACT: m = 1 a
        // reference-order SpMV layout, else parity; m > 1 the row-panel path).
        st = sm_addmatmat(mat, da, m, lda, dc, ldc, alpha, beta, SM_ALGO_EXACT, nullptr);
        if (st == SM_OK) e = hipMemcpy(c, dc, (size_t)c_elems * 4, hipMemcpyDeviceToHost);
    }
    if (st != SM_OK) return st;
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_addmatmat_host");
}

sm_status sm_beta_scale(float *c, int32_t m, int32_t n, int32_t ldc, float beta, sm_stream stream) {
    if (m < 0 || n < 0 || (m > 0 && ldc < n)) return fail(SM_ERR_INVALID_ARG, "bad shape");
    if ((int64_t)m * n == 0) return SM_OK;
    if (!c) return fail(SM_ERR_INVALID_ARG, "null c");
    hipError_t e = launch_beta(c, m, n, ldc, beta, (hipStream_t)stream);
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_beta_scale");
}

sm_status sm_transpose(const float *a, int32_t m, int32_t n, int32_t lda, float *sa, int32_t ldsa,
                       sm_stream stream) {
    if (m < 0 || n < 0 || (m > 0 && lda < n) || (n > 0 && ldsa < m))
        return fail(SM_ERR_INVALID_ARG, "bad shape");   // kernel.cc:33 asserts ldsa >= m
    if ((int64_t)m * n == 0) return SM_OK;
    if (!a || !sa) return fail(SM_ERR_INVALID_ARG, "null pointer");
    hipError_t e = launch_transpose(a, m, n, lda, sa, ldsa, (hipStream_t)stream);
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_transpose");
}

sm_status sm_panel_kernel(int32_t variant, int32_t m, int32_t n, int32_t k, const float *a,
                          int32_t lda, float *c, int32_t ldc, float alpha, const uint8_t *ppos,
                          const uint8_t *pval, int32_t pos_len, const float *table,
                          int32_t valid_table_size, sm_stream stream) {
    if (variant < 0 || variant > 3) return fail(SM_ERR_INVALID_ARG, "variant must be 0..3");
    if (m < 0 || n < 0 || k < 0 || n > 256 || pos_len < 0)
        return fail(SM_ERR_INVALID_ARG, "bad panel shape m=%d n=%d k=%d pos_len=%d", m, n, k, pos_len);
    if (valid_table_size < 0 || valid_table_size > 255)
        return fail(SM_ERR_INVALID_ARG, "valid_table_size not in [0, 255]");
    const bool tr = variant >= 2;
    if (m > 0 && ((!tr && (lda < k || ldc < n)) || (tr && (lda < m || ldc < m))))
        return fail(SM_ERR_INVALID_ARG, "lda/ldc too small for variant %d", variant);
    if ((int64_t)m * n == 0 || pos_len == 0) return SM_OK;
    if (!a || !c || !ppos || !pval || !table) return fail(SM_ERR_INVALID_ARG, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    DevScratch tmp;
    uint8_t *ws = nullptr;
    // Not a hot path: a plain allocation, synchronised before it is released.
    hipError_t e = tmp.alloc(&ws, (int64_t)panel_kernel_workspace_bytes(pos_len, n));
    if (e != hipSuccess) return hip_fail(e, "sm_panel_kernel workspace");
    e = launch_panel_kernel(variant, m, n, k, a, lda, c, ldc, alpha, ppos, pval, pos_len, table,
                            valid_table_size, ws, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_panel_kernel");
}

sm_status sm_stream_sync(sm_stream stream) {
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_stream_sync");
}

}  // extern "C"
