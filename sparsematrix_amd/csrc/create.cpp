// create.cpp -- the constructors of the C ABI (include/sparsematrix.h): every sm_create_*, the
// pieces the derived ones are made of (sm_quantize_*, sm_prune_mask), sm_build_ref_stream and the
// source-map copies.  Host-side C++: argument checks, then device work that fills a new matrix's
// CSR arrays, then one of the two tails of layouts.cpp.  Every constructor begins with the same
// entry lines (clear_out, enter_device, check_table_size) and every device-side one ends in
// finish_created, so a failed constructor leaves the same state whichever it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "capi_util.h"
#include "encode.h"
#include "sm_internal.h"

using namespace smamd;

namespace {

constexpr int64_t kI32Max = std::numeric_limits<int32_t>::max();

// The first lines of every constructor: `out` is there and holds no handle until the end.
sm_status clear_out(sm_matrix **out) {
    if (!out) return fail(SM_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    return SM_OK;
}

// `T` in [lo, 255], lo 0 or 1; `empty_ok`: a matrix without terms may also have no table.
sm_status check_table_size(int32_t T, int32_t lo, bool empty_ok = false) {
    if (T > 255 || T < (empty_ok ? 0 : lo)) return fail(SM_ERR_INVALID_ARG, "table_size %d not in [%d, 255]", T, lo);
    return SM_OK;
}

sm_status check_sizes(int64_t n_rows, int64_t n_cols, int64_t nnz) {
    if (n_rows < 0 || n_cols < 0 || nnz < 0) return fail(SM_ERR_INVALID_ARG, "negative size");
    if (n_rows >= kI32Max || n_cols >= kI32Max || nnz >= kI32Max - kPadElems)
        return fail(SM_ERR_TOO_LARGE, "rows/cols/nnz must be < 2^31 (int32 indexing)");
    return SM_OK;
}

// `device` exists and is current for the scope of the caller's guard.
sm_status enter_device(DeviceGuard &g, int32_t device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(SM_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SM_ERR_INVALID_ARG, "device %d out of range", device);
    g.enter(device);
    return g.err == hipSuccess ? SM_OK : hip_fail(g.err, "hipSetDevice");
}

// The device side of a table matrix (sm_internal.h): the ids (filled by the caller), the
// authoritative table of 256 floats (zero past T; `table` a host pointer, or null when the caller
// copies it on the device) and sm_sddmm_table's partials, all counted in sm_info.device_bytes.
sm_status alloc_table(sm_matrix *m, const float *table, int32_t table_size) {
    m->is_table = true;
    m->tab_size = table_size;
    m->tab_chunks = (m->nnz + kSddmmChunk - 1) / kSddmmChunk;
    SM_TRY_HIP(m->mem.alloc(&m->d_tab_ids, m->nnz));
    SM_TRY_HIP(dev_upload_table(m->mem, &m->d_tab, table, table_size));
    SM_TRY_HIP(m->mem.alloc(&m->d_tab_partials, m->tab_chunks * kTablePartialStride));
    return SM_OK;
}

// A table handed on to a matrix made on the device: alloc_table, then `n_floats` of `d_table` (on
// the matrix's device) copied on `s`.  alloc_table zeroes the table on the default stream, which
// a non-blocking `s` does not wait for, so the zeroing is waited for here.
sm_status hand_on_table(sm_matrix *m, int32_t table_size, const float *d_table, int32_t n_floats, hipStream_t s,
                        const char *what) {
    if (const sm_status st = alloc_table(m, nullptr, table_size)) return st;
    hipError_t e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess && n_floats > 0)
        e = hipMemcpyAsync(m->d_tab, d_table, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? SM_OK : hip_fail(e, what);
}

std::unique_ptr<sm_matrix> new_matrix(int32_t device, const sm_build_opts *opts = nullptr) {
    std::unique_ptr<sm_matrix> m(new sm_matrix());
    m->device = device;
    m->opts = resolve_opts(opts);
    return m;
}

// The last lines of every constructor that works on the device: the caller gets the matrix, or,
// after a failure, nothing -- the work enqueued on `s` has drained before the matrix's arrays
// are freed, and a failed allocation leaves no sticky HIP error behind.
sm_status give_or_drop(std::unique_ptr<sm_matrix> m, sm_status st, hipStream_t s, sm_matrix **out) {
    if (st != SM_OK) {
        (void)hipStreamSynchronize(s);
        m.reset();
        (void)hipGetLastError();
        return st;
    }
    *out = m.release();
    return SM_OK;
}

// The tail of the device-side constructors: `m` holds its CSR arrays, filled on `s`, unless `st`
// says that something failed on the way; then the device-CSR tail of layouts.cpp.
sm_status finish_created(std::unique_ptr<sm_matrix> m, sm_status st, hipStream_t s, bool exact_sell, sm_matrix **out) {
    if (st == SM_OK) st = finish_from_device_csr(m.get(), s, exact_sell);
    return give_or_drop(std::move(m), st, s, out);
}

// B is n_rows x n_cols; the reference's S = B^T.
void set_shape(sm_matrix *m, int64_t n_rows, int64_t n_cols, int64_t nnz) {
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->nnz = nnz;
    m->s_rows = n_cols;
    m->s_cols = n_rows;
}

// The matrix takes the reference stream of an encoding (its codebook is the caller's business).
void adopt_ref_stream(sm_matrix *m, EncodeResult &&er) {
    m->has_ref = true;
    m->pos = std::move(er.pos);
    m->val = std::move(er.val_id);
    m->panel_row_off = std::move(er.panel_row_off);
    m->panel_col_off = std::move(er.panel_col_off);
    m->panel_begin = std::move(er.panel_begin);
    m->panel_end = std::move(er.panel_end);
}

// Host validation of a CSR: monotone row_ptr, columns in range and, with `ids` (a table
// matrix's terms), ids inside the table.
sm_status check_host_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const uint8_t *ids, int32_t table_size) {
    if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz)
        return fail(SM_ERR_INVALID_MATRIX, "row_ptr[0] must be 0 and row_ptr[n] == nnz");
    for (int64_t r = 0; r < n_rows; r++)
        if (row_ptr[r + 1] < row_ptr[r])
            return fail(SM_ERR_INVALID_MATRIX, "row_ptr decreases at row %lld", (long long)r);
    for (int64_t e = 0; e < nnz; e++) {
        if (col_idx[e] < 0 || col_idx[e] >= n_cols)
            return fail(SM_ERR_INVALID_MATRIX, "col_idx[%lld] = %d out of range", (long long)e, col_idx[e]);
        if (ids && ids[e] >= table_size)
            return fail(SM_ERR_INVALID_MATRIX, "ids[%lld] = %d >= table_size %d", (long long)e, (int)ids[e], table_size);
    }
    return SM_OK;
}
}  // namespace

extern "C" {

sm_status sm_create_from_dense_index(const uint8_t *index, int32_t rows, int32_t cols,
                                     int32_t stride, const float *table, int32_t table_size,
                                     sm_trans trans, int32_t device, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (const sm_status st = check_table_size(table_size, 0)) return st;
    if (rows < 0 || cols < 0 || stride < cols)
        return fail(SM_ERR_INVALID_ARG, "bad shape rows=%d cols=%d stride=%d", rows, cols, stride);
    if (trans != SM_NO_TRANS && trans != SM_TRANS) return fail(SM_ERR_INVALID_ARG, "bad trans");
    if (table_size > 0 && rows > 0 && cols > 0 && (!index || !table))
        return fail(SM_ERR_INVALID_ARG, "null index/table");
    DeviceGuard g;
    sm_status st = enter_device(g, device);
    if (st != SM_OK) return st;

    EncodeResult er;
    if (table_size > 0 && rows > 0 && cols > 0) {
        if (encode_dense_index(index, rows, cols, stride, table, table_size, trans == SM_TRANS, er))
            return fail(SM_ERR_INVALID_ARG, "encode failed");
    } else if (table_size > 0) {
        // degenerate shape: the reference still records rows_/cols_ (:63-64, :96-97)
        er.s_rows = trans == SM_TRANS ? cols : rows;
        er.s_cols = trans == SM_TRANS ? rows : cols;
        er.table.assign(table, table + table_size);
        er.table.push_back(0.0f);
        er.table_size = table_size;
        er.row_ptr.assign((size_t)er.s_cols + 1, 0);
    } else {
        er.row_ptr.assign(1, 0);   // val_table_size == 0: empty 0 x 0 (:26)
    }
    const int64_t nnz = er.row_ptr.back();
    st = check_sizes(er.s_cols, er.s_rows, nnz);
    if (st != SM_OK) return st;

    auto m = new_matrix(device);
    set_shape(m.get(), er.s_cols, er.s_rows, nnz);
    m->from_index = true;
    m->table_size = er.table_size;
    m->table = std::move(er.table);
    std::vector<int32_t> rp32(er.row_ptr.size());
    for (size_t i = 0; i < rp32.size(); i++) rp32[i] = (int32_t)er.row_ptr[i];
    const std::vector<int32_t> col = std::move(er.col);
    const std::vector<float> val = std::move(er.val);
    adopt_ref_stream(m.get(), std::move(er));   // the reference encoding exists (possibly empty)
    st = finish_from_host_csr(m.get(), rp32.data(), col.data(), val.data());
    if (st == SM_OK) st = upload_native(m.get());
    if (st != SM_OK) return st;
    *out = m.release();
    return SM_OK;
}

// CopyForm's scan on the device (encode_dev.hip): count, host prefix sum, fill, then the
// device-CSR constructor (validation, plans, band layout).  Same CSR as the host
// encoder, bit for bit, and the same reference stream (refenc_dev.hip, from the ids).
sm_status sm_create_from_dense_index_device(const uint8_t *d_index, int32_t rows, int32_t cols,
                                            int32_t stride, const float *table,
                                            int32_t table_size, sm_trans trans, int32_t device,
                                            sm_stream stream, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (const sm_status st = check_table_size(table_size, 0)) return st;
    if (rows < 0 || cols < 0 || stride < cols)
        return fail(SM_ERR_INVALID_ARG, "bad shape rows=%d cols=%d stride=%d", rows, cols, stride);
    if (trans != SM_NO_TRANS && trans != SM_TRANS) return fail(SM_ERR_INVALID_ARG, "bad trans");
    if (table_size == 0 || rows == 0 || cols == 0)   // nothing to scan: the host rules apply
        return sm_create_from_dense_index(nullptr, rows, cols, stride, table, table_size, trans,
                                          device, out);
    if (!d_index || !table) return fail(SM_ERR_INVALID_ARG, "null index/table");
    DeviceGuard g;
    sm_status st = enter_device(g, device);
    if (st != SM_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const bool tr = trans == SM_TRANS;
    const uint8_t T = (uint8_t)table_size;
    const int64_t nb = tr ? rows : cols;    // rows of B = columns of S
    const int64_t kb = tr ? cols : rows;    // columns of B = rows of S
    // NoTrans: index rows split in chunks so the count/fill grids fill the chip.
    const int32_t chunk_rows = tr ? rows : std::max<int32_t>(256, (rows + 63) / 64);
    const int32_t n_chunks = tr ? 1 : (rows + chunk_rows - 1) / chunk_rows;
    const int64_t n_cnt = tr ? nb : (int64_t)n_chunks * nb;
    std::vector<int32_t> cnt((size_t)n_cnt);
    int32_t *d_cnt = nullptr, *d_offs = nullptr, *d_rp = nullptr, *d_col = nullptr;
    float *d_table = nullptr, *d_val = nullptr;
    uint8_t *d_ids = nullptr;
    DevScratch tmp;
    hipError_t e = tmp.alloc(&d_cnt, n_cnt);
    if (e == hipSuccess)
        e = launch_encode_count(d_index, rows, cols, stride, tr, chunk_rows, n_chunks, T, d_cnt, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n_cnt * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "dense index count");
    // Prefix sums: row_ptr over B rows; per (chunk, row) start offsets.
    std::vector<int64_t> rp64((size_t)nb + 1, 0);
    std::vector<int32_t> offs((size_t)n_cnt);
    for (int64_t j = 0; j < nb; j++) {
        int64_t t = 0;
        for (int32_t ch = 0; ch < n_chunks; ch++) t += cnt[(size_t)(ch * nb + j)];
        rp64[(size_t)j + 1] = rp64[(size_t)j] + t;
    }
    const int64_t nnz = rp64[(size_t)nb];
    st = check_sizes(nb, kb, nnz);
    if (st != SM_OK) return st;
    for (int64_t j = 0; j < nb; j++) {
        int64_t o = rp64[(size_t)j];
        for (int32_t ch = 0; ch < n_chunks; ch++) {
            offs[(size_t)(ch * nb + j)] = (int32_t)o;
            o += cnt[(size_t)(ch * nb + j)];
        }
    }
    std::vector<int32_t> rp32(rp64.begin(), rp64.end());
    std::vector<float> tb(table, table + table_size);
    tb.push_back(0.0f);
    e = tmp.alloc(&d_offs, n_cnt);
    if (e == hipSuccess) e = tmp.alloc(&d_rp, nb + 1);
    if (e == hipSuccess) e = tmp.alloc(&d_table, (int64_t)tb.size());
    if (e == hipSuccess) e = tmp.alloc(&d_col, nnz);
    if (e == hipSuccess) e = tmp.alloc(&d_val, nnz);
    if (e == hipSuccess) e = tmp.alloc(&d_ids, nnz);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_offs, offs.data(), (size_t)n_cnt * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_rp, rp32.data(), rp32.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_table, tb.data(), tb.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch_encode_fill(d_index, rows, cols, stride, tr, chunk_rows, n_chunks, T,
                               tr ? d_rp : d_offs, d_table, d_col, d_val, d_ids, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // host vectors above go out of scope
    if (e != hipSuccess) return hip_fail(e, "dense index fill");
    sm_build_opts o;   // the CopyForm path: SM_ALGO_EXACT keeps a reference-order kernel
    sm_build_opts_init(&o);
    o.exact_sell = 1;
    st = sm_create_from_csr_device_ex(nb, kb, nnz, d_rp, d_col, d_val, device, stream, &o, out);
    if (st != SM_OK) return st;
    std::unique_ptr<sm_matrix> m(*out);   // back in hand until the stream below is in place too
    *out = nullptr;
    m->from_index = true;
    m->table_size = table_size;
    m->table = std::move(tb);
    // The reference stream from the index's own ids (refenc_dev.hip), as the host
    // constructor keeps it; S rows >= 2^23 (the reference's int32 offsets) keep none.
    EncodeResult er;
    hipError_t he = hipSuccess;
    const int rc = encode_csr_ref_device(d_rp, d_col, d_val, d_ids, nb, kb, nnz, table, table_size, er, s, he);
    if (rc == 0) {
        adopt_ref_stream(m.get(), std::move(er));
        st = upload_native(m.get());
    } else if (rc != -4) {
        st = rc == -5 ? hip_fail(he, "dense index reference stream")
                      : fail(SM_ERR_INVALID_ARG, "dense index reference stream (%d)", rc);
    }
    return give_or_drop(std::move(m), st, s, out);
}

void sm_build_opts_init(sm_build_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->layout = SM_LAYOUT_AUTO;
    o->sell = -1;
    o->sell_codebook = -1;
    o->relabel = -1;
    o->ccsell = -1;
}

sm_status sm_create_from_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row_ptr,
                             const int32_t *col_idx, const float *val, int32_t device,
                             sm_matrix **out) {
    return sm_create_from_csr_ex(n_rows, n_cols, nnz, row_ptr, col_idx, val, device, nullptr, out);
}

sm_status sm_create_from_csr_ex(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                const int32_t *row_ptr, const int32_t *col_idx, const float *val,
                                int32_t device, const sm_build_opts *opts, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    sm_status st = check_opts(opts);
    if (st != SM_OK) return st;
    st = check_sizes(n_rows, n_cols, nnz);
    if (st != SM_OK) return st;
    if (!row_ptr || (nnz > 0 && (!col_idx || !val)))
        return fail(SM_ERR_INVALID_ARG, "null CSR array");
    st = check_host_csr(n_rows, n_cols, nnz, row_ptr, col_idx, nullptr, 0);
    if (st != SM_OK) return st;
    DeviceGuard g;
    st = enter_device(g, device);
    if (st != SM_OK) return st;
    auto m = new_matrix(device, opts);
    set_shape(m.get(), n_rows, n_cols, nnz);
    st = finish_from_host_csr(m.get(), row_ptr, col_idx, val);
    if (st != SM_OK) return st;
    *out = m.release();
    return SM_OK;
}

sm_status sm_create_from_csr_ids(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row_ptr,
                                 const int32_t *col_idx, const uint8_t *ids, const float *table,
                                 int32_t table_size, int32_t device, const sm_build_opts *opts, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    sm_status st = check_opts(opts, true);
    if (st != SM_OK) return st;
    st = check_sizes(n_rows, n_cols, nnz);
    if (st != SM_OK) return st;
    if (!row_ptr || (nnz > 0 && (!col_idx || !ids))) return fail(SM_ERR_INVALID_ARG, "null CSR array");
    if ((st = check_table_size(table_size, 1, nnz == 0)) != SM_OK) return st;
    if (table_size > 0 && !table) return fail(SM_ERR_INVALID_ARG, "null table");
    st = check_host_csr(n_rows, n_cols, nnz, row_ptr, col_idx, ids, table_size);
    if (st != SM_OK) return st;
    DeviceGuard g;
    st = enter_device(g, device);
    if (st != SM_OK) return st;
    std::vector<float> val((size_t)nnz);   // the stored values: table[ids[e]], bit for bit
    for (int64_t e = 0; e < nnz; e++) memcpy(&val[(size_t)e], &table[ids[e]], 4);
    auto m = new_matrix(device, opts);
    set_shape(m.get(), n_rows, n_cols, nnz);
    st = alloc_table(m.get(), table, table_size);
    if (st == SM_OK && nnz) {
        const hipError_t e = hipMemcpy(m->d_tab_ids, ids, (size_t)nnz, hipMemcpyHostToDevice);
        if (e != hipSuccess) st = hip_fail(e, "upload term ids");
    }
    if (st == SM_OK) st = finish_from_host_csr(m.get(), row_ptr, col_idx, val.data(), ids, table);
    if (st != SM_OK) return st;
    *out = m.release();
    return SM_OK;
}

sm_status sm_create_from_csr_device(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                    const int32_t *d_row_ptr, const int32_t *d_col_idx,
                                    const float *d_val, int32_t device, sm_stream stream,
                                    sm_matrix **out) {
    return sm_create_from_csr_device_ex(n_rows, n_cols, nnz, d_row_ptr, d_col_idx, d_val, device,
                                        stream, nullptr, out);
}


sm_status sm_create_from_csr_device_ex(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                       const int32_t *d_row_ptr, const int32_t *d_col_idx,
                                       const float *d_val, int32_t device, sm_stream stream,
                                       const sm_build_opts *opts, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    sm_status st = check_opts(opts);
    if (st != SM_OK) return st;
    st = check_sizes(n_rows, n_cols, nnz);
    if (st != SM_OK) return st;
    if (!d_row_ptr || (nnz > 0 && (!d_col_idx || !d_val)))
        return fail(SM_ERR_INVALID_ARG, "null CSR array");
    DeviceGuard g;
    st = enter_device(g, device);
    if (st != SM_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    auto m = new_matrix(device, opts);
    set_shape(m.get(), n_rows, n_cols, nnz);
    st = alloc_csr(m.get());
    if (st == SM_OK) {
        hipError_t e = hipMemcpyAsync(m->d_row_ptr, d_row_ptr, (size_t)(n_rows + 1) * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(m->d_col, d_col_idx, (size_t)nnz * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(m->d_val, d_val, (size_t)nnz * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_from_csr_device");
    }
    return finish_created(std::move(m), st, s, false, out);
}

// The codebook ids of a CopyForm-built matrix's terms in CSR order, on the device: read back
// from the reference stream it holds (encode.cpp: per panel of 256 B rows the entries run by
// B column, then B row -- every B row's entries in its CSR order; (255, T) entries are
// fillers).  *d_ids stays null when the matrix holds no stream (nothing to hand on).
static sm_status ids_from_ref_stream(const sm_matrix *src, DevScratch &tmp, uint8_t **d_ids) {
    *d_ids = nullptr;
    if (!src->has_ref || src->nnz == 0 || src->table_size <= 0) return SM_OK;
    std::vector<int32_t> fill((size_t)src->n_rows + 1);
    SM_TRY_HIP(hipMemcpy(fill.data(), src->d_row_ptr, fill.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> ids((size_t)src->nnz);
    const uint8_t T = (uint8_t)src->table_size;
    int64_t seen = 0;
    for (size_t p = 0; p < src->panel_col_off.size(); p++) {
        const int64_t row0 = src->panel_col_off[p];
        int64_t lin = 0;
        for (int64_t i = src->panel_begin[p]; i < src->panel_end[p]; i++) {
            lin += src->pos[(size_t)i];
            const uint8_t id = src->val[(size_t)i];
            if (id >= T) continue;   // filler step
            const int64_t row = row0 + (lin & 255);
            if (row >= src->n_rows || fill[(size_t)row] >= src->nnz) return fail(SM_ERR_INVALID_MATRIX, "reference stream and CSR disagree");
            ids[(size_t)fill[(size_t)row]++] = id;
            seen++;
        }
    }
    if (seen != src->nnz) return fail(SM_ERR_INVALID_MATRIX, "reference stream and CSR disagree");
    SM_TRY_HIP(tmp.alloc(d_ids, src->nnz));
    const hipError_t e = hipMemcpy(*d_ids, ids.data(), ids.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        *d_ids = nullptr;
        return hip_fail(e, "upload term ids");
    }
    return SM_OK;
}

// B^T of a held matrix: its device CSR transposed on the device (transpose_dev.hip) straight
// into the new matrix's arrays, then the device-CSR constructors' tail.  A CopyForm-built source
// hands on its codebook and its default options, so the result is the twin CopyForm would build
// from the same index with the other `trans` (but for the reference stream, which
// sm_build_ref_stream adds).
sm_status sm_create_transpose(const sm_matrix *src, const sm_build_opts *opts, sm_stream stream,
                              sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (!src) return fail(SM_ERR_INVALID_ARG, "null matrix");
    sm_status st = check_opts(opts, src->is_table);
    if (st != SM_OK) return st;
    st = check_sizes(src->n_cols, src->n_rows, src->nnz);
    if (st != SM_OK) return st;
    DeviceGuard g(src->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    if (src->from_index && resolve_opts(opts).updatable)
        return fail(SM_ERR_NOT_SUPPORTED, "updatable transpose of a dense-index matrix: its values are its codebook");
    auto m = new_matrix(src->device, opts);
    set_shape(m.get(), src->n_cols, src->n_rows, src->nnz);
    if (src->from_index) {   // the CopyForm path: SM_ALGO_EXACT keeps a reference-order kernel
        m->from_index = true;
        m->table_size = src->table_size;
        m->table = src->table;
        if (m->opts.exact_sell == 0) m->opts.exact_sell = 1;
    }
    st = alloc_csr(m.get());
    if (st == SM_OK) {
        const hipError_t e = transpose_csr_device(src->d_row_ptr, src->d_col, src->d_val, src->n_rows, src->n_cols,
                                                  src->nnz, m->d_row_ptr, m->d_col, m->d_val, s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_transpose");
    }
    if (st == SM_OK && src->from_index && src->nnz > 0) {
        // The ids travel too (1 byte per term): the codebook alone cannot tell equal entries apart.
        DevScratch tmp;
        uint8_t *own = nullptr;
        if (!src->d_term_ids) st = ids_from_ref_stream(src, tmp, &own);
        const uint8_t *ids = src->d_term_ids ? src->d_term_ids : own;
        if (st == SM_OK && ids) {
            hipError_t e = m->mem.alloc(&m->d_term_ids, m->nnz);
            if (e == hipSuccess)
                e = transpose_ids_device(src->d_row_ptr, src->d_col, ids, src->n_rows, src->n_cols, src->nnz,
                                         m->d_term_ids, s);
            if (e != hipSuccess) st = hip_fail(e, "sm_create_transpose (term ids)");
        }
    }
    if (st == SM_OK && m->opts.updatable) {   // values given in src's CSR order reach this matrix too
        m->has_src_term = true;
        if (m->nnz > 0) {
            hipError_t e = m->mem.alloc(&m->d_src_term, m->nnz);
            if (e == hipSuccess)
                e = transpose_terms_device(src->d_row_ptr, src->d_col, src->n_rows, src->n_cols, src->nnz,
                                           m->d_src_term, s);
            if (e != hipSuccess) st = hip_fail(e, "sm_create_transpose (source terms)");
        }
    }
    // A table matrix hands on its current table and its ids (through the same sort as the terms).
    if (st == SM_OK && src->is_table) {
        st = hand_on_table(m.get(), src->tab_size, src->d_tab, 256, s, "sm_create_transpose (table)");
        if (st == SM_OK && m->nnz > 0) {
            const hipError_t e = transpose_ids_device(src->d_row_ptr, src->d_col, src->d_tab_ids, src->n_rows, src->n_cols,
                                                      src->nnz, m->d_tab_ids, s);
            if (e != hipSuccess) st = hip_fail(e, "sm_create_transpose (table)");
        }
    }
    return finish_created(std::move(m), st, s, true, out);
}

// A table matrix from device arrays, the arguments checked and `device` current: the CSR arrays
// copied, the values expanded from (ids, table) by a kernel that also validates the ids, then
// the device-CSR constructors' tail (as sm_create_transpose hands a table matrix on).
static sm_status create_from_ids_device(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *d_rp,
                                        const int32_t *d_col, const uint8_t *d_ids, const float *d_table,
                                        int32_t table_size, int32_t device, hipStream_t s, const sm_build_opts *opts,
                                        sm_matrix **out) {
    auto m = new_matrix(device, opts);
    set_shape(m.get(), n_rows, n_cols, nnz);
    sm_status st = alloc_csr(m.get());
    if (st == SM_OK) {
        DevScratch tmp;
        int32_t *d_flag = nullptr;
        int32_t flag = 0;
        hipError_t e = tmp.alloc(&d_flag, 1);
        if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int32_t), s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(m->d_row_ptr, d_rp, (size_t)(n_rows + 1) * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && nnz) e = hipMemcpyAsync(m->d_col, d_col, (size_t)nnz * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = launch_expand_ids(nnz, d_ids, d_table, table_size, m->d_val, d_flag, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_from_csr_ids_device");
        else if (flag) st = fail(SM_ERR_INVALID_MATRIX, "an id is >= table_size %d", table_size);
    }
    if (st == SM_OK) st = hand_on_table(m.get(), table_size, d_table, table_size, s, "sm_create_from_csr_ids_device (table)");
    if (st == SM_OK && nnz) {
        const hipError_t e = hipMemcpyAsync(m->d_tab_ids, d_ids, (size_t)nnz, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_from_csr_ids_device (table)");
    }
    return finish_created(std::move(m), st, s, true, out);
}

// What the two device table constructors refuse beyond check_opts(opts, true).
static sm_status check_table_opts(const sm_build_opts *opts) {
    const sm_status st = check_opts(opts, true);
    if (st != SM_OK) return st;
    if (resolve_opts(opts).updatable)
        return fail(SM_ERR_INVALID_ARG, "updatable: a table matrix takes new values through its table (table_updatable)");
    return SM_OK;
}

sm_status sm_create_from_csr_ids_device(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *d_row_ptr,
                                        const int32_t *d_col_idx, const uint8_t *d_ids, const float *d_table,
                                        int32_t table_size, int32_t device, sm_stream stream,
                                        const sm_build_opts *opts, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    sm_status st = check_table_opts(opts);
    if (st != SM_OK) return st;
    st = check_sizes(n_rows, n_cols, nnz);
    if (st != SM_OK) return st;
    if (!d_row_ptr || (nnz > 0 && (!d_col_idx || !d_ids))) return fail(SM_ERR_INVALID_ARG, "null CSR array");
    if ((st = check_table_size(table_size, 1, nnz == 0)) != SM_OK) return st;
    if (table_size > 0 && !d_table) return fail(SM_ERR_INVALID_ARG, "null table");
    DeviceGuard g;
    st = enter_device(g, device);
    if (st != SM_OK) return st;
    return create_from_ids_device(n_rows, n_cols, nnz, d_row_ptr, d_col_idx, d_ids, d_table, table_size, device,
                                  (hipStream_t)stream, opts, out);
}

sm_status sm_quantize_assign(const sm_matrix *m, const float *d_table, int32_t table_size, uint8_t *d_ids,
                             sm_stream stream) {
    if (const sm_status st = check_table_size(table_size, 1)) return st;   // before the matrix is looked at
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (m->nnz == 0) return SM_OK;
    if (!d_table || !d_ids) return fail(SM_ERR_INVALID_ARG, "sm_quantize_assign: null array");
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_quantize_assign(m->nnz, m->d_val, d_table, table_size, d_ids, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_quantize_assign");
}

sm_status sm_quantize_update(const sm_matrix *m, const uint8_t *d_ids, int32_t table_size, float *d_table,
                             int32_t *d_counts, double *d_sse, sm_stream stream) {
    if (const sm_status st = check_table_size(table_size, 1)) return st;   // before the matrix is looked at
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (!d_table || (m->nnz > 0 && !d_ids)) return fail(SM_ERR_INVALID_ARG, "sm_quantize_update: null array");
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = (m->nnz + kSddmmChunk - 1) / kSddmmChunk;
    DevScratch tmp;
    double *d_psum = nullptr;
    int32_t *d_pcnt = nullptr, *d_flag = nullptr;
    int32_t flag = 0;
    hipError_t e = tmp.alloc(&d_psum, chunks * kTablePartialStride);
    if (e == hipSuccess) e = tmp.alloc(&d_pcnt, chunks * kTablePartialStride);
    if (e == hipSuccess) e = tmp.alloc(&d_flag, 1);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int32_t), s);
    if (e == hipSuccess)
        e = launch_quantize_chunks(m->nnz, m->d_val, d_table, table_size, d_ids, d_psum, d_pcnt, d_flag, s);
    if (e == hipSuccess) e = launch_quantize_finish(chunks, table_size, d_psum, d_pcnt, d_table, d_counts, d_sse, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "sm_quantize_update");
    }
    if (flag) return fail(SM_ERR_INVALID_MATRIX, "sm_quantize_update: an id is >= table_size %d", table_size);
    return SM_OK;
}

sm_status sm_create_quantized(const sm_matrix *src, int32_t table_size, int32_t iters, const float *d_init,
                              const sm_build_opts *opts, sm_stream stream, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (const sm_status st = check_table_size(table_size, 1)) return st;   // before the matrix is looked at
    if (iters < 0) return fail(SM_ERR_INVALID_ARG, "iters %d < 0", iters);
    sm_status st = check_table_opts(opts);
    if (st != SM_OK) return st;
    if (!src) return fail(SM_ERR_INVALID_ARG, "null matrix");
    DeviceGuard g(src->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nnz = src->nnz;
    const int32_t T = table_size;
    const int64_t chunks = (nnz + kSddmmChunk - 1) / kSddmmChunk, parts = quantize_minmax_blocks(nnz);
    DevScratch tmp;
    float *d_table = nullptr, *d_parts = nullptr;
    uint8_t *d_ids = nullptr;
    double *d_psum = nullptr;
    int32_t *d_pcnt = nullptr, *d_flag = nullptr;
    int32_t flag = 0;
    std::vector<float> h_parts((size_t)parts * 2), h_table((size_t)T);
    hipError_t e = tmp.alloc(&d_table, T);
    if (e == hipSuccess) e = tmp.alloc(&d_ids, nnz);
    if (e == hipSuccess) e = tmp.alloc(&d_parts, parts * 2);
    if (e == hipSuccess) e = tmp.alloc(&d_flag, 2);
    if (e == hipSuccess && iters > 0) e = tmp.alloc(&d_psum, chunks * kTablePartialStride);
    if (e == hipSuccess && iters > 0) e = tmp.alloc(&d_pcnt, chunks * kTablePartialStride);
    // The least and greatest value (the linear start) and the finiteness check, which runs also
    // when the start is given.
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, 2 * sizeof(int32_t), s);
    if (e == hipSuccess) e = launch_quantize_minmax(nnz, src->d_val, d_parts, d_flag, s);
    if (e == hipSuccess && parts)
        e = hipMemcpyAsync(h_parts.data(), d_parts, h_parts.size() * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "sm_create_quantized (value range)");
    }
    if (flag) return fail(SM_ERR_INVALID_MATRIX, "sm_create_quantized: a stored value is NaN or Inf");
    if (d_init) {
        e = hipMemcpyAsync(d_table, d_init, (size_t)T * sizeof(float), hipMemcpyDeviceToDevice, s);
    } else {
        float lo = 0.0f, hi = 0.0f;   // no term: all zeros
        for (int64_t b = 0; b < parts; b++) {
            lo = b ? std::min(lo, h_parts[(size_t)(2 * b)]) : h_parts[0];
            hi = b ? std::max(hi, h_parts[(size_t)(2 * b + 1)]) : h_parts[1];
        }
        const double dlo = (double)lo + 0.0, dhi = (double)hi + 0.0;   // a zero bound counts as +0.0
        for (int32_t t = 0; t < T; t++)
            h_table[(size_t)t] = T == 1 ? (float)((dlo + dhi) / 2) : (float)(dlo + (dhi - dlo) * ((double)t / (double)(T - 1)));
        e = hipMemcpyAsync(d_table, h_table.data(), (size_t)T * sizeof(float), hipMemcpyHostToDevice, s);
    }
    // Lloyd: the launches of sm_quantize_assign and sm_quantize_update, with no synchronise or
    // allocation between them; the last assignment makes the ids those of the final table.
    for (int32_t it = 0; it < iters && e == hipSuccess; it++) {
        e = launch_quantize_assign(nnz, src->d_val, d_table, T, d_ids, s);
        if (e == hipSuccess) e = launch_quantize_chunks(nnz, src->d_val, d_table, T, d_ids, d_psum, d_pcnt, d_flag + 1, s);
        if (e == hipSuccess) e = launch_quantize_finish(chunks, T, d_psum, d_pcnt, d_table, nullptr, nullptr, s);
    }
    if (e == hipSuccess) e = launch_quantize_assign(nnz, src->d_val, d_table, T, d_ids, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // h_table is read until here
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "sm_create_quantized");
    }
    return create_from_ids_device(src->n_rows, src->n_cols, nnz, src->d_row_ptr, src->d_col, d_ids, d_table, T,
                                  src->device, s, opts, out);
}

// What sm_prune_mask and sm_create_pruned check before the matrix is looked at.
static sm_status check_prune_args(sm_prune_mode mode, int64_t count, float threshold) {
    if (mode != SM_PRUNE_GLOBAL_TOPK && mode != SM_PRUNE_ROW_TOPK && mode != SM_PRUNE_THRESHOLD)
        return fail(SM_ERR_INVALID_ARG, "unknown sm_prune_mode %d", (int)mode);
    if (mode != SM_PRUNE_THRESHOLD && count < 0) return fail(SM_ERR_INVALID_ARG, "count %lld < 0", (long long)count);
    if (mode == SM_PRUNE_THRESHOLD && !(threshold >= 0.0f))   // NaN compares false; -0.0 >= 0 holds
        return fail(SM_ERR_INVALID_ARG, "threshold must be a number >= 0");
    return SM_OK;
}

sm_status sm_prune_mask(const sm_matrix *m, sm_prune_mode mode, int64_t count, float threshold, uint8_t *d_keep,
                        int64_t *kept, sm_stream stream) {
    if (const sm_status st = check_prune_args(mode, count, threshold)) return st;
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (kept) *kept = 0;
    if (m->nnz == 0) return SM_OK;
    if (!d_keep) return fail(SM_ERR_INVALID_ARG, "sm_prune_mask: null array");
    DeviceGuard g(m->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    const hipError_t e = prune_mask_device(m->d_row_ptr, m->d_val, m->n_rows, m->nnz, mode, count, threshold, d_keep,
                                           kept, (hipStream_t)stream);
    return e == hipSuccess ? SM_OK : hip_fail(e, "sm_prune_mask");
}

// The compaction of `src` by a mask on its device, the arguments checked and the device current:
// positions, the new matrix's arrays filled by one scatter, a table source's ids and table handed
// on as sm_create_transpose does, then the device-CSR constructors' tail.
static sm_status create_masked(const sm_matrix *src, const uint8_t *d_keep, const sm_build_opts *opts, hipStream_t s,
                               sm_matrix **out) {
    DevScratch tmp;
    int32_t *d_pos = nullptr;
    int64_t new_nnz = 0;
    hipError_t e = tmp.alloc(&d_pos, src->nnz + 1);
    if (e == hipSuccess) e = prune_positions_device(src->nnz, d_keep, d_pos, &new_nnz, s);
    if (e != hipSuccess) return hip_fail(e, "sm_create_masked (positions)");
    auto m = new_matrix(src->device, opts);
    set_shape(m.get(), src->n_rows, src->n_cols, new_nnz);
    sm_status st = alloc_csr(m.get());
    m->has_src_term = true;
    if (st == SM_OK && new_nnz > 0) {
        e = m->mem.alloc(&m->d_src_term, new_nnz);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_masked (source terms)");
    }
    if (st == SM_OK && src->is_table)
        st = hand_on_table(m.get(), src->tab_size, src->d_tab, 256, s, "sm_create_masked (table)");
    if (st == SM_OK) {
        e = launch_prune_compact(src->n_rows, src->nnz, d_keep, d_pos, src->d_row_ptr, src->d_col, src->d_val,
                                 src->is_table ? src->d_tab_ids : nullptr, m->d_row_ptr, m->d_col, m->d_val,
                                 m->d_src_term, m->d_tab_ids, new_nnz > 0, s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_masked (scatter)");
    }
    return finish_created(std::move(m), st, s, src->is_table, out);   // synchronises s: d_pos is free to go
}

sm_status sm_create_masked(const sm_matrix *src, const uint8_t *d_keep, const sm_build_opts *opts, sm_stream stream,
                           sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (!src) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (const sm_status st = check_opts(opts, src->is_table)) return st;
    if (src->nnz > 0 && !d_keep) return fail(SM_ERR_INVALID_ARG, "sm_create_masked: null array");
    DeviceGuard g(src->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    return create_masked(src, d_keep, opts, (hipStream_t)stream, out);
}

sm_status sm_create_pruned(const sm_matrix *src, sm_prune_mode mode, int64_t count, float threshold,
                           const sm_build_opts *opts, sm_stream stream, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (const sm_status st = check_prune_args(mode, count, threshold)) return st;
    if (!src) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (const sm_status st = check_opts(opts, src->is_table)) return st;
    DeviceGuard g(src->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    DevScratch tmp;
    uint8_t *d_keep = nullptr;
    hipError_t e = tmp.alloc(&d_keep, src->nnz);
    if (e == hipSuccess)
        e = prune_mask_device(src->d_row_ptr, src->d_val, src->n_rows, src->nnz, mode, count, threshold, d_keep, nullptr, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, "sm_create_pruned (mask)");
    }
    return create_masked(src, d_keep, opts, s, out);
}

// The entrance of the pipeline: select and compact straight from a dense device matrix
// (kernels_dense.hip), then the device-CSR constructors' tail, as create_masked ends.
sm_status sm_create_from_dense_device(const float *d_w, int64_t n_rows, int64_t n_cols, int64_t ld, sm_prune_mode mode,
                                      int64_t count, float threshold, int32_t device, sm_stream stream,
                                      const sm_build_opts *opts, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (const sm_status st = check_prune_args(mode, count, threshold)) return st;
    if (n_rows < 0 || n_cols < 0) return fail(SM_ERR_INVALID_ARG, "negative size");
    if (n_rows > 1 && ld < n_cols)
        return fail(SM_ERR_INVALID_ARG, "sm_create_from_dense_device: ld %lld < n_cols %lld", (long long)ld, (long long)n_cols);
    if (const sm_status st = check_opts(opts)) return st;   // table_updatable among them
    if (const sm_status st = check_sizes(n_rows, n_cols, 0)) return st;
    // n_rows, n_cols < 2^31: the product fits 64 bits.  The 32-bit bins of the select count E.
    const uint64_t E = (uint64_t)n_rows * (uint64_t)n_cols;
    if (E > 0xFFFFFFFFull)
        return fail(SM_ERR_TOO_LARGE, "sm_create_from_dense_device: %llu elements, at most 2^32 - 1", (unsigned long long)E);
    int64_t known = -1;   // the kept count where the arguments give it
    if (mode == SM_PRUNE_GLOBAL_TOPK) known = (int64_t)std::min<uint64_t>((uint64_t)count, E);
    if (mode == SM_PRUNE_ROW_TOPK) known = n_rows * std::min(count, n_cols);
    if (known >= 0)
        if (const sm_status st = check_sizes(n_rows, n_cols, known)) return st;
    if (E > 0 && !d_w) return fail(SM_ERR_INVALID_ARG, "sm_create_from_dense_device: null matrix pointer");
    DeviceGuard g;
    sm_status st = enter_device(g, device);
    if (st != SM_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    DevScratch tmp;
    uint8_t *d_keep = nullptr;
    uint32_t *d_base = nullptr;
    int64_t kept = 0;
    if (E > 0 && known != 0) {
        const hipError_t e = dense_mask_device(d_w, n_rows, n_cols, ld, mode, count, threshold, tmp, &d_keep, &d_base, &kept, s);
        if (e != hipSuccess) return hip_fail(e, "sm_create_from_dense_device (select)");
        if (const sm_status sz = check_sizes(n_rows, n_cols, kept)) return sz;   // SM_PRUNE_THRESHOLD: known only now
    }
    auto m = new_matrix(device, opts);
    set_shape(m.get(), n_rows, n_cols, kept);
    st = alloc_csr(m.get());
    if (st == SM_OK) {
        const hipError_t e = kept > 0 ? launch_dense_fill(d_w, n_rows, n_cols, ld, d_keep, d_base, m->d_row_ptr, m->d_col, m->d_val, s)
                                      : hipMemsetAsync(m->d_row_ptr, 0, (size_t)(n_rows + 1) * sizeof(int32_t), s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_from_dense_device (fill)");
    }
    return finish_created(std::move(m), st, s, false, out);   // synchronises s: the scratch is free to go
}

// C = alpha A + beta B on the union of the patterns (kernels_sum.hip): count, check the size, fill
// the new matrix's arrays and maps, then the device-CSR constructors' tail, as create_masked ends.
sm_status sm_create_sum(const sm_matrix *a, float alpha, const sm_matrix *b, float beta, const sm_build_opts *opts,
                        sm_stream stream, sm_matrix **out) {
    if (const sm_status st = clear_out(out)) return st;
    if (!a || !b) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (const sm_status st = check_opts(opts)) return st;   // table_updatable among them
    if (a->n_rows != b->n_rows || a->n_cols != b->n_cols)
        return fail(SM_ERR_INVALID_ARG, "sm_create_sum: a is %lld x %lld, b is %lld x %lld", (long long)a->n_rows,
                    (long long)a->n_cols, (long long)b->n_rows, (long long)b->n_cols);
    if (a->device != b->device)
        return fail(SM_ERR_INVALID_ARG, "sm_create_sum: a is on device %d, b on device %d", a->device, b->device);
    for (const sm_matrix *x : {a, b})
        if (!x->rows_ascend)
            return fail(SM_ERR_NOT_SUPPORTED, "sm_create_sum: a row of operand %s holds a descending step or a repeated "
                                              "column: no merge and no single source term", x == a ? "a" : "b");
    DeviceGuard g(a->device);
    if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    DevScratch tmp;
    int32_t *d_m = nullptr, *d_S = nullptr, *d_rpc = nullptr;
    uint64_t nnz_c = 0;
    hipError_t e = sum_count_device(a->n_rows, a->nnz, b->nnz, a->d_row_ptr, a->d_col, b->d_row_ptr, b->d_col, tmp, &d_m,
                                    &d_S, &d_rpc, &nnz_c, s);
    if (e != hipSuccess) return hip_fail(e, "sm_create_sum (count)");
    if (const sm_status st = check_sizes(a->n_rows, a->n_cols, (int64_t)nnz_c)) return st;   // nnz_c < 2^32
    const int64_t nnz = (int64_t)nnz_c;
    auto m = new_matrix(a->device, opts);
    set_shape(m.get(), a->n_rows, a->n_cols, nnz);
    sm_status st = alloc_csr(m.get());
    m->has_sum_terms = true;
    if (st == SM_OK && nnz > 0) {
        e = m->mem.alloc(&m->d_sum_terms_a, nnz);
        if (e == hipSuccess) e = m->mem.alloc(&m->d_sum_terms_b, nnz);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_sum (source maps)");
    }
    if (st == SM_OK) {
        e = hipMemcpyAsync(m->d_row_ptr, d_rpc, (size_t)(a->n_rows + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && nnz > 0)
            e = launch_sum_fill(a->n_rows, a->nnz, b->nnz, a->d_row_ptr, a->d_col, a->d_val, alpha, b->d_row_ptr, b->d_col,
                                b->d_val, beta, d_m, d_S, d_rpc, m->d_col, m->d_val, m->d_sum_terms_a, m->d_sum_terms_b, s);
        if (e != hipSuccess) st = hip_fail(e, "sm_create_sum (fill)");
    }
    return finish_created(std::move(m), st, s, false, out);   // synchronises s: the scratch is free to go
}

sm_status sm_copy_sum_terms_device(const sm_matrix *m, int32_t *d_terms_a, int32_t *d_terms_b, sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (!m->has_sum_terms)
        return fail(SM_ERR_NOT_SUPPORTED, "sm_copy_sum_terms_device: the matrix holds no sum maps (sm_create_sum)");
    if (m->nnz == 0) return SM_OK;
    DeviceGuard g(m->device);
    if (d_terms_a)
        SM_TRY_HIP(hipMemcpyAsync(d_terms_a, m->d_sum_terms_a, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_terms_b)
        SM_TRY_HIP(hipMemcpyAsync(d_terms_b, m->d_sum_terms_b, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SM_OK;
}

sm_status sm_copy_source_terms_device(const sm_matrix *m, int32_t *d_terms, sm_stream stream) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (!m->has_src_term)
        return fail(SM_ERR_NOT_SUPPORTED, "sm_copy_source_terms_device: the matrix holds no source map (sm_create_masked, "
                                          "sm_create_pruned, or sm_create_transpose with updatable)");
    if (m->nnz == 0) return SM_OK;
    if (!d_terms) return fail(SM_ERR_INVALID_ARG, "sm_copy_source_terms_device: null array");
    DeviceGuard g(m->device);
    SM_TRY_HIP(hipMemcpyAsync(d_terms, m->d_src_term, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SM_OK;
}

sm_status sm_build_ref_stream(sm_matrix *m, const float *table, int32_t table_size) {
    if (!m) return fail(SM_ERR_INVALID_ARG, "null matrix");
    if (m->opts.updatable)
        return fail(SM_ERR_NOT_SUPPORTED, "updatable matrix: the stream would go stale with the next update");
    if (m->opts.table_updatable)
        return fail(SM_ERR_NOT_SUPPORTED, "table_updatable matrix: the stream would go stale with the next update");
    if (m->has_ref) return SM_OK;
    if (table)
        if (const sm_status st = check_table_size(table_size, 0)) return st;
    DeviceGuard g(m->device);
    // On the device (refenc_dev.hip): sort, gaps, scan and emit; the host keeps the stream's
    // copy (sm_copy_ref_stream, sm_equal) and derives the native layout's batch metadata.
    EncodeResult er;
    hipError_t he = hipSuccess;
    // A transposed CopyForm matrix given its own codebook: the ids the index gave its terms.
    const uint8_t *ids = nullptr;
    if (m->d_term_ids && table && table_size > 0 && table_size == m->table_size &&
        m->table.size() >= (size_t)table_size && memcmp(table, m->table.data(), (size_t)table_size * 4) == 0)
        ids = m->d_term_ids;
    const int rc = encode_csr_ref_device(m->d_row_ptr, m->d_col, m->d_val, ids, m->n_rows, m->n_cols,
                                         m->nnz, table, table_size, er, nullptr, he);
    if (rc == -5) return hip_fail(he, "sm_build_ref_stream");
    if (rc == -2) return fail(SM_ERR_INVALID_ARG, "a value is not in the codebook");
    if (rc == -3) return fail(SM_ERR_NOT_SUPPORTED, "more than 255 distinct values: no uint8 ids");
    if (rc == -4) return fail(SM_ERR_NOT_SUPPORTED, "S rows >= 2^23: the reference's int32 offsets overflow");
    if (rc == -6)
        return fail(SM_ERR_NOT_SUPPORTED, "a (row, column) is stored more than once: the reference's "
                                          "stream comes from a dense index and cannot hold a repeat");
    if (rc != 0) return fail(SM_ERR_INVALID_ARG, "bad codebook");
    // d_term_ids indexes m->table and lives only while no stream is held: from here the stream
    // carries the ids (of whichever codebook was given), so the carried ones go.
    m->mem.release(m->d_term_ids);
    m->table_size = er.table_size;
    m->table = std::move(er.table);
    adopt_ref_stream(m, std::move(er));
    const size_t mark = m->mem.mark();
    const sm_status st = upload_native(m);
    if (st != SM_OK) {   // no half-built encoding -- a retry starts over
        m->mem.release_since(mark);
        m->plan.nat = NativeDev{};
        m->has_ref = false;
        m->table_size = 0;
        for (auto *v : {&m->pos, &m->val}) std::vector<uint8_t>().swap(*v);
        std::vector<float>().swap(m->table);
        std::vector<int32_t>().swap(m->panel_row_off);
        std::vector<int32_t>().swap(m->panel_col_off);
        std::vector<int64_t>().swap(m->panel_begin);
        std::vector<int64_t>().swap(m->panel_end);
    }
    return st;
}

}  // extern "C"
