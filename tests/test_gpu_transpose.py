"""The transposed matrix built on the device (sm_create_transpose) and the products with B^T.

Oracles: the reference's own Trans encoding of the same index (the golden fixtures and the CPU
restatement oracle.RefModel built with the other `trans`), and for CSR sources a stable
argsort by column on the CPU.  Structures are compared exactly (values by bits), parity / exact
products by bits, the fast kernels within the project's 1e-6 * sum|terms| bound.
"""
import numpy as np
import pytest

import oracle

from golden_util import bits_equal, case_names, load_case
from gpu_util import assert_terms_close, bits, skewed_csr, to_dev, to_host, torch_dev, uniform_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _build(sm, c, trans):
    return sm.SparseMatrix(c.dm, c.rows, c.cols, c.stride, c.table, c.table_size,
                           sm.SblasTrans if trans else sm.SblasNoTrans)


def _twin_model(c):
    return oracle.RefModel(c.dm, c.rows, c.cols, c.stride, c.table, c.table_size, trans=not c.trans)


def cpu_transpose(rp, ci, va, n_cols):
    """CSR of B^T: the terms stably sorted by column; their source rows become the columns."""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    t_rp = np.zeros(n_cols + 1, np.int64)
    t_rp[1:] = np.cumsum(np.bincount(ci, minlength=n_cols))
    return t_rp.astype(np.int32), rows[order].astype(np.int32), np.asarray(va, np.float32)[order]


def assert_csr_equal(got, want):
    assert np.array_equal(np.asarray(got[0], np.int64), np.asarray(want[0], np.int64)), "row_ptr"
    assert np.array_equal(np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)), "col_idx"
    assert np.array_equal(bits(got[2]), bits(want[2])), "values (bits)"


# ------------------------------------------------------- 1. the reference's Trans encoding
@pytest.mark.parametrize("name", case_names())
def test_transposed_equals_trans_built_twin(sm, name):
    c = load_case(name)
    A = _build(sm, c, c.trans)
    At = A.transposed()
    Twin = _build(sm, c, not c.trans)
    assert At == Twin
    assert_csr_equal(At.csr(), Twin.csr())
    model = _twin_model(c)
    assert_csr_equal(At.csr(), model.to_csr()[:3])
    ia, it, iw = A.info(), At.info(), Twin.info()
    assert (it["s_rows"], it["s_cols"], it["n_rows"], it["n_cols"]) == \
           (ia["s_cols"], ia["s_rows"], ia["n_cols"], ia["n_rows"])
    assert it["nnz"] == ia["nnz"]
    assert it["table_size"] == iw["table_size"] and it["exact_algo"] == iw["exact_algo"]
    assert it["has_ref_stream"] == 0
    At.build_ref_stream(c.table[: c.table_size])
    got, want = At.ref_stream(), model.stream()
    assert (got["rows"], got["cols"]) == (want.rows, want.cols)
    for k in ("pos", "val", "panel_row_off", "panel_col_off", "panel_begin", "panel_end"):
        assert np.array_equal(got[k], getattr(want, k)), k
    assert At == Twin   # now the reference's member-wise comparison


def test_equal_codebook_entries_keep_their_ids(sm):
    """zero_table_entries' codebook holds 0.0 sixteen times: the values alone cannot name the
    ids the index used, so they travel with the terms -- also through B^T^T."""
    c = load_case("zero_table_entries")
    A = _build(sm, c, c.trans)
    Att = A.transposed().transposed()
    Att.build_ref_stream(c.table[: c.table_size])
    got, want = Att.ref_stream(), A.ref_stream()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert Att == A
    # another codebook (here: derived from the values) does not use the carried ids
    B = A.transposed()
    B.build_ref_stream()
    assert B.info()["table_size"] < c.table_size


def test_ids_follow_the_codebook_in_use(sm):
    """B = A^T takes another codebook (the derived one), then C = B^T is given B's codebook: the
    ids C uses must be ids into that codebook, not the ones A's index gave.  C's stream and its
    native product against the oracle encoding of the same matrix with that codebook."""
    c = load_case("zero_table_entries")
    A = _build(sm, c, c.trans)
    B = A.transposed()
    B.build_ref_stream()   # derived: the values' distinct bit patterns in B's CSR order
    vb = bits(B.csr()[2])
    uniq, first = np.unique(vb, return_index=True)
    table2 = uniq[np.argsort(first)].view(np.float32)
    T2 = table2.size
    assert B.info()["table_size"] == T2 < c.table_size
    # the same index renamed onto table2 (ids >= table_size stay empty: 255 >= T2)
    pos_of = {int(u): i for i, u in enumerate(bits(table2))}
    remap = np.full(256, 255, np.uint8)
    for i, u in enumerate(bits(c.table[: c.table_size])):
        remap[i] = pos_of.get(int(u), 255)   # an entry no term uses stays empty
    dm2 = remap[c.dm]
    model_b = oracle.RefModel(dm2, c.rows, c.cols, c.stride, table2, T2, trans=not c.trans)
    model_c = oracle.RefModel(dm2, c.rows, c.cols, c.stride, table2, T2, trans=c.trans)
    C = B.transposed()
    assert C.info()["table_size"] == T2
    C.build_ref_stream(table2)
    for M, model in ((B, model_b), (C, model_c)):
        got, want = M.ref_stream(), model.stream()
        for k in ("pos", "val", "panel_row_off", "panel_col_off", "panel_begin", "panel_end"):
            assert np.array_equal(got[k], getattr(want, k)), k
    k, n = model_c.rows, model_c.cols
    rng = np.random.default_rng(13)
    for m in (1, 3):
        a = rng.uniform(-1, 1, m * k).astype(np.float32)
        c0 = rng.uniform(-1, 1, m * n).astype(np.float32)
        c_d = to_dev(c0)
        C.AddMatMat(to_dev(a), m, k, c_d, n, 1.3, 0.7, algo="native")
        assert bits_equal(to_host(c_d), model_c.add_mat_mat(a, m, k, c0, n, 1.3, 0.7)), m
    # and given A's codebook instead, a fresh B^T still gets the index's own ids
    C2 = A.transposed().transposed()
    C2.build_ref_stream(c.table[: c.table_size])
    assert C2 == A


# ------------------------------------------------------------------- 2. products, bit-exact
PRODUCT_CASES = ["sweep_1024x1_0.001_n_T255", "sweep_1x1024_0.001_n_T255", "sweep_257x1_0.01_t_T63",
                 "sweep_1024x257_0.01_t_T255", "sweep_257x257_0.25_n_T63", "sweep_300x257_0.001_t_T255",
                 "published_1023x2047_t", "zero_table_entries", "fillers_4000x300"]


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_transposed_addmatmat_bit_exact(sm, name):
    c = load_case(name)
    At = _build(sm, c, c.trans).transposed()
    model = _twin_model(c)
    k, n = model.rows, model.cols
    assert (At.NumRows(), At.NumCols()) == (k, n)
    rng = np.random.default_rng(11)
    for m in (1, 3):
        a = rng.uniform(-1, 1, m * k).astype(np.float32)
        c0 = rng.uniform(-1, 1, m * n).astype(np.float32)
        want = model.add_mat_mat(a, m, k, c0, n, 1.3, 0.7)
        for algo in ("exact", "parity"):
            c_d = to_dev(c0)
            At.AddMatMat(to_dev(a), m, k, c_d, n, 1.3, 0.7, algo=algo)
            assert bits_equal(to_host(c_d), want), (algo, m)


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_spmv_t_spmm_t(sm, name):
    c = load_case(name)
    A = _build(sm, c, c.trans)
    rp, ci, va = A.csr()
    n_rows, n_cols = A.n_rows, A.n_cols
    trp, tci, tva = cpu_transpose(rp, ci, va, n_cols)
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, n_rows).astype(np.float32)
    y0 = rng.uniform(-1, 1, n_cols).astype(np.float32)
    want = oracle.csr_spmv(trp, tci, tva, x, y0, 1.3, 0.7)
    _, absum = oracle.csr_spmv_f64(trp.astype(np.int64), tci, tva, x, y0, 1.3, 0.7)
    y = to_dev(y0)
    A.spmv_t(to_dev(x), y, 1.3, 0.7, algo="parity")
    assert bits_equal(to_host(y), want)
    y = to_dev(y0)
    A.spmv_t(to_dev(x), y, 1.3, 0.7, algo="auto")
    assert_terms_close(to_host(y), want, absum)
    N = 4
    X = rng.uniform(-1, 1, (n_rows, N)).astype(np.float32)
    Y0 = rng.uniform(-1, 1, (n_cols, N)).astype(np.float32)
    wantY = oracle.csr_spmm(trp.astype(np.int64), tci, tva, X, Y0, 1.3, 0.7)
    Y = to_dev(Y0)
    A.spmm_t(to_dev(X), Y, 1.3, 0.7, algo="parity")
    assert bits_equal(to_host(Y), wantY)
    Y = to_dev(Y0)
    A.spmm_t(to_dev(X), Y, 1.3, 0.7, algo="auto")
    got = to_host(Y)
    for i in range(N):
        _, ab = oracle.csr_spmv_f64(trp.astype(np.int64), tci, tva, X[:, i].copy(), Y0[:, i].copy(), 1.3, 0.7)
        assert_terms_close(got[:, i], wantY[:, i], ab)


# ------------------------------------------------------------------------- 3. CSR sources
def _skewed():
    rng = np.random.default_rng(21)
    lengths = rng.integers(0, 40, 400)
    lengths[::7] = 0
    lengths[123] = 5000   # 300 columns: every column repeats in it, hub columns of B^T
    return skewed_csr(400, 300, lengths, seed=22) + (300,)


def _edge_empty_columns():
    rp, ci, va = uniform_csr(500, 300, 4, seed=23)
    return rp, (ci + 64).astype(np.int32), va, 300 + 128   # the first and last 64 columns empty


CSR_SOURCES = {
    "uniform_1000x777": lambda: uniform_csr(1000, 777, 5, seed=1000) + (777,),
    "wide_777x4099": lambda: uniform_csr(777, 4099, 3, seed=777) + (4099,),
    "skewed_400x300": _skewed,
    "empty_edge_columns": _edge_empty_columns,
}


@pytest.mark.parametrize("ingest", ["host", "device"])
@pytest.mark.parametrize("source", list(CSR_SOURCES))
def test_csr_source(sm, source, ingest):
    rp, ci, va, n_cols = CSR_SOURCES[source]()
    n_rows = rp.size - 1
    if ingest == "device":
        M = sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), n_cols)
    else:
        M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    want = cpu_transpose(rp, ci, va, n_cols)
    t = M.transposed()
    assert (t.n_rows, t.n_cols, t.nnz) == (n_cols, n_rows, ci.size)
    assert_csr_equal(t.csr(), want)
    # every source here has ascending (non-decreasing) columns per row: B^T^T is B, term for term
    assert_csr_equal(t.transposed().csr(), (rp, ci, va))
    t2 = M.transposed()
    assert_csr_equal(t2.csr(), t.csr())
    assert t2.layout_digest() == t.layout_digest()
    assert t2.info()["device_bytes"] == t.info()["device_bytes"]
    rng = np.random.default_rng(24)
    x = rng.uniform(-1, 1, n_rows).astype(np.float32)
    y0 = rng.uniform(-1, 1, n_cols).astype(np.float32)
    y = to_dev(y0)
    t.spmv(to_dev(x), y, 1.3, 0.7, algo="parity")
    assert bits_equal(to_host(y), oracle.csr_spmv(*want, x, y0, 1.3, 0.7))


def test_values_carried_bit_for_bit(sm):
    """Explicit zeros, -0.0, infinities and NaN payloads travel unchanged."""
    rp, ci, va = uniform_csr(300, 257, 6, seed=31)
    u = va.view(np.uint32).copy()
    u[::5] = 0x00000000
    u[1::7] = 0x80000000
    u[2::11] = 0x7FC0DEAD
    u[3::13] = 0xFFC12345
    u[4::17] = 0x7F800000
    va = u.view(np.float32)
    M = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    assert_csr_equal(M.transposed().csr(), cpu_transpose(rp, ci, va, 257))


# ------------------------------------------------------------------ 4. options pass through
def test_options_pass_through(sm):
    n = 4096
    rp, ci, va = uniform_csr(n, n, 8, seed=41)   # values from a 255-entry codebook
    M = sm.SparseMatrix.from_csr(rp, ci, va, n)
    want = cpu_transpose(rp, ci, va, n)
    t = M.transposed(opts={"layout": "cband", "band_slabs": 1})
    info = t.info()
    assert info["has_xband"] == 5 and info["xband_slabs"] == 1, info
    assert_csr_equal(t.csr(), want)
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    y0 = rng.uniform(-1, 1, n).astype(np.float32)
    y = to_dev(y0)
    t.spmv(to_dev(x), y, 1.3, 0.7, algo="xband")
    assert bits_equal(to_host(y), oracle.csr_spmv(*want, x, y0, 1.3, 0.7))
    assert M.transposed(opts={"layout": "no_bands"}).info()["has_xband"] == 0
    with pytest.raises(sm.SparseMatrixError) as ei:
        M.transposed(opts={"band_tall": 3})
    assert ei.value.status == 1   # SM_ERR_INVALID_ARG


# ------------------------------------------------------------------ 5. empty and degenerate
def test_no_terms(sm):
    n_rows, n_cols = 37, 53
    M = sm.SparseMatrix.from_csr(np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32),
                                 np.zeros(0, np.float32), n_cols)
    t = M.transposed()
    info = t.info()
    assert (info["n_rows"], info["n_cols"], info["nnz"]) == (n_cols, n_rows, 0)
    assert np.array_equal(t.csr()[0], np.zeros(n_cols + 1, np.int32))
    y0 = np.random.default_rng(51).uniform(-1, 1, n_cols).astype(np.float32)
    y = to_dev(y0)
    t.spmv(to_dev(np.ones(n_rows, np.float32)), y, 1.0, 0.5)
    assert bits_equal(to_host(y), y0 * np.float32(0.5))


def test_empty_zero_by_zero(sm):
    M = sm.SparseMatrix(np.zeros(4, np.uint8), 2, 2, 2, None, 0)   # val_table_size == 0: 0 x 0
    assert (M.NumRows(), M.NumCols()) == (0, 0)
    t = M.transposed()
    info = t.info()
    assert (info["n_rows"], info["n_cols"], info["nnz"], info["s_rows"], info["s_cols"]) == (0, 0, 0, 0, 0)
    assert t == M


# ------------------------------------------------------------------------ 6. Python surface
def test_python_surface(sm):
    c = load_case("sweep_257x300_0.001_t_T255")
    m = _build(sm, c, c.trans)
    t = m.T
    assert m.T is t
    assert t is not m and t.T is not m and t.T == m   # m.T.T: a third matrix equal to m
    x_bad = to_dev(np.zeros(m.n_rows - 1, np.float32))
    with pytest.raises(ValueError):
        m.spmv_t(x_bad, to_dev(np.zeros(m.n_cols, np.float32)))
    m.CopyForm(c.dm, c.rows, c.cols, c.stride, c.table, c.table_size,
               sm.SblasNoTrans if c.trans else sm.SblasTrans)
    assert t._h is None        # the old companion went with the old matrix
    t2 = m.T
    assert t2 is not t and t2 == _build(sm, c, c.trans)
    m.Destroy()
    assert m._t is None and t2._h is None
    with pytest.raises(RuntimeError):
        m.T


# ------------------------------------------------------------------------------ 7. autograd
@pytest.fixture(scope="module")
def grad_case(sm):
    rp, ci, va = uniform_csr(300, 257, 6, seed=71)
    m = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    dense = np.zeros((300, 257), np.float64)
    rows = np.repeat(np.arange(300), np.diff(rp))
    np.add.at(dense, (rows, ci), va.astype(np.float64))
    return m, dense


@pytest.mark.parametrize("shape", ["spmm", "spmm_noncontiguous_grad", "spmv"])
def test_autograd(sm, grad_case, shape):
    torch = torch_dev()
    from sparsematrix_amd import autograd
    m, dense = grad_case
    rng = np.random.default_rng(72)
    tail = () if shape == "spmv" else (4,)
    Xh = rng.uniform(-1, 1, (257,) + tail).astype(np.float32)
    Gh = rng.uniform(-1, 1, (300,) + tail).astype(np.float32)
    X = to_dev(Xh).requires_grad_(True)
    G = to_dev(Gh)
    if shape == "spmm_noncontiguous_grad":
        G = to_dev(np.ascontiguousarray(Gh.T)).t()
        assert not G.is_contiguous()
    Y = autograd.apply(m, X, alpha=1.3)
    Y.backward(G)
    Y0 = torch.zeros_like(Y)
    Gc = G.contiguous()
    gX = torch.zeros_like(X)
    if shape == "spmv":
        m.spmv(X.detach(), Y0, 1.3, 0.0)
        m.T.spmv(Gc, gX, 1.3, 0.0)
    else:
        m.spmm(X.detach(), Y0, 1.3, 0.0)
        m.T.spmm(Gc, gX, 1.3, 0.0)
    assert bits_equal(to_host(Y), to_host(Y0))
    assert X.grad.shape == X.shape
    assert bits_equal(to_host(X.grad), to_host(gX))
    want = dense.T @ (1.3 * Gh.astype(np.float64))
    absum = np.abs(dense).T @ np.abs(1.3 * Gh.astype(np.float64))
    assert_terms_close(to_host(X.grad), want, absum)
