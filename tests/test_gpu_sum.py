"""The sum of two matrices on the GPU: sm_create_sum and sm_copy_sum_terms_device.

Every result is compared with sum_ref, the numpy restatement of the header's rule: row_ptr, col_idx
and both source maps exactly, the values bit for bit where the restatement is not a NaN and a NaN
where it is; and with SparseMatrix.from_csr of the restated arrays (on the device, same opts): ==,
digests, info, where the layouts were built, products, bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_specs
import sum_ref as sr
import table_ref
from gpu_util import bits, messy_csr, to_dev, to_host, torch_dev, uniform_csr
from test_gpu_prune import SPECIAL   # the prune tests' special values

pytestmark = pytest.mark.gpu

INVALID, NOT_SUPPORTED = 1, 4
GUARD = 64
CHUNK = 2048
COEFS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (-0.5, 3.0), (1.0, -1.0))
ALGOS = ("auto", "parity", "exact")


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def status_of(call):
    from sparsematrix_amd._lib import SparseMatrixError
    with pytest.raises(SparseMatrixError) as ei:
        call()
    return ei.value.status


# ------------------------------------------------------------------------------- inputs
def specials(nnz, seed):
    """Uniform values with the prune tests' special values at the front, at the back and across the
    2048-term chunk boundary (as many of them as fit)."""
    v = np.random.default_rng(seed).uniform(-1, 1, nnz).astype(np.float32)
    n = min(SPECIAL.size, nnz)
    v[:n] = SPECIAL[:n]
    v[nnz - n:] = SPECIAL[:n][::-1]
    if nnz > CHUNK + n:
        v[CHUNK - n // 2: CHUNK - n // 2 + n] = SPECIAL
    return v


def empty(n_rows):
    return np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32)


def from_rows(rows):
    lens = np.array([len(c) for c in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)
    return rp, ci


def long_rows(n_rows, n_cols, seed, long_cols):
    """5 sorted columns per row, row 17 replaced by `long_cols` (None: left at 5)."""
    rp, ci, _ = uniform_csr(n_rows, n_cols, 5, seed=seed)
    rows = [ci[rp[r]:rp[r + 1]] for r in range(n_rows)]
    if long_cols is not None:
        rows[17] = np.sort(long_cols)
    return from_rows(rows)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(rp_a, ci_a, rp_b, ci_b, n_cols); the second pair None for A + A (one handle on both sides)."""
    if name in ("300x257", "1000x777"):             # one partial 2048-term chunk; three, a row across each boundary
        n_rows, n_cols = (300, 257) if name == "300x257" else (1000, 777)
        a, b = uniform_csr(n_rows, n_cols, 5, seed=7), uniform_csr(n_rows, n_cols, 6, seed=8)
        return a[0], a[1], b[0], b[1], n_cols
    if name == "a_plus_a":
        a = uniform_csr(1000, 777, 5, seed=7)
        return a[0], a[1], None, None, 777
    if name == "disjoint":                          # A on even columns, B on odd ones
        a, b = uniform_csr(300, 128, 5, seed=9), uniform_csr(300, 128, 6, seed=10)
        return a[0], 2 * a[1], b[0], 2 * b[1] + 1, 257
    if name in ("a_empty", "b_empty", "both_empty"):
        a = uniform_csr(300, 257, 5, seed=7)[:2] if name == "b_empty" else empty(300)
        b = uniform_csr(300, 257, 6, seed=8)[:2] if name == "a_empty" else empty(300)
        return a[0], a[1], b[0], b[1], 257
    if name == "no_rows":
        return (*empty(0), *empty(0), 5)
    if name == "one_column":
        r = np.arange(300)
        a = from_rows([[0] if k % 2 == 0 else [] for k in r])
        b = from_rows([[0] if k % 3 == 0 else [] for k in r])
        return a[0], a[1], b[0], b[1], 1
    if name == "a_every_7th_row_empty":
        a, b = uniform_csr(1000, 777, 5, seed=7), uniform_csr(1000, 777, 6, seed=8)
        rows = [a[1][a[0][r]:a[0][r + 1]] if r % 7 else a[1][:0] for r in range(1000)]
        return (*from_rows(rows), b[0], b[1], 777)
    perm = np.random.default_rng(12).permutation(8000)
    if name == "long_a":                            # one 3000-term row against 5 terms
        return (*long_rows(40, 8000, 13, perm[:3000]), *long_rows(40, 8000, 14, None), 8000)
    if name == "long_b":
        return (*long_rows(40, 8000, 13, None), *long_rows(40, 8000, 14, perm[:3000]), 8000)
    if name == "long_both":                         # 3000 against 3000, 1500 of them shared
        return (*long_rows(40, 8000, 13, perm[:3000]), *long_rows(40, 8000, 14, perm[1500:4500]), 8000)
    raise KeyError(name)


PATTERNS = ("300x257", "1000x777", "a_plus_a", "disjoint", "a_empty", "b_empty", "both_empty", "no_rows", "one_column",
            "a_every_7th_row_empty", "long_a", "long_b", "long_both")


# ------------------------------------------------------------------------------- comparisons
def check_against_ref(Cm, a, alpha, b, beta, n_cols, tag):
    """The CSR and the maps of Cm against sum_ref; returns the restated arrays, the NaN results
    carrying the device's payloads (the header leaves a NaN's payload to the hardware)."""
    rp, ci, va, ta, tb = sr.sum_csr(a[0], a[1], a[2], alpha, b[0], b[1], b[2], beta, n_cols)
    g_rp, g_ci, g_va = Cm.csr()
    assert np.array_equal(g_rp, rp), tag + ": row_ptr"
    assert np.array_equal(g_ci, ci), tag + ": col_idx"
    g_ta, g_tb = Cm.sum_terms_device()
    assert g_ta.dtype == g_tb.dtype == torch_dev().int32
    assert np.array_equal(to_host(g_ta), ta), tag + ": terms_a"
    assert np.array_equal(to_host(g_tb), tb), tag + ": terms_b"
    nan = np.isnan(va)
    assert np.array_equal(np.isnan(g_va), nan), tag + ": NaN pattern"
    bad = np.flatnonzero(bits(g_va)[~nan] != bits(va)[~nan])
    assert bad.size == 0, f"{tag}: {bad.size} of {va.size} values differ (bits), first at {bad[:6].tolist()}"
    va = va.copy()
    va[nan] = g_va[nan]
    return rp, ci, va


def same_as_fresh(Cm, F, ops, tag):
    """Cm (summed on the device) is F (from_csr of the restated arrays on the device)."""
    assert Cm == F, tag + ": =="
    assert Cm.layout_digest() == F.layout_digest(), tag + ": layout digest"
    ci_, fi = Cm.info(), F.info()
    assert ci_.pop("device_bytes") >= fi.pop("device_bytes") + 8 * ci_["nnz"], tag + ": the maps are counted"
    assert ci_ == fi, tag + ": info"
    assert ci_["table_size"] == 0 and ci_["has_ref_stream"] == 0
    assert Cm.built_on_device() == F.built_on_device(), tag + ": built_on_device"
    if ci_["n_rows"] == 0:
        return
    for algo in ALGOS:
        yc, yf = ops.y0.clone(), ops.y0.clone()
        Cm.spmv(ops.x, yc, 1.3, 0.7, algo=algo)
        F.spmv(ops.x, yf, 1.3, 0.7, algo=algo)
        assert table_ref.same_bits(yc, yf), f"{tag}: spmv {algo}"


class Xy:
    def __init__(self, n_rows, n_cols):
        rng = np.random.default_rng(11)
        self.x = to_dev(rng.uniform(-1, 1, n_cols).astype(np.float32))
        self.y0 = to_dev(rng.uniform(-1, 1, n_rows).astype(np.float32))


def fresh(sm, rp, ci, va, n_cols, opts=None):
    return sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), n_cols, opts=opts)


# ------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", PATTERNS)
def test_sum_is_the_restatement(sm, name):
    rp_a, ci_a, rp_b, ci_b, n_cols = pattern(name)
    va_a = specials(ci_a.size, 21)
    A = sm.SparseMatrix.from_csr(rp_a, ci_a, va_a, n_cols)
    if rp_b is None:                                # A + A: the same handle twice
        rp_b, ci_b, va_b, B = rp_a, ci_a, va_a, A
        B_nan = sm.SparseMatrix.from_csr(rp_b, ci_b, np.full(ci_b.size, np.nan, np.float32), n_cols)
    else:
        va_b = specials(ci_b.size, 22)
        B = sm.SparseMatrix.from_csr(rp_b, ci_b, va_b, n_cols)
        B_nan = sm.SparseMatrix.from_csr(rp_b, ci_b, np.full(ci_b.size, np.nan, np.float32), n_cols)
    ops = Xy(rp_a.size - 1, n_cols)
    for alpha, beta in COEFS:
        tag = f"{name} ({alpha}, {beta})"
        # beta == 0: a B full of NaN shows that B's values are not read
        Bm, vb = (B_nan, np.full(ci_b.size, np.nan, np.float32)) if beta == 0 else (B, va_b)
        Cm = A.sum(Bm, alpha, beta)
        rp, ci, va = check_against_ref(Cm, (rp_a, ci_a, va_a), alpha, (rp_b, ci_b, vb), beta, n_cols, tag)
        same_as_fresh(Cm, fresh(sm, rp, ci, va, n_cols), ops, tag)
    assert np.array_equal(bits(A.csr()[2]), bits(va_a)), "the operands are untouched"


def test_alpha_zero_leaves_a_unread(sm):
    rp_a, ci_a, rp_b, ci_b, n_cols = pattern("1000x777")
    A = sm.SparseMatrix.from_csr(rp_a, ci_a, np.full(ci_a.size, np.nan, np.float32), n_cols)
    vb = np.random.default_rng(23).uniform(-1, 1, ci_b.size).astype(np.float32)
    B = sm.SparseMatrix.from_csr(rp_b, ci_b, vb, n_cols)
    for beta in (1.0, 2.5, 0.0):
        va = A.sum(B, 0.0, beta).csr()[2]
        assert not np.isnan(va).any()


def test_two_runs_agree(sm):
    rp_a, ci_a, rp_b, ci_b, n_cols = pattern("1000x777")
    A = sm.SparseMatrix.from_csr(rp_a, ci_a, specials(ci_a.size, 21), n_cols)
    B = sm.SparseMatrix.from_csr(rp_b, ci_b, specials(ci_b.size, 22), n_cols)
    C1, C2 = A.sum(B, -0.5, 3.0), A.sum(B, -0.5, 3.0)
    assert C1 == C2 and C1.layout_digest() == C2.layout_digest()
    torch = torch_dev()
    for t1, t2 in zip(C1.sum_terms_device(), C2.sum_terms_device()):
        assert torch.equal(t1, t2)


# ------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("layout", ["band2", "no_bands"])
def test_device_builders_run(sm, layout):
    """layout_specs' shape (20011 x 120001, 8 per row): the summed matrix's layouts are built on the
    device and are those of from_csr on the restated arrays."""
    c, d = layout_specs._base(), layout_specs._plain()          # two patterns of the same shape
    opts = {"layout": layout, "band_slabs": 1} if layout == "band2" else {"layout": layout}
    A = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts={"layout": "no_bands"})
    B = sm.SparseMatrix.from_csr(d.rp, d.ci, d.va, d.n_cols, opts={"layout": "no_bands"})
    Cm = A.sum(B, 1.0, -0.5, opts=opts)
    rp, ci, va = check_against_ref(Cm, (c.rp, c.ci, c.va), 1.0, (d.rp, d.ci, d.va), -0.5, c.n_cols, layout)
    F = fresh(sm, rp, ci, va, c.n_cols, opts)
    assert Cm.built_on_device() != 0, "the device builders ran"
    if layout == "band2":
        assert Cm.info()["has_xband"] == layout_specs.BAND_CODE["band2"]
    same_as_fresh(Cm, F, Xy(c.n_rows, c.n_cols), layout)


def test_updatable(sm):
    rp_a, ci_a, rp_b, ci_b, n_cols = pattern("1000x777")
    va_a, va_b = specials(ci_a.size, 21), specials(ci_b.size, 22)
    A = sm.SparseMatrix.from_csr(rp_a, ci_a, va_a, n_cols)
    B = sm.SparseMatrix.from_csr(rp_b, ci_b, va_b, n_cols)
    opts = {"updatable": 1}
    Cm = A.sum(B, 1.0, 1.0, opts=opts)
    assert Cm.info()["updatable"] == 1
    rp, ci, va = check_against_ref(Cm, (rp_a, ci_a, va_a), 1.0, (rp_b, ci_b, va_b), 1.0, n_cols, "updatable")
    ops = Xy(rp_a.size - 1, n_cols)
    same_as_fresh(Cm, fresh(sm, rp, ci, va, n_cols, opts), ops, "updatable")
    new = np.random.default_rng(24).uniform(-1, 1, ci.size).astype(np.float32)
    Cm.set_values(to_dev(new))
    same_as_fresh(Cm, fresh(sm, rp, ci, new, n_cols, opts), ops, "updatable, set_values")
    g_rp, g_ci, g_va = Cm.csr()
    assert np.array_equal(g_rp, rp) and np.array_equal(g_ci, ci) and np.array_equal(bits(g_va), bits(new))
    _, _, ta, tb = sr.union(rp_a, ci_a, rp_b, ci_b, n_cols)
    g_ta, g_tb = Cm.sum_terms_device()
    assert np.array_equal(to_host(g_ta), ta) and np.array_equal(to_host(g_tb), tb), "the maps stay"
    from sparsematrix_amd import _lib
    L = _lib.load()
    assert L.sm_set_values(Cm._h, to_dev(new).data_ptr(), _lib.SM_VALUES_SOURCE, None) == NOT_SUPPORTED   # no single source
    assert status_of(Cm.source_terms_device) == NOT_SUPPORTED
    torch_dev().cuda.synchronize()


# ------------------------------------------------------------------------------- sources
def test_table_and_dense_index_sources(sm):
    rng = np.random.default_rng(25)
    rows, cols, T = 300, 257, 63
    dm = np.where(rng.random((rows, cols)) < 0.05, rng.integers(0, T, (rows, cols)), 255).astype(np.uint8)
    table = rng.uniform(-1, 1, T).astype(np.float32)
    Dx = sm.SparseMatrix(dm, rows, cols, cols, table, T)         # a dense-index (CopyForm) matrix
    assert Dx.info()["has_ref_stream"] == 1 and Dx.info()["table_size"] == T
    d_rp, d_ci, d_va = Dx.csr()
    n_rows, n_cols = Dx.info()["n_rows"], Dx.info()["n_cols"]
    t_rp, t_ci, _ = uniform_csr(n_rows, n_cols, 6, seed=26)
    tab = rng.uniform(-1, 1, 7).astype(np.float32)
    ids = rng.integers(0, 7, t_ci.size).astype(np.uint8)
    Tm = sm.SparseMatrix.from_csr_ids(t_rp, t_ci, ids, tab, n_cols)   # a table matrix
    assert Tm.info()["table_size"] == 7
    ops = Xy(n_rows, n_cols)
    for (X, x), (Y, y), tag in (((Dx, (d_rp, d_ci, d_va)), (Tm, (t_rp, t_ci, tab[ids])), "index + table"),
                                ((Tm, (t_rp, t_ci, tab[ids])), (Dx, (d_rp, d_ci, d_va)), "table + index")):
        Cm = X.sum(Y, 2.0, -1.0)
        rp, ci, va = check_against_ref(Cm, x, 2.0, y, -1.0, n_cols, tag)
        same_as_fresh(Cm, fresh(sm, rp, ci, va, n_cols), ops, tag)   # table_size == 0 and has_ref_stream == 0 inside


def test_refusals(sm):
    from sparsematrix_amd import _lib
    torch = torch_dev()
    L = _lib.load()
    rp, ci, va = messy_csr("shuffled_repeated", seed=27)
    n_rows, n_cols = rp.size - 1, 40000
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    g_rp, g_ci, g_va = uniform_csr(n_rows, n_cols, 4, seed=28)
    G = sm.SparseMatrix.from_csr(g_rp, g_ci, g_va, n_cols)
    assert status_of(lambda: M.sum(G)) == NOT_SUPPORTED and b"operand a" in L.sm_last_error()
    assert status_of(lambda: G.sum(M)) == NOT_SUPPORTED and b"operand b" in L.sm_last_error()
    assert status_of(lambda: M.sum(M)) == NOT_SUPPORTED
    for shape in ((n_rows + 1, n_cols), (n_rows, n_cols + 1)):
        e_rp, e_ci = empty(shape[0])
        E = sm.SparseMatrix.from_csr(e_rp, e_ci, np.zeros(0, np.float32), shape[1])
        assert status_of(lambda: G.sum(E)) == INVALID and status_of(lambda: E.sum(G)) == INVALID
    assert status_of(lambda: G.sum(G, opts={"table_updatable": 1})) == INVALID
    assert status_of(G.sum_terms_device) == NOT_SUPPORTED       # a from_csr matrix holds no sum maps
    t = torch.empty(g_ci.size, dtype=torch.int32, device="cuda")
    assert L.sm_copy_sum_terms_device(G._h, t.data_ptr(), t.data_ptr(), None) == NOT_SUPPORTED
    assert b"sm_create_sum" in L.sm_last_error()
    with pytest.raises(TypeError):
        G.sum(g_va)
    torch.cuda.synchronize()


def test_map_copies_stay_inside_their_buffers(sm):
    torch = torch_dev()
    from sparsematrix_amd import _lib
    L = _lib.load()
    rp_a, ci_a, rp_b, ci_b, n_cols = pattern("300x257")
    A = sm.SparseMatrix.from_csr(rp_a, ci_a, specials(ci_a.size, 21), n_cols)
    B = sm.SparseMatrix.from_csr(rp_b, ci_b, specials(ci_b.size, 22), n_cols)
    Cm = A.sum(B)
    _, _, ta, tb = sr.union(rp_a, ci_a, rp_b, ci_b, n_cols)
    nnz = ta.size
    assert Cm.nnz == nnz
    FILL = -0x5A5A5A5B

    def guarded():
        parent = torch.full((GUARD + nnz + GUARD,), FILL, dtype=torch.int32, device="cuda")
        return parent[GUARD: GUARD + nnz], parent

    def intact(parent):
        w = to_host(parent)
        return (w[:GUARD] == FILL).all() and (w[GUARD + nnz:] == FILL).all()

    stream = torch.cuda.current_stream().cuda_stream
    (va_, pa), (vb_, pb) = guarded(), guarded()
    _lib.check(L.sm_copy_sum_terms_device(Cm._h, va_.data_ptr(), vb_.data_ptr(), stream), "both maps")
    assert np.array_equal(to_host(va_), ta) and np.array_equal(to_host(vb_), tb) and intact(pa) and intact(pb)
    (va_, pa), (vb_, pb) = guarded(), guarded()
    _lib.check(L.sm_copy_sum_terms_device(Cm._h, va_.data_ptr(), None, stream), "terms_a only")
    assert np.array_equal(to_host(va_), ta) and intact(pa)
    _lib.check(L.sm_copy_sum_terms_device(Cm._h, None, vb_.data_ptr(), stream), "terms_b only")
    assert np.array_equal(to_host(vb_), tb) and intact(pb)
    _lib.check(L.sm_copy_sum_terms_device(Cm._h, None, None, stream), "neither")
    E = A.sum(A, opts=None).pruned(keep=0)                       # not a sum matrix any more
    assert L.sm_copy_sum_terms_device(E._h, None, None, stream) == NOT_SUPPORTED
    e_rp, e_ci = empty(rp_a.size - 1)
    Z = sm.SparseMatrix.from_csr(e_rp, e_ci, np.zeros(0, np.float32), n_cols)
    ZZ = Z.sum(Z)                                                # nnz == 0: SM_OK, nothing launched
    assert L.sm_copy_sum_terms_device(ZZ._h, None, None, stream) == 0
    assert all(t.numel() == 0 for t in ZZ.sum_terms_device())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the regrow step
def test_regrow_end_to_end(sm):
    """Prune-and-regrow of dynamic sparse training at 64 x 96: the candidates from |grad|, A's values
    on the union, momentum carried through terms_a, one update step -- against numpy."""
    torch = torch_dev()
    rng = np.random.default_rng(29)
    W = rng.uniform(-1, 1, (64, 96)).astype(np.float32)
    grad = rng.uniform(-1, 1, (64, 96)).astype(np.float32)
    up = {"updatable": 1}
    A = sm.SparseMatrix.from_dense(to_dev(W), per_row=8, opts=up)
    G = sm.SparseMatrix.from_dense(to_dev(np.abs(grad)), keep=100)
    Cm = A.sum(G, 1.0, 0.0, opts=up)
    dense_a, dense_c = A.dense_device(), Cm.dense_device()
    assert table_ref.same_bits(dense_a, dense_c), "A's values on the union pattern, the new positions at +0.0"
    a_rp, a_ci, a_va = A.csr()
    g_rp, g_ci, _ = G.csr()
    pos_a = set(zip(np.repeat(np.arange(64), np.diff(a_rp)).tolist(), a_ci.tolist()))
    pos_g = set(zip(np.repeat(np.arange(64), np.diff(g_rp)).tolist(), g_ci.tolist()))
    assert Cm.nnz == len(pos_a | pos_g) and len(pos_g) == 100 and len(pos_a) == 64 * 8
    # momentum laid out for A moves to C through terms_a; new positions start at 0
    mom_a = rng.uniform(-1, 1, a_va.size).astype(np.float32)
    ta, tb = Cm.sum_terms_device()
    d_mom = to_dev(mom_a)
    mom_c = torch.where(ta >= 0, d_mom[ta.clamp(min=0).long()], torch.zeros((), device="cuda"))
    Cm.axpy_values(-0.1, mom_c)
    # the same in numpy, on the dense matrix
    c_rp, c_ci, _ = Cm.csr()
    h_ta = to_host(ta)
    h_mom_c = np.where(h_ta >= 0, mom_a[np.maximum(h_ta, 0)], np.float32(0)).astype(np.float32)
    old = np.where(h_ta >= 0, a_va[np.maximum(h_ta, 0)], np.float32(0)).astype(np.float32)
    want_vals = table_ref.axpy_reference(old, -0.1, h_mom_c)
    want = np.zeros((64, 96), np.float32)
    want[np.repeat(np.arange(64), np.diff(c_rp)), c_ci] = want_vals
    got = to_host(Cm.dense_device())
    # dense_device(trans=True) is B = S^T: n_rows x n_cols, as from_dense took it
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert np.array_equal(to_host(tb) >= 0, np.array([(r, c) in pos_g for r, c in
                                                      zip(np.repeat(np.arange(64), np.diff(c_rp)).tolist(), c_ci.tolist())]))
