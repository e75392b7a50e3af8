"""Operand placement through the C ABI (include/sparsematrix.h: "plain pointers and sizes
only"): x / y / X / Y that are only 4-byte aligned, padded leading dimensions that are
multiples of 4, and SpMVs captured into a graph as bench.py times them.

Every operand lives inside a parent allocation between guard words (gpu_util.placed): a store
one row too far, or into a padding column, shows as a changed guard.  Expected values come
from code outside the kernel under test: oracle.csr_spmv / csr_spmm / RefModel where the
header promises the reference's order, gpu_util.slab_order_for for several slabs, and
1e-6 * sum|terms| (gpu_util.TOL) for the rest.  Matrix shape: 20011 rows (3 mod 4, two row
blocks of <= 16384), 8 terms per row, every 50th row empty with y = -0.0 there.
"""
import functools

import numpy as np
import pytest

import oracle
from gpu_util import (assert_guards, assert_guards_2d, assert_terms_close, bits, placed, placed_2d,
                      slab_order_for, to_dev, to_host, torch_dev)
from layout_specs import (N_COLS, SPECS, _band_spec, _build, _csr_spec, _long_sell, _pos, _ragged, _same,
                          _sell_spec)

pytestmark = pytest.mark.gpu

OFFSETS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 3)]      # (x_off, y_off) in floats
SCALARS = [(1.3, 0.7), (1.0, 1.0), (0.5, 0.0)]


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _spmv_at(M, case, xs, alpha, beta, algo, x_off, y_off):
    """One product with x at x_off and y at y_off floats past 16-byte alignment; y's guards
    checked.  Returns the host copy of y."""
    yv, yp = placed(case.y_in(beta), y_off)
    M.spmv(xs[x_off][0], yv, alpha, beta, algo=algo)
    got = to_host(yv).copy()
    assert_guards(yp, y_off, case.n_rows)
    return got


# ---------------------------------------------------------------------------- 1. SpMV
@pytest.mark.parametrize("name", list(SPECS))
def test_spmv_operand_offsets(sm, name):
    """Every layout and algorithm at every (x_off, y_off) and (alpha, beta).

    Aligned x (and the layouts without an alignment rule): rows inside the documented limits
    are bit-identical to oracle.csr_spmv (one slab, exact, sweep, ccsell, parity, exact; sell
    rows up to its segment cap, stream rows up to 64 terms, merge rows inside one thread),
    several slabs to gpu_util.slab_order_for, and every offset pair gives the bits of (0, 0).
    Unaligned x on a band layout: AUTO / XBAND run the next kernel of the fall-back chain
    (sell, else stream) and must equal that algo at offset 0 bit for bit; EXACT stays
    bit-identical to the oracle.  Everything is within 1e-6 * sum|terms| of the oracle, y's
    guards are checked after every call, x's once per matrix.

    Widths: 120001 columns everywhere (no forced slab count needed more) except blocked and
    gather, built at 400000 columns for 7 slabs instead of the 2 they get at 120001."""
    spec = SPECS[name]()
    M, info = _build(sm, spec)
    c = spec.case
    multi = spec.band and info["xband_slabs"] > 1
    fallback = "sell" if info["sell_slices"] > 0 or info["ccsell_chunks"] > 0 else "stream"
    xs = {off: placed(c.x, off) for off in sorted({o for o, _ in OFFSETS})}
    for alpha, beta in SCALARS:
        want, absum = c.ref(alpha, beta)
        fb = None
        if spec.band:   # the fall-back kernel's own result: the reference's order on these rows
            fb = _spmv_at(M, c, xs, alpha, beta, fallback, 0, 0)
            _same(fb, want, c.lens <= 64, f"{name} {fallback} at offset 0 vs oracle")
        for algo in spec.algos:
            base = None
            for x_off, y_off in OFFSETS:
                got = _spmv_at(M, c, xs, alpha, beta, algo, x_off, y_off)
                tag = f"{name} {algo} x+{x_off} y+{y_off} alpha {alpha} beta {beta}"
                assert_terms_close(got, want, absum)
                moved = spec.band and x_off != 0
                if algo == "exact":
                    _same(got, want, None, tag + " vs oracle")
                elif moved:
                    _same(got, fb, None, tag + f" vs {fallback} at offset 0")
                elif multi:
                    _same(got, c.slab_ref(info, alpha, beta), None, tag + " vs slab order")
                else:
                    _same(got, want, spec.masks[algo], tag + " vs oracle")
                if (x_off, y_off) == (0, 0):
                    base = got
                elif not moved:
                    _same(got, base, None, tag + " vs offsets (0, 0)")
    for off, (xv, xp) in xs.items():
        assert_guards(xp, off, c.n_cols)
        assert np.array_equal(bits(to_host(xv)), bits(c.x)), "x was written"


# ---------------------------------------------------------------------------- 2. SpMM
@functools.lru_cache(maxsize=None)
def _panel(n_rows, n_rhs):
    n_cols = 5000
    rng = np.random.default_rng(100 + n_rhs)
    X = rng.uniform(-1, 1, (n_cols, n_rhs)).astype(np.float32)
    X[::3] = 0.0
    X[1::9] = -0.0
    Y0 = rng.uniform(-1, 1, (n_rows, n_rhs)).astype(np.float32)
    Y0[::4] = -0.0
    return X, Y0


SPMM_SCALARS = [(1.3, 0.7), (-2.0, 0.0)]


@functools.lru_cache(maxsize=None)
def _spmm_ref(n_rows, n_rhs, alpha, beta):
    rp, ci, va, _ = _ragged(n_rows)
    X, Y0 = _panel(n_rows, n_rhs)
    return oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)


@functools.lru_cache(maxsize=None)
def _spmm_absum(n_rows, n_rhs, alpha, beta):
    rp, ci, va, _ = _ragged(n_rows)
    X, Y0 = _panel(n_rows, n_rhs)
    ab = np.empty(Y0.shape, np.float64)
    for j in range(n_rhs):
        _, a = oracle.csr_spmv_f64(rp.astype(np.int64), ci, va, np.ascontiguousarray(X[:, j]),
                                   np.ascontiguousarray(Y0[:, j]), alpha, beta)
        ab[:, j] = a
    return ab


def _spmm_placed(sm, n_rows, n_rhs, ldx, ldy, x_off, y_off, algos, exact=True):
    rp, ci, va, n_cols = _ragged(n_rows)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    X, Y0 = _panel(n_rows, n_rhs)
    Xv, Xp = placed_2d(X, ldx, x_off)
    for algo in algos:
        for alpha, beta in SPMM_SCALARS:
            Yv, Yp = placed_2d(Y0, ldy, y_off)
            M.spmm(Xv, Yv, alpha, beta, algo=algo)
            got = to_host(Yv)
            want = _spmm_ref(n_rows, n_rhs, alpha, beta)
            tag = f"{algo} N {n_rhs} ld ({ldx}, {ldy}) off ({x_off}, {y_off}) alpha {alpha} beta {beta}"
            if exact:
                _same(got, want, None, tag)
            else:
                assert_terms_close(got, want, _spmm_absum(n_rows, n_rhs, alpha, beta))
            assert_guards_2d(Yp, y_off, n_rows, n_rhs, ldy)
    assert_guards_2d(Xp, x_off, n_cols, n_rhs, ldx)
    assert np.array_equal(bits(to_host(Xv)), bits(X)), "X was written"


@pytest.mark.parametrize("n_rows", [3000, 3003])
@pytest.mark.parametrize("n_rhs", [4, 16, 32, 128])
def test_spmm_rowpanel_padded_ld(sm, n_rows, n_rhs):
    """ldx = n_rhs + 4, ldy = n_rhs + 8 with 16-byte aligned bases: the vec_ok conditions hold,
    so "auto" and "vector" run the two row-panel kernels on padded rows (and X's buffer range
    x_rows * ldx).  Bit-exact against oracle.csr_spmm; padding columns and guards unchanged."""
    _spmm_placed(sm, n_rows, n_rhs, n_rhs + 4, n_rhs + 8, 0, 0, ("auto", "vector"))


@pytest.mark.parametrize("n_rows", [3000, 3003])
@pytest.mark.parametrize("n_rhs", [4, 16, 32, 128])
@pytest.mark.parametrize("x_off,y_off", [(1, 0), (0, 1)])
def test_spmm_generic_unaligned_base(sm, n_rows, n_rhs, x_off, y_off):
    """The same shapes with X or Y one float past 16-byte alignment: vec_ok is false at a
    multiple-of-4 n_rhs and the generic kernel runs.  Bit-exact against the oracle."""
    _spmm_placed(sm, n_rows, n_rhs, n_rhs + 4, n_rhs + 8, x_off, y_off, ("auto",))


@pytest.mark.parametrize("n_rows", [3000, 3003])
def test_spmm_mfma_legal_minimum(sm, n_rows):
    """SM_ALGO_MFMA at the least it accepts: X and Y 8-byte but not 16-byte aligned, even
    leading dimensions 34 and 38 (its float2 accesses; X staged without the LDS form).  Within
    1e-6 * sum|terms| of the oracle; padding columns and guards unchanged."""
    _spmm_placed(sm, n_rows, 32, 34, 38, 2, 2, ("mfma",), exact=False)


@pytest.mark.parametrize("ldx,x_off,y_off", [(34, 1, 2), (34, 2, 1), (35, 2, 2)])
def test_spmm_mfma_rejects_placement(sm, ldx, x_off, y_off):
    """A 4-byte aligned X or Y, or an odd ldx: SM_ERR_NOT_SUPPORTED, Y bit-unchanged."""
    torch = torch_dev()
    rp, ci, va, n_cols = _ragged(3003)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    X, Y0 = _panel(3003, 32)
    Xv, _ = placed_2d(X, ldx, x_off)
    Yv, Yp = placed_2d(Y0, 38, y_off)
    before = Yp.view(torch.int32).cpu().numpy().copy()
    with pytest.raises(sm.SparseMatrixError) as ei:
        M.spmm(Xv, Yv, 1.3, 0.7, algo="mfma")
    assert ei.value.status == 4
    torch.cuda.synchronize()
    assert np.array_equal(Yp.view(torch.int32).cpu().numpy(), before)


# ---------------------------------------------------------------------------- 2b. AddMatMat
@functools.lru_cache(maxsize=None)
def _dense_index():
    """300 x 257 ids at 5 % density over a 255-entry table (S = the index, NoTrans)."""
    rng = np.random.default_rng(300 + 257)
    rows, cols, T = 300, 257, 255
    table = rng.uniform(-1, 1, T).astype(np.float32)
    dm = np.where(rng.random((rows, cols)) < 0.05, rng.integers(0, T, (rows, cols)), 255).astype(np.uint8)
    return dm, rows, cols, table, T


@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("algo", ["auto", "exact", "parity", "native"])
def test_addmatmat_odd_leading_dimensions(sm, m, algo):
    """C (m x 257, ldc 258) = alpha A (m x 300, lda 303) S + beta C on a dense-index matrix.
    With m <= 2 the narrow-matrix route runs SpMVs on a + i lda and c + i ldc: row 1 is an x
    12 bytes and a y 8 bytes past 16-byte alignment.  Every algo is bit-identical to the
    reference's AddMatMat (oracle.RefModel); A's padding columns hold NaN (the guard pattern),
    C's padding columns and guards are unchanged."""
    dm, rows, cols, table, T = _dense_index()
    M = sm.SparseMatrix(dm, rows, cols, cols, table, T, sm.SblasNoTrans)
    ref = oracle.RefModel(dm, rows, cols, cols, table, T, trans=False)
    k, n = M.NumRows(), M.NumCols()
    assert (k, n) == (300, 257)
    lda, ldc = k + 3, n + 1
    rng = np.random.default_rng(m)
    A = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    C = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    A_full = np.zeros((m, lda), np.float32)
    A_full[:, :k] = A
    C_full = np.zeros((m, ldc), np.float32)
    C_full[:, :n] = C
    Av, Ap = placed_2d(A, lda, 0)
    for alpha, beta in ((1.3, 0.7), (1.0, 0.0)):
        want = ref.add_mat_mat(A_full.reshape(-1), m, lda, C_full.reshape(-1), ldc, alpha, beta)
        Cv, Cp = placed_2d(C, ldc, 0)
        # the m x ld storage behind the views, flat (the C ABI takes a pointer and ld)
        a_flat, c_flat = Av.as_strided((m * lda,), (1,)), Cv.as_strided((m * ldc,), (1,))
        assert a_flat.data_ptr() == Av.data_ptr() and c_flat.data_ptr() == Cv.data_ptr()
        M.AddMatMat(a_flat, m, lda, c_flat, ldc, alpha, beta, algo=algo)
        _same(to_host(Cv), want.reshape(m, ldc)[:, :n], None, f"{algo} m {m} alpha {alpha} beta {beta}")
        assert_guards_2d(Cp, 0, m, n, ldc)
    assert_guards_2d(Ap, 0, m, k, lda)
    assert np.array_equal(bits(to_host(Av)), bits(A)), "A was written"


# ---------------------------------------------------------------------------- 3. graphs
GRAPH_K, GRAPH_REPLAYS, GRAPH_WARMUP = 6, 3, 2

GRAPH_SPECS = {
    "cband-3slabs": lambda: (_band_spec("cband", N_COLS, band_tall=0, band_slabs=3), "auto"),
    "gcb-3slabs": lambda: (_band_spec("gcb", N_COLS, band_slabs=3), "auto"),
    "sell-relabel-long": lambda: (_sell_spec(_long_sell(), 2048,
                                             dict(sell_slices=_pos, col_relabel=1, n_long_rows=_pos),
                                             relabel=1), "auto"),
    "merge-long": lambda: (_csr_spec(0), "merge"),
}


@pytest.mark.parametrize("name", list(GRAPH_SPECS))
def test_spmv_captured_graph_vs_oracle(sm, name):
    """What bench.py times: after two eager products, K = 6 products y_r <- 0.5 y_r + B x_r
    (two (x, y) replicas in turn) captured into one linear graph by torch.cuda.graph and
    replayed three times.  Inside a capture sm_spmv skips the scratch-ordering event, every
    replay advances the band2 / cband epoch counter, and the relabeled x and the partial sums
    are reused from node to node.  After each replay both y are compared with the same 8 / 14 /
    20 products restated on the CPU -- gpu_util.slab_order_for bit for bit on the band layouts;
    oracle.csr_spmv on the others, bit for bit on the rows inside the kernel's exact limit and
    within the bound on the rest -- and the 20 products run eagerly give the graph's bits.

    The bound for an iterated product: with e_j the error of y after j products of a replica
    and T = sum|alpha v x|, e_j <= 0.5 e_{j-1} + 1e-6 (0.5 |y_{j-1}| + T), so
    e_j <= 1e-6 A_j with A_j = 0.5 A_{j-1} + (0.5 |y_{j-1}| + T), A_0 = 0 (the second term is
    oracle.csr_spmv_f64's sum|terms| of product j)."""
    torch = torch_dev()
    spec, algo = GRAPH_SPECS[name]()
    M, info = _build(sm, spec)
    c = spec.case
    multi = spec.band and info["xband_slabs"] > 1
    if spec.band:
        assert multi, info
    rng = np.random.default_rng(77)
    xh = [c.x, rng.uniform(-1, 1, c.n_cols).astype(np.float32)]
    yh = [c.y0.copy(), rng.uniform(-1, 1, c.n_rows).astype(np.float32)]
    xd = [to_dev(x) for x in xh]
    total = GRAPH_WARMUP + GRAPH_K * GRAPH_REPLAYS

    def product(ys, i):
        M.spmv(xd[i % 2], ys[i % 2], 1.0, 0.5, algo=algo)

    # the graph
    yg = [to_dev(y) for y in yh]
    for i in range(GRAPH_WARMUP):
        product(yg, i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(GRAPH_WARMUP, GRAPH_WARMUP + GRAPH_K):
            product(yg, i)
    torch.cuda.synchronize()
    snaps = []
    for _ in range(GRAPH_REPLAYS):
        graph.replay()
        torch.cuda.synchronize()
        snaps.append([to_host(y).copy() for y in yg])
    # the same products eagerly
    ye = [to_dev(y) for y in yh]
    for i in range(total):
        product(ye, i)
    eager = [to_host(y).copy() for y in ye]
    # the same products on the CPU
    ys = [y.copy() for y in yh]
    A = [np.zeros(c.n_rows), np.zeros(c.n_rows)]
    mask = None if multi else spec.masks[algo]
    for i in range(total):
        r = i % 2
        _, absum = oracle.csr_spmv_f64(c.rp, c.ci, c.va, xh[r], ys[r], 1.0, 0.5)
        A[r] = 0.5 * A[r] + absum
        if multi:
            ys[r] = slab_order_for(info, c.rp, c.ci, c.va, xh[r], ys[r], 1.0, 0.5)
        else:
            ys[r] = oracle.csr_spmv(c.rp, c.ci, c.va, xh[r], ys[r], 1.0, 0.5)
        done = i + 1 - GRAPH_WARMUP
        if done > 0 and done % GRAPH_K == 0:
            snap = snaps[done // GRAPH_K - 1]
            for q in range(2):
                tag = f"{name} replay {done // GRAPH_K} replica {q}"
                _same(snap[q], ys[q], mask, tag)
                assert_terms_close(snap[q], ys[q], A[q])
    for q in range(2):
        _same(eager[q], snaps[-1][q], None, f"{name} eager vs graph, replica {q}")
