"""Every product kernel at the edges of the float range (tests/range_edges.py): subnormal terms
and sums, fl(v * alpha) that underflows or overflows, sums that overflow midway, alpha = inf.

Where include/sparsematrix.h says "bit-identical" the outputs are compared with
assert_same_nanclass (NaN where the reference has one, every other output by bits) against the
oracle or the restatement the operand tests already use; where it gives the sum|terms| bound,
and only in the regimes whose terms stay finite (`subnormal`, `fold_under`), with
assert_sum_close against the rounded terms, which has no absolute slack beyond one rounding of
the smallest subnormal per fused term.  The inputs themselves are held to what the regimes
are named for by tests/test_range_edges_cpu.py.
"""
import dataclasses
import functools

import numpy as np
import pytest

import oracle
import range_edges as re_
import sddmm_ref
import table_ref
from gpu_util import bits, to_dev, to_host, torch_dev, uniform_csr
from layout_specs import SPECS, _build, _ragged
from range_edges import REGIMES, assert_same_nanclass, assert_sum_close
from table_ref import axpy_reference
from test_gpu_table import T_UPD, ids_for_update, uniform_ids
from test_gpu_update_values import Operands as ValueOperands
from test_gpu_update_values import assert_same_matrix as assert_same_values_matrix
from test_gpu_update_values import pattern

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _rng(regime, salt):
    """One stream per (regime, use): the registry's cases draw from range_edges.draw itself."""
    return np.random.default_rng([re_.SEED, sorted(REGIMES).index(regime) if regime in REGIMES else 99, salt])


# ---------------------------------------------------------------------------- 1. SpMV
_CASES = {}


def _regime_case(case, regime):
    """The regime's data on a registry case (cached there), shared by the specs that share it."""
    if (id(case), regime) not in _CASES:
        _CASES[id(case), regime] = case.with_data(*re_.draw(regime, case.va, case.n_cols, case.n_rows))
    return _CASES[id(case), regime]


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", list(SPECS))
def test_spmv(sm, name, regime):
    """Every layout of the registry, every algorithm of the layout, aligned operands, one build
    per regime.  Rows inside the documented limits (spec.masks) against oracle.csr_spmv, several
    slabs against the slab-order restatement; in `subnormal` and `fold_under` every row of every
    algorithm also against the rounded terms.  Where sums overflow, rows outside a mask are not
    compared: the bound says nothing there."""
    spec = SPECS[name]()
    c = _regime_case(spec.case, regime)
    spec = dataclasses.replace(spec, case=c)
    M, info = _build(sm, spec)
    multi = spec.band and info["xband_slabs"] > 1
    xd = to_dev(c.x)
    empty = c.lens == 0
    for alpha, beta in REGIMES[regime].scalars:
        y0 = c.y_in(beta)
        want = oracle.csr_spmv(c.rp, c.ci, c.va, c.x, y0, alpha, beta)
        terms = re_.rounded_terms(c.rp, c.ci, c.va, c.x, y0, alpha, beta) if regime in re_.BOUND_REGIMES else None
        seeded = np.isnan(y0)
        for algo in spec.algos:
            yd = to_dev(y0)
            M.spmv(xd, yd, alpha, beta, algo=algo)
            got = to_host(yd).copy()
            tag = f"{name} {algo} {regime} alpha {alpha} beta {beta}"
            if regime == "fold_over":
                print(f"{tag}: generated NaN bits {re_.nan_patterns(got)}")
            if algo != "exact" and multi:
                ref, mask = c.slab_ref(info, alpha, beta), None
            else:
                ref, mask = want, (None if algo == "exact" else spec.masks[algo])
            assert_same_nanclass(got, ref, mask, tag)
            if terms is not None:
                assert np.isnan(got[seeded]).all(), tag
                s, ab, n_r = (t[~seeded] for t in terms)
                assert_sum_close(got[~seeded], s, ab, n_r, tag)
            if regime == "alpha_inf":
                assert np.array_equal(bits(got)[empty], bits(c.y0)[empty]), tag + ": an empty row changed"
                if not multi or algo == "exact":
                    rows = ~empty if mask is None else (~empty & mask)
                    assert (bits(got)[rows] == INF_BITS).all(), tag + ": a row is not +inf"
                else:
                    assert (bits(ref)[~empty] == INF_BITS).all()
    assert np.array_equal(bits(to_host(xd)), bits(c.x)), "x was written"


# ---------------------------------------------------------------------------- 2. SpMM
@functools.lru_cache(maxsize=None)
def _ragged_regime(n_rows, regime):
    """_ragged's pattern with one value per term, and X / Y0 panels of 128 columns whose
    leading columns serve the narrower widths."""
    rp, ci, va, n_cols = _ragged(n_rows)
    reg, rng = REGIMES[regime], _rng(regime, n_rows)
    return (rp, ci, re_.values_like(rng, reg, va), n_cols,
            reg.draw_x(rng, (n_cols, 128)), reg.draw_y0(rng, (n_rows, 128)))


def _panels(n_rows, regime, n_rhs):
    rp, ci, va, n_cols, X, Y0 = _ragged_regime(n_rows, regime)
    return rp, ci, va, n_cols, np.ascontiguousarray(X[:, :n_rhs]), np.ascontiguousarray(Y0[:, :n_rhs])


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("n_rows", [3000, 3003])
def test_spmm(sm, n_rows, regime):
    """n_rhs 4 and 32 (the gather-pipelined row panel under "auto", the plain panel under
    "vector"), 128 (the plain panel under both) and 33 (the generic kernel): every output
    against oracle.csr_spmm."""
    rp, ci, va, n_cols, _, _ = _ragged_regime(n_rows, regime)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    for n_rhs, algos in ((4, ("auto", "vector")), (32, ("auto", "vector")), (128, ("auto", "vector")),
                         (33, ("auto",))):
        *_, X, Y0 = _panels(n_rows, regime, n_rhs)
        Xd = to_dev(X)
        for alpha, beta in REGIMES[regime].scalars:
            want = oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)
            for algo in algos:
                Yd = to_dev(Y0)
                M.spmm(Xd, Yd, alpha, beta, algo=algo)
                assert_same_nanclass(to_host(Yd), want, None, f"{algo} N {n_rhs} {regime} alpha {alpha} beta {beta}")


def _column_terms(rp, ci, va, X, Y0, alpha, beta):
    s, ab = np.empty(Y0.shape), np.empty(Y0.shape)
    for j in range(Y0.shape[1]):
        s[:, j], ab[:, j], n_r = re_.rounded_terms(rp, ci, va, X[:, j], Y0[:, j], alpha, beta)
    return s, ab, n_r[:, None]


def _zero_sign_free(a):
    """As tests/test_gpu_spmm_mfma.py: a tile's other rows' zero A entries add fma(0, x, acc),
    which turns an accumulator of -0.0 into +0.0."""
    b = bits(a).copy()
    b[b == 0x80000000] = 0
    return b


@pytest.mark.parametrize("regime", re_.BOUND_REGIMES)
@pytest.mark.parametrize("n_rows", [3000, 3003])
def test_spmm_mfma(sm, n_rows, regime):
    """SM_ALGO_MFMA (finite X only): the fma-chain model by bits, and the rounded terms' bound
    per output."""
    rp, ci, va, n_cols, X, Y0 = _panels(n_rows, regime, 32)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    Xd = to_dev(X)
    for alpha, beta in REGIMES[regime].scalars:
        Yd = to_dev(Y0)
        M.spmm(Xd, Yd, alpha, beta, algo="mfma")
        got = to_host(Yd)
        tag = f"mfma {regime} alpha {alpha} beta {beta}"
        assert_sum_close(got, *_column_terms(rp, ci, va, X, Y0, alpha, beta), tag)
        model = oracle.csr_spmm_fma(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)
        bad = np.flatnonzero(_zero_sign_free(got) != _zero_sign_free(model))
        assert bad.size == 0, f"{tag}: {bad.size} of {got.size} outputs differ from the fma chain, first {bad[:5].tolist()}"


# ---------------------------------------------------------------------------- 3. AddMatMat
@functools.lru_cache(maxsize=None)
def _dense_index(regime, zeros):
    """300 x 257 ids at density 0.1 over the regime's 255-entry table, with one 0.0 and one -0.0
    entry when `zeros`."""
    rng = _rng(regime, 257)
    rows, cols, T = 300, 257, 255
    table = REGIMES[regime].table(rng, T)
    if zeros:
        table[17], table[201] = 0.0, -0.0
    dm = np.where(rng.random((rows, cols)) < 0.1, rng.integers(0, T, (rows, cols)), 255).astype(np.uint8)
    assert (dm == 17).any() and (dm == 201).any()
    return dm, rows, cols, table, T


ADDMATMAT_RUNS = [(r, True) for r in REGIMES] + [("alpha_inf", False)]


@pytest.mark.parametrize("trans", [False, True], ids=["n", "t"])
@pytest.mark.parametrize("regime,zeros", ADDMATMAT_RUNS, ids=[f"{r}-{'zeros' if z else 'nozeros'}"
                                                               for r, z in ADDMATMAT_RUNS])
def test_addmatmat(sm, regime, zeros, trans):
    """C = alpha A S + beta C on a dense-index matrix, m in {1, 3, 32}, odd lda / ldc, every
    algorithm and the host entry point against the reference's AddMatMat (oracle.RefModel).
    alpha = inf runs with and without the table's zero entries: with them every output that a
    zero entry reaches is NaN, without them every reached output is +inf."""
    reg = REGIMES[regime]
    dm, rows, cols, table, T = _dense_index(regime, zeros)
    M = sm.SparseMatrix(dm, rows, cols, cols, table, T, sm.SblasTrans if trans else sm.SblasNoTrans)
    ref = oracle.RefModel(dm, rows, cols, cols, table, T, trans=trans)
    k, n = M.NumRows(), M.NumCols()
    assert (k, n) == ((257, 300) if trans else (300, 257))
    assert M.info()["max_row_nnz"] <= 64
    lda, ldc = k + 3, n + 1
    rng = _rng(regime, 1000 + trans)
    for m in (1, 3, 32):
        A_full = reg.draw_x(rng, (m, lda))
        C_full = reg.draw_y0(rng, (m, ldc))
        a_dev = to_dev(A_full.reshape(-1))
        for alpha, beta in reg.scalars:
            want = ref.add_mat_mat(A_full.reshape(-1), m, lda, C_full.reshape(-1), ldc, alpha, beta)
            wv = want.reshape(m, ldc)[:, :n]
            if regime == "alpha_inf" and zeros and m == 1:   # 0 * inf, for include/sparsematrix.h
                c_dev = to_dev(C_full.reshape(-1))
                M.AddMatMat(a_dev, m, lda, c_dev, ldc, alpha, beta, algo="parity")
                print(f"alpha_inf trans {trans}: NaN bits of 0 * inf {re_.nan_patterns(to_host(c_dev))}")
            if regime == "alpha_inf":
                hit = np.isnan(wv) if zeros else (bits(wv) == INF_BITS).reshape(wv.shape)
                assert hit.any() and (zeros or hit.mean() > 0.9)
            tag = f"{regime} trans {trans} m {m} alpha {alpha} beta {beta}"
            for algo in ("parity", "auto", "exact", "native"):
                c_dev = to_dev(C_full.reshape(-1))
                M.AddMatMat(a_dev, m, lda, c_dev, ldc, alpha, beta, algo=algo)
                assert_same_nanclass(to_host(c_dev), want, None, f"{algo} {tag}")
            c_host = C_full.reshape(-1).copy()
            M.AddMatMat(A_full.reshape(-1), m, lda, c_host, ldc, alpha, beta)
            assert_same_nanclass(c_host, want, None, f"host {tag}")


# ---------------------------------------------------------------------------- 4. SDDMM
# alpha * s underflows: G in 2^[-60, -50] and X in 2^[-55, -45] give products of 2^-115 .. 2^-93 and
# dots of up to 33 of them below 2^-88, so fl(alpha * s) with alpha = 1.3 * 2^-40 stays below 2^-127:
# subnormal (at N = 1 about one in eight underflows to zero); out0 is subnormal too, so the last sum
# stays there.
ALPHA_UNDER = re_.Regime((-60, -50, True), (-55, -45, True), (-140, -127, True),
                         ((re_.A_UNDER, 0.7), (re_.A_UNDER, 1.0)))
SDDMM_REGIMES = {"subnormal": REGIMES["subnormal"], "midsum_over": REGIMES["midsum_over"],
                 "alpha_under": ALPHA_UNDER}
SDDMM_N = (1, 4, 32, 33)


@pytest.fixture(scope="module")
def grid_case(sm):
    rp, ci, va = uniform_csr(300, 257, 6, seed=501)           # tests/test_gpu_sddmm.py's grid pattern
    return sm.SparseMatrix.from_csr(rp, ci, va, 257), rp, ci


def _sddmm_inputs(regime, N, nnz):
    reg, rng = SDDMM_REGIMES[regime], _rng(regime, 2000 + N)
    return reg.table(rng, 300 * N).reshape(300, N), reg.draw_x(rng, (257, N)), reg.draw_y0(rng, nnz)


def _sddmm(m, G, X, out0, alpha, beta, algo):
    out = to_dev(out0)
    m.sddmm(to_dev(G), to_dev(X), out, alpha, beta, algo=algo)
    return to_host(out)


@pytest.mark.parametrize("regime", list(SDDMM_REGIMES))
@pytest.mark.parametrize("N", SDDMM_N)
def test_sddmm_parity(grid_case, N, regime):
    """SM_ALGO_PARITY against the header's order restated in float32 (sddmm_ref.parity)."""
    m, rp, ci = grid_case
    G, X, out0 = _sddmm_inputs(regime, N, ci.size)
    for alpha, beta in SDDMM_REGIMES[regime].scalars:
        want = sddmm_ref.parity(rp, ci, G, X, out0, alpha, beta)
        if regime == "alpha_under":
            dots = sddmm_ref.parity(rp, ci, G, X, np.zeros(ci.size, np.float32), 1.0, 0.0)
            assert re_.is_subnormal(np.float32(alpha) * dots).mean() > 0.5 and not re_.is_subnormal(dots).any()
        assert_same_nanclass(_sddmm(m, G, X, out0, alpha, beta, "parity"), want, None,
                             f"parity N {N} {regime} alpha {alpha} beta {beta}")


@pytest.mark.parametrize("N", SDDMM_N)
def test_sddmm_auto_subnormal(grid_case, N):
    """SM_ALGO_AUTO: the PARITY kernel's bits for N <= 3; otherwise (fused multiply-adds and a
    tree) within 1e-6 * absum + (N + 2) * 2**-149 of the float64 value: one rounding of at most
    2**-150 per fused product, one for alpha * s and one for beta * out."""
    m, rp, ci = grid_case
    G, X, out0 = _sddmm_inputs("subnormal", N, ci.size)
    for alpha, beta in REGIMES["subnormal"].scalars:
        got = _sddmm(m, G, X, out0, alpha, beta, "auto")
        tag = f"auto N {N} alpha {alpha} beta {beta}"
        if N <= 3:
            assert_same_nanclass(got, _sddmm(m, G, X, out0, alpha, beta, "parity"), None, tag)
        else:
            want64, absum = sddmm_ref.exact(rp, ci, G, X, out0, alpha, beta)
            assert_sum_close(got, want64, absum, np.full(ci.size, N + 1), tag)


# ---------------------------------------------------------------------------- 5. sm_sddmm_table
@pytest.mark.parametrize("N", [1, 4, 32])
def test_sddmm_table_subnormal(sm, N):
    """The table gradient on test_gpu_table.py's 300 x 257 pattern (T = 7) in `subnormal`: both
    algorithms equal the header's reduction order restated from the GPU's own per-term dots
    (table_ref), bit for bit, and lie within R_t * 2**-24 * absum + (count_t + 2) * 2**-149 of
    the float64 value, count_t the terms that share the id (one rounding of the smallest
    subnormal per dot, one for alpha * S, one for beta * out)."""
    rp, ci = pattern(300, 257, 6)
    T, ids = 7, uniform_ids(ci.size, 7)
    reg, rng = REGIMES["subnormal"], _rng("subnormal", 3000 + N)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, reg.table(rng, T), 257)
    G, X, out0 = reg.table(rng, 300 * N).reshape(300, N), reg.draw_x(rng, (257, N)), reg.draw_y0(rng, T)
    Gd, Xd = to_dev(G), to_dev(X)
    assert re_.is_subnormal(G[sddmm_ref.term_rows(rp)] * X[ci]).mean() > 0.9
    count = np.bincount(ids, minlength=T)
    for algo in ("auto", "parity"):
        d = to_host(M.sddmm(Gd, Xd, alpha=1.0, beta=0.0, algo=algo))
        p = table_ref.chunk_partials(d, ids, T)
        for alpha, beta in reg.scalars:
            got = to_host(M.sddmm_table(Gd, Xd, out=to_dev(out0), alpha=alpha, beta=beta, algo=algo))
            tag = f"sddmm_table N {N} {algo} alpha {alpha} beta {beta}"
            assert_same_nanclass(got, table_ref.finish_partials(p, out0, alpha, beta), None, tag)
            val, absum, R = table_ref.exact_by_id(rp, ci, ids, T, G, X, out0, alpha, beta,
                                                  algo == "auto" and N >= 4 and N % 4 == 0)
            err = np.abs(got.astype(np.float64) - val)
            bound = R * 2.0 ** -24 * absum + (count + 2) * re_.ULP_MIN
            print(f"{tag}: worst ratio {float((err / bound).max()):.3g}")
            assert np.all(err <= bound), f"{tag}: worst ratio {float((err / bound).max()):.3g}"


# ---------------------------------------------------------------------------- 6. in-place updates
# fl(a * delta) subnormal: a = 1.3 * 2^-40 on delta in 2^[-105, -90] gives 2^-145 .. 2^-128, added to
# values of 2^[-140, -120] (subnormal and just normal).  fl(a * delta) overflowing: a = 1.3 * 2^28 on
# delta in 2^[95, 99] passes 2^128 for the upper half of the mantissas at e = 99, and the finite ones
# (up to 2^127.9) overflow in the sum with values of 2^[120, 127] of the same sign.  The current values
# are finite, so no NaN is generated and the bit-for-bit matrix comparisons stay meaningful.
UPDATE_RUNS = {"under": (re_.A_UNDER, (-140, -120), (-105, -90)), "over": (re_.A_OVER, (120, 127), (95, 99))}


def _update_data(run, n):
    a, cur, dlt = UPDATE_RUNS[run]
    rng = _rng("subnormal", 4000 + len(run))
    val1, delta = re_.pow2(rng, n, *cur), re_.pow2(rng, n, *dlt)
    want = axpy_reference(val1, a, delta)
    with np.errstate(over="ignore"):
        prod = np.float32(a) * delta
    if run == "under":
        assert re_.is_subnormal(prod).mean() > 0.9 and re_.is_subnormal(want).mean() > 0.2
    else:
        assert 0.02 < np.isinf(prod).mean() < 0.5 and np.isinf(want).mean() > np.isinf(prod).mean()
        assert not np.isnan(want).any()
    return a, val1, delta, want


@pytest.mark.parametrize("run", list(UPDATE_RUNS))
@pytest.mark.parametrize("layout", ["band2", "sell"])
def test_axpy_values(sm, layout, run):
    """sm_axpy_values on a band2 and a sliced-ELL case of test_gpu_update_values.py: the CSR
    values are fl(val + fl(a * delta)), and the matrix is what a fresh build from them gives."""
    if layout == "band2":
        (rp, ci), n_cols, opts = pattern(5000, 1000, 5), 1000, dict(layout="band2", band_slabs=0, band_tall=0)
    else:
        (rp, ci), n_cols, opts = pattern(5000, 1000, 5, long_row=True), 1000, dict(layout="no_bands", sell_max_len=64)
    opts = dict(opts, updatable=1)
    a, val1, delta, want = _update_data(run, ci.size)
    M = sm.SparseMatrix.from_csr(rp, ci, val1, n_cols, opts=opts)
    info = M.info()
    assert info["updatable"] == 1 and (info["has_xband"] == 4 if layout == "band2" else info["sell_slices"] > 0)
    M.axpy_values(a, to_dev(delta))
    assert_same_nanclass(M.csr()[2], want, None, f"axpy_values {layout} {run}")
    F = sm.SparseMatrix.from_csr(rp, ci, want, n_cols, opts=opts)
    assert_same_values_matrix(M, F, ValueOperands(rp.size - 1, n_cols), f"axpy_values {layout} {run}:")


@pytest.mark.parametrize("run", list(UPDATE_RUNS))
def test_axpy_table(sm, run):
    """sm_axpy_table on a cband case of test_gpu_table.py, the same two runs on the table."""
    rp, ci = pattern(5000, 1000, 5)
    ids = ids_for_update(ci.size)
    opts = dict(layout="cband", band_slabs=1, band_tall=0, table_updatable=1)
    a, t1, delta, want = _update_data(run, T_UPD)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, t1, 1000, opts=opts)
    assert M.info()["has_xband"] == 5 and M.info()["table_updatable"] == 1
    M.axpy_table(a, to_dev(delta))
    assert_same_nanclass(to_host(M.table_device()), want, None, f"axpy_table {run}: table")
    assert_same_nanclass(M.csr()[2], want[ids], None, f"axpy_table {run}: CSR values")
    F = sm.SparseMatrix.from_csr_ids(rp, ci, ids, want, 1000, opts=opts)
    table_ref.assert_same_matrix(M, F, table_ref.Operands(5000, 1000), f"axpy_table {run}:")
