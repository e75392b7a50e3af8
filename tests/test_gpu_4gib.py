"""Byte offsets of 2^32 and above: operands that span 4 GiB (part A), an x of 4 GiB and more
(part B) and term arrays of 4 GiB and more (part C).

Expected values never come from the library: oracle.csr_spmv / csr_spmm / csr_spmv_f64,
oracle.RefModel, sddmm_ref, table_ref, the golden fixture and numpy.  A product does not depend
on a leading dimension or on columns it never touches, so the oracle runs on a compact twin:
the same operands at ld = n_rhs and, in part B, the columns in use relabelled to their ranks
with x gathered to match (the same terms in the same order).

Operands live in big_operands.spread_2d parents: about 4 GiB each, never initialised but for
the live columns and 64 guard words on each side of every row.  A test holds at most two of
them and releases them before it returns.

Leading dimensions (big_operands): ld_below / ld_at sit on the two sides of the library's
switches (rows * ld * 4 < 0xFFFFFFF0); at ld_at every row still starts below 2^32 bytes, so
ld_past, where the last row starts at 2^32 bytes or more, is the placement at which a 32-bit
byte offset would wrap.
"""
import functools
import gc
import time

import numpy as np
import pytest

import big_operands as bo
import oracle
import sddmm_ref
import table_ref
from gpu_util import assert_terms_close, bits, slab_order_spmv, to_dev, to_host, torch_dev
from layout_specs import _same

pytestmark = pytest.mark.gpu

SCALARS = [(1.3, 0.7), (-2.0, 0.0)]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


@pytest.fixture(autouse=True)
def _release_device_memory():
    """Free the big buffers after every test; a device error ends the session (nothing more
    is started on a GPU that has faulted)."""
    yield
    torch = torch_dev()
    gc.collect()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a test of test_gpu_4gib.py: {e}", returncode=3)
    torch.cuda.empty_cache()


def _live(view) -> np.ndarray:
    """Host copy of a spread view's live elements only."""
    torch = torch_dev()
    torch.cuda.synchronize()
    return view.contiguous().cpu().numpy()


def _unchanged(view, parent, mat, ld, off, what):
    rows, n = mat.shape
    assert np.array_equal(bits(_live(view)), bits(mat)), f"{what} was written"
    bo.assert_spread_guards(parent, rows, n, ld, off)


# =========================================================================== part A
ROWS_A, COLS_A, LD_X, LD_Y, SDDMM_PLACES = bo.ROWS_A, bo.COLS_A, bo.LD_X, bo.LD_Y, bo.SDDMM_PLACES
_small = functools.lru_cache(maxsize=None)(bo.small_csr)


def _small_matrix(sm):
    rp, ci, va, _, _ = _small()
    return sm.SparseMatrix.from_csr(rp, ci, va, COLS_A, opts=dict(layout="no_bands"))


@functools.lru_cache(maxsize=None)
def _panel(n_rhs):
    X, Y0, _ = bo.spmm_panel(n_rhs)
    return X, Y0


@functools.lru_cache(maxsize=None)
def _spmm_want(n_rhs, alpha, beta):
    rp, ci, va, _, _ = _small()
    X, Y0 = _panel(n_rhs)
    return oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)


@functools.lru_cache(maxsize=None)
def _spmm_absum(n_rhs, alpha, beta):
    rp, ci, va, _, _ = _small()
    X, Y0 = _panel(n_rhs)
    ab = np.empty(Y0.shape, np.float64)
    for j in range(n_rhs):
        _, ab[:, j] = oracle.csr_spmv_f64(rp.astype(np.int64), ci, va, np.ascontiguousarray(X[:, j]),
                                          np.ascontiguousarray(Y0[:, j]), alpha, beta)
    return ab


def _spmm_spread(sm, n_rhs, ldx, ldy, x_off, algos, exact=True):
    """Every algo and (alpha, beta) with X at (ldx, x_off) and Y at ldy: Y bit-identical to
    oracle.csr_spmm (exact) or within 1e-6 * sum|terms|; guards of both intact, X unchanged."""
    torch = torch_dev()
    M = _small_matrix(sm)
    X, Y0 = _panel(n_rhs)
    Xv, Xp = bo.spread_2d(X, ldx, x_off)
    Yv, Yp = bo.spread_2d(Y0, ldy)
    y0_dev = to_dev(Y0)
    # Where a 32-bit byte offset of X's last row would wrap to: defined data that differs from
    # that row in every column (test_big_operands_cpu.py), not whatever the allocation held.
    decoy = bo.spmm_panel(n_rhs)[2] if bo.decoy_is_clear(COLS_A, n_rhs, ldx) else None
    Dv = bo.write_decoy(Xp, COLS_A, n_rhs, ldx, decoy, x_off) if decoy is not None else None
    try:
        for algo in algos:
            for alpha, beta in SCALARS:
                Yv.copy_(y0_dev)
                M.spmm(Xv, Yv, alpha, beta, algo=algo)
                got = _live(Yv)
                tag = f"{algo} N {n_rhs} ld ({ldx}, {ldy}) x_off {x_off} alpha {alpha} beta {beta}"
                if exact:
                    _same(got, _spmm_want(n_rhs, alpha, beta), None, tag)
                else:
                    assert_terms_close(got, _spmm_want(n_rhs, alpha, beta), _spmm_absum(n_rhs, alpha, beta))
                bo.assert_spread_guards(Yp, ROWS_A, n_rhs, ldy)
        _unchanged(Xv, Xp, X, ldx, x_off, "X")
        if Dv is not None:
            assert np.array_equal(bits(to_host(Dv)), bits(decoy)), "the decoy was written"
    finally:
        M.Destroy()
        del Xv, Xp, Yv, Yp, Dv
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- A1
@pytest.mark.parametrize("place", ["below", "at", "past"])
@pytest.mark.parametrize("n_rhs", [4, 32, 64, 128])
def test_spmm_rowpanel_across_the_x_switch(sm, n_rhs, place):
    """sm_spmm "auto" and "vector" with 16-byte aligned operands and ld % 4 == 0 (vec_ok).
    below: X spans just under 0xFFFFFFF0 bytes -- "auto" runs the gather-pipelined kernel
    (spmm_rowpanel2_kernel, N <= 64).  at: X spans 2^32 bytes -- "auto" must drop it for
    spmm_rowpanel_kernel; every X row still starts below 2^32, so only the switch is tested.
    past: X's row 63 and Y's row 69 start at or past 2^32 bytes -- the pipelined kernel's 32-bit
    offset 4 * (63 ldx + 4g) would wrap to float 188 + 4g of X's storage, in the unused stretch
    between rows 0 and 1.  For N <= 64 a decoy row is written there, and X's row 63, in nearly
    every matrix row, is non-zero and differs from it in every column, so the wrapped read gives
    other bits whatever the allocation held (shown on the CPU in test_big_operands_cpu.py).
    "vector" and N = 128 (G = 32) run spmm_rowpanel_kernel at every placement; at N = 128 the
    decoy would overlap row 0's guard and is left out.  Y at ld_at(70) (ld_past(70) in the last
    case).  Bit-identical to oracle.csr_spmm; X's bits unchanged; row guards of both intact."""
    _spmm_spread(sm, n_rhs, LD_X[place], LD_Y["past" if place == "past" else "at"], 0, ("auto", "vector"))


# ---------------------------------------------------------------------------- A2
@pytest.mark.parametrize("n_rhs,x_off,algo,place", [(5, 0, "auto", "at"), (32, 1, "auto", "at"),
                                                    (32, 0, "parity", "at"), (5, 0, "auto", "past"),
                                                    (32, 0, "parity", "past")])
def test_spmm_generic_kernel_past_4gib(sm, n_rhs, x_off, algo, place):
    """spmm_generic_kernel (one thread per output, plain 64-bit pointers): N = 5 (not a multiple
    of 4), N = 32 with X one float off 16-byte alignment, and algo "parity", with both operands
    at ld_at and with both last rows past 2^32 bytes.  Bit-identical to oracle.csr_spmm."""
    _spmm_spread(sm, n_rhs, LD_X[place], LD_Y[place], x_off, (algo,))


# ---------------------------------------------------------------------------- A3
def test_spmm_mfma_takes_x_below_the_limit(sm):
    """SM_ALGO_MFMA, N = 32, X at ld_below(64): the last placement it accepts (its byte
    offsets into X are 32-bit).  Within 1e-6 * sum|terms| of the oracle."""
    _spmm_spread(sm, 32, LD_X["below"], LD_Y["at"], 0, ("mfma",), exact=False)


@pytest.mark.parametrize("place", ["at", "past"])
def test_spmm_mfma_refuses_x_at_the_limit(sm, place):
    """X at ld_at(64) and beyond: SM_ERR_NOT_SUPPORTED (status 4) from sm_spmm's own check --
    launch_spmm_mfma's copy of it would give SM_ERR_HIP -- and Y's live part and guards
    bit-unchanged."""
    torch = torch_dev()
    M = _small_matrix(sm)
    X, Y0 = _panel(32)
    ldx, ldy = LD_X[place], LD_Y["at"]
    Xv, Xp = bo.spread_2d(X, ldx)
    Yv, Yp = bo.spread_2d(Y0, ldy)
    try:
        with pytest.raises(sm.SparseMatrixError) as ei:
            M.spmm(Xv, Yv, 1.3, 0.7, algo="mfma")
        assert ei.value.status == 4
        _unchanged(Yv, Yp, Y0, ldy, 0, "Y")
    finally:
        M.Destroy()
        del Xv, Xp, Yv, Yp
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- A4 / A5
def _sddmm_inputs(n_rhs):
    rp, ci, _, _, _ = _small()
    G, X, out0 = sddmm_ref.grid_inputs(ROWS_A, COLS_A, ci.size, n_rhs, seed=700)
    return G, X, out0


def _sddmm_place(G, X, place):
    ldg, ldx = SDDMM_PLACES[place]
    Gv, Gp = bo.spread_2d(G, ldg) if ldg else (to_dev(G), None)
    Xv, Xp = bo.spread_2d(X, ldx) if ldx else (to_dev(X), None)
    return Gv, Gp, Xv, Xp


def _sddmm_unchanged(G, X, place, Gv, Gp, Xv, Xp):
    ldg, ldx = SDDMM_PLACES[place]
    if ldg:
        _unchanged(Gv, Gp, G, ldg, 0, "G")
    if ldx:
        _unchanged(Xv, Xp, X, ldx, 0, "X")


@pytest.mark.parametrize("place", list(SDDMM_PLACES))
@pytest.mark.parametrize("n_rhs", [4, 32, 5])
def test_sddmm_across_the_operand_switch(sm, n_rhs, place):
    """sm_sddmm with G (70 rows) or X (64 rows) at ld_at / ld_past and the other operand compact,
    and with both at ld_below.  "parity" is always bit-identical to sddmm_ref.parity.  "auto"
    with an operand at or past the limit must drop the vector kernel (sddmm_panel_ok) and give
    PARITY's bits -- at N = 32 the vector kernel's fused order gives other bits, and at ld_past
    its 32-bit descriptor size and offsets would wrap; with both operands below the limit it
    runs the vector kernel (N = 4, 32): within the header's bound of sddmm_ref.exact and
    bit-identical on a second call.  N = 5 is the one-lane-per-term kernel everywhere."""
    torch = torch_dev()
    rp, ci, _, _, _ = _small()
    M = _small_matrix(sm)
    G, X, out0 = _sddmm_inputs(n_rhs)
    Gv, Gp, Xv, Xp = _sddmm_place(G, X, place)
    vector = place == "both_below" and n_rhs % 4 == 0
    try:
        for alpha, beta in SCALARS:
            want = sddmm_ref.parity(rp, ci, G, X, out0, alpha, beta)
            tag = f"N {n_rhs} {place} alpha {alpha} beta {beta}"
            got = to_host(M.sddmm(Gv, Xv, to_dev(out0), alpha, beta, algo="parity"))
            _same(got, want, None, "parity " + tag)
            got = to_host(M.sddmm(Gv, Xv, to_dev(out0), alpha, beta, algo="auto"))
            if vector:
                val, absum = sddmm_ref.exact(rp, ci, G, X, out0, alpha, beta)
                assert_terms_close(got, val, absum)
                again = to_host(M.sddmm(Gv, Xv, to_dev(out0), alpha, beta, algo="auto"))
                _same(again, got, None, "auto, second call " + tag)
            else:
                _same(got, want, None, "auto vs PARITY " + tag)
        _sddmm_unchanged(G, X, place, Gv, Gp, Xv, Xp)
    finally:
        M.Destroy()
        del Gv, Gp, Xv, Xp
        torch.cuda.empty_cache()


@pytest.mark.parametrize("place", list(SDDMM_PLACES))
@pytest.mark.parametrize("n_rhs", [4, 32, 5])
def test_sddmm_table_across_the_operand_switch(sm, n_rhs, place):
    """sm_sddmm_table on from_csr_ids of the same pattern (T = 7, seeded ids), the placements of
    the sddmm test.  Expected values as tests/test_gpu_table.py forms them: the header's steps
    2-4 (table_ref.chunk_partials / finish_partials) over the per-term dots.  The dots are
    sddmm_ref.parity's for "parity" and for "auto" wherever the PARITY order must run (an operand
    at or past the limit, N = 5): bit for bit.  With both operands below the limit "auto" runs
    the vector kernel (N = 4, 32): bit for bit over sm_sddmm's own dots at the same placement,
    and within the header's R_t * 2^-24 bound of table_ref.exact_by_id."""
    torch = torch_dev()
    rp, ci, _, ids, table7 = _small()
    T = table7.size
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table7, COLS_A, opts=dict(layout="no_bands"))
    G, X, _ = _sddmm_inputs(n_rhs)
    out0 = np.random.default_rng(77).uniform(-1, 1, T).astype(np.float32)
    Gv, Gp, Xv, Xp = _sddmm_place(G, X, place)
    vector = place == "both_below" and n_rhs % 4 == 0
    try:
        # s itself: -0.0 + 1 * s
        d_par = sddmm_ref.parity(rp, ci, G, X, np.full(ci.size, -0.0, np.float32), 1.0, 1.0)
        p_par = table_ref.chunk_partials(d_par, ids, T)
        p_auto = p_par
        if vector:
            p_auto = table_ref.chunk_partials(to_host(M.sddmm(Gv, Xv, alpha=1.0, beta=0.0, algo="auto")), ids, T)
        for alpha, beta in SCALARS:
            tag = f"N {n_rhs} {place} alpha {alpha} beta {beta}"
            for algo, p in (("parity", p_par), ("auto", p_auto)):
                got = to_host(M.sddmm_table(Gv, Xv, out=to_dev(out0), alpha=alpha, beta=beta, algo=algo))
                _same(got, table_ref.finish_partials(p, out0, alpha, beta), None, f"{algo} {tag}")
                val, absum, R = table_ref.exact_by_id(rp, ci, ids, T, G, X, out0, alpha, beta,
                                                      vector and algo == "auto")
                err = np.abs(got.astype(np.float64) - val)
                assert np.all(err <= R * U * absum + 1e-37), f"{algo} {tag}: {float((err / (R * U * absum + 1e-37)).max()):.3g}"
        _sddmm_unchanged(G, X, place, Gv, Gp, Xv, Xp)
    finally:
        M.Destroy()
        del Gv, Gp, Xv, Xp
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- A6
@pytest.mark.parametrize("algo", ["auto", "exact", "parity", "native"])
@pytest.mark.parametrize("m", [2, 3])
def test_addmatmat_rows_far_apart(sm, m, algo):
    """AddMatMat on device pointers with lda = 2^29 + 3, ldc = 2^29 + 1 on the dense-index matrix
    of test_gpu_operands (300 x 257): row 1 of A and C starts past 2 GiB, row 2 past 4 GiB; the
    odd leading dimensions leave rows 1 and 2 only 4-byte aligned.  m = 2 takes the per-row SpMV
    route (x = a + lda, y = c + ldc), m = 3 the transposes into the workspace and the row
    panel; "parity" the in-place generic kernel, "native" the reference stream's kernel.
    Bit-identical to RefModel.add_mat_mat run with lda = k, ldc = n on the same rows."""
    from test_gpu_operands import _dense_index
    torch = torch_dev()
    dm, rows, cols, table, T = _dense_index()
    M = sm.SparseMatrix(dm, rows, cols, cols, table, T, sm.SblasNoTrans)
    ref = oracle.RefModel(dm, rows, cols, cols, table, T, trans=False)
    k, n = M.NumRows(), M.NumCols()
    assert (k, n) == (300, 257)
    lda, ldc = (1 << 29) + 3, (1 << 29) + 1
    rng = np.random.default_rng(40 + m)
    A = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    C0[:, ::5] = -0.0
    Av, Ap = bo.spread_2d(A, lda)
    Cv, Cp = bo.spread_2d(C0, ldc)
    c0_dev = to_dev(C0)
    a_flat, c_flat = bo.flat(Av, m, k, lda), bo.flat(Cv, m, n, ldc)
    try:
        for alpha, beta in SCALARS:
            want = ref.add_mat_mat(A.reshape(-1), m, k, C0.reshape(-1), n, alpha, beta)
            Cv.copy_(c0_dev)
            M.AddMatMat(a_flat, m, lda, c_flat, ldc, alpha, beta, algo=algo)
            _same(_live(Cv), want.reshape(m, n), None, f"{algo} m {m} alpha {alpha} beta {beta}")
            bo.assert_spread_guards(Cp, m, n, ldc)
        _unchanged(Av, Ap, A, lda, 0, "A")
    finally:
        M.Destroy()
        del Av, Ap, Cv, Cp, a_flat, c_flat
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- A7
def test_beta_and_transpose_kernels_rows_far_apart(sm):
    """sblas_beta_operation_kernel on a 3 x 5 matrix at ld = 2^29 + 1 and sblas_trans_kernel from
    it into a 5 x 3 matrix at ldsa = 2^28 + 3 (row 2 of the input and row 4 of the output start
    past 4 GiB; int32 leading dimensions whose products with the row index are formed in 64
    bits).  Bit for bit: oracle.beta_scale and oracle.transpose on the compact matrices."""
    torch = torch_dev()
    from sparsematrix_amd.sparse_matrix import sblas_beta_operation_kernel, sblas_trans_kernel
    m, n, ld, ldsa = 3, 5, (1 << 29) + 1, (1 << 28) + 3
    rng = np.random.default_rng(35)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    C0[1, 2] = np.nan
    C0[2, 4] = -0.0
    Cv, Cp = bo.spread_2d(C0, ld)
    S0 = rng.uniform(-1, 1, (n, m)).astype(np.float32)
    Sv, Sp = bo.spread_2d(S0, ldsa)
    try:
        want_t = oracle.transpose(C0, m, n, n, m, n * m).reshape(n, m)
        assert np.array_equal(bits(want_t), bits(C0.T))
        sblas_trans_kernel(bo.flat(Cv, m, n, ld), m, n, ld, bo.flat(Sv, n, m, ldsa), ldsa)
        _same(_live(Sv), want_t, None, "transpose")
        bo.assert_spread_guards(Sp, n, m, ldsa)
        _unchanged(Cv, Cp, C0, ld, 0, "the transpose's input")
        cur = C0
        for beta in (1.0, 0.7, 0.0):
            cur = oracle.beta_scale(cur, m, n, n, beta).reshape(m, n)
            sblas_beta_operation_kernel(bo.flat(Cv, m, n, ld), m, n, ld, beta)
            _same(_live(Cv), cur, None, f"beta {beta}")
            bo.assert_spread_guards(Cp, m, n, ld)
        assert np.isnan(cur[1, 2])          # beta = 0 multiplies: the NaN stays
    finally:
        del Cv, Cp, Sv, Sp
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------- A8
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_panel_kernels_rows_far_apart(sm, variant):
    """sm_panel_kernel on the golden case of test_panel_kernels_vs_golden (m 13, n 256, k 300)
    with A and C spread at ld_past(rows): the last row in use starts at or past 2^30 floats and
    each allocation stays under 6 GiB (variants 0, 1: 13 rows each; the transposed variants 2, 3:
    A^T 300 rows, C^T 256 rows, 13 live columns).  Bit-identical to the fixture's out_v*."""
    from golden_util import load_kernels
    from sparsematrix_amd import _lib
    torch = torch_dev()
    g = load_kernels()
    L = _lib.load()
    m, n, k = int(g["m"]), int(g["n"]), int(g["k"])
    if variant < 2:
        A = g["a"].reshape(m, int(g["lda"]))[:, :k]
        C0 = g["c"].reshape(m, int(g["ldc"]))[:, :n]
        want = g[f"out_v{variant}"].reshape(m, int(g["ldc"]))[:, :n]
    else:
        ldt = int(g["ldt"])
        A = g["aT"].reshape(k, ldt)[:, :m]
        C0 = g["cT"].reshape(n, ldt)[:, :m]
        want = g[f"out_v{variant}"].reshape(n, ldt)[:, :m]
    lda, ldc = bo.ld_past(A.shape[0]), bo.ld_past(C0.shape[0])
    assert (A.shape[0] - 1) * lda >= 1 << 30 and A.shape[0] * lda * 4 < 6 << 30
    assert (C0.shape[0] - 1) * ldc >= 1 << 30 and C0.shape[0] * ldc * 4 < 6 << 30
    pos, val, tab = to_dev(g["pos"]), to_dev(g["val"]), to_dev(g["table"])
    Av, Ap = bo.spread_2d(A, lda)
    Cv, Cp = bo.spread_2d(C0, ldc)
    try:
        st = L.sm_panel_kernel(variant, m, n, k, Av.data_ptr(), lda, Cv.data_ptr(), ldc, float(g["alpha"]),
                               pos.data_ptr(), val.data_ptr(), int(g["pos"].size), tab.data_ptr(),
                               int(g["table_size"]), None)
        assert st == 0, L.sm_last_error()
        _same(_live(Cv), want, None, f"variant {variant}")
        bo.assert_spread_guards(Cp, C0.shape[0], C0.shape[1], ldc)
        _unchanged(Av, Ap, np.ascontiguousarray(A), lda, 0, "A")
    finally:
        del Av, Ap, Cv, Cp
        torch.cuda.empty_cache()


# =========================================================================== part B
ROWS_B = 300
WIDTHS_B = {"2^30-8": (1 << 30) - 8, "2^30+8": (1 << 30) + 8}
BUILDS_B = {
    "auto": {}, "no_bands": dict(layout="no_bands"), "no_bands_ccsell": dict(layout="no_bands", ccsell=1),
    "no_bands_sell": dict(layout="no_bands", ccsell=0),        # the sorted sliced ELL instead
    "gcb": dict(layout="gcb"), "band2": dict(layout="band2"), "cband": dict(layout="cband"),
}
BAND_CODE_B = {"gcb": 6, "band2": 4, "cband": 5}


@functools.lru_cache(maxsize=None)
def _wide(n_cols):
    """300 x n_cols CSR: every 50th row empty; 8 ascending distinct columns per row, one below
    2^16 and one within 8 of each of 2^28, 2^29, 2^30 - 1 and n_cols - 1; row 123 of 300 and row
    234 of 2100 distinct columns; values from a 200-entry table.  Returns the CSR, its compact
    twin (columns relabelled to their ranks among the columns in use), the columns in use, their
    seeded x values and y0 (with -0.0 in places)."""
    rng = np.random.default_rng(n_cols % 1000 + 30)
    table = rng.uniform(-1, 1, 200).astype(np.float32)
    rows = []
    for r in range(ROWS_B):
        if r % 50 == 0:
            rows.append(np.zeros(0, np.int64))
            continue
        if r in (123, 234):
            k = 300 if r == 123 else 2100
            near_end = n_cols - 1 - rng.choice(64, 4, replace=False)
            c = np.unique(np.concatenate([rng.integers(0, n_cols, k - 4), near_end]))
            while c.size < k:
                c = np.unique(np.concatenate([c, rng.integers(0, n_cols, k - c.size)]))
            rows.append(c)
            continue
        c = [int(rng.integers(0, 1 << 16))]
        for p in (1 << 28, 1 << 29, (1 << 30) - 1, n_cols - 1):
            c.append(min(n_cols - 1, p - 8 + int(rng.integers(0, 17))))
        c = np.unique(np.array(c, np.int64))
        while c.size < 8:
            c = np.unique(np.concatenate([c, rng.integers(0, n_cols, 8 - c.size)]))
        rows.append(c)
    lens = np.array([c.size for c in rows], np.int64)
    assert set(lens.tolist()) == {0, 8, 300, 2100}
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci64 = np.concatenate(rows)
    assert ci64.min() >= 0 and ci64.max() == n_cols - 1
    ci = ci64.astype(np.int32)
    va = np.ascontiguousarray(table[rng.integers(0, table.size, ci.size)], np.float32)
    used = np.unique(ci64)
    twin_ci = np.searchsorted(used, ci64).astype(np.int32)
    x_used = rng.uniform(-1, 1, used.size).astype(np.float32)
    y0 = rng.uniform(-1, 1, ROWS_B).astype(np.float32)
    y0[lens == 0] = -0.0
    y0[7::31] = -0.0
    return rp, ci, va, twin_ci, used, x_used, y0, lens


@functools.lru_cache(maxsize=None)
def _wide_ref(n_cols, alpha, beta):
    rp, _, va, twin_ci, _, x_used, y0, _ = _wide(n_cols)
    want = oracle.csr_spmv(rp, twin_ci, va, x_used, y0, alpha, beta)
    _, absum = oracle.csr_spmv_f64(rp, twin_ci, va, x_used, y0, alpha, beta)
    return want, absum


def _wide_slab_ref(info, n_cols, alpha, beta):
    """gpu_util.slab_order_for on the compact twin: every term's slab from its real column."""
    rp, ci, va, twin_ci, _, x_used, y0, _ = _wide(n_cols)
    s0, sc = info["xband_slab0_cols"], info["xband_slab_cols"]
    c = ci.astype(np.int64)
    term_slab = np.where(c < s0, 0, 1 + (c - s0) // sc)
    return slab_order_spmv(rp, twin_ci, va, x_used, y0, alpha, beta, sc, s0,
                           beta_last=bool(info["xband_beta_last"]), term_slab=term_slab,
                           n_slabs=info["xband_slabs"])


# device arrays only for the forced kinds: the other builds run no device builder of their own here
CASES_B = [(w, b, "host") for w in WIDTHS_B for b in BUILDS_B] + \
          [(w, b, "device") for w in WIDTHS_B for b in BAND_CODE_B]


@pytest.mark.parametrize("width,build,source", CASES_B)
def test_spmv_x_of_4gib(sm, width, build, source):
    """SpMV with an x of 2^30 -+ 8 elements (4 GiB -+ 32 bytes, one buffer, zeros but for the
    columns in use) on whatever each build gives: AUTO, no_bands, no_bands with and without ccsell, and forced
    gcb / band2 / cband, from host arrays and (the forced kinds, whose device builders have
    their own size checks) from device arrays.  At 2^30 + 8 columns no band layout may be built
    (band2, cband and gcb decline from 2^30 columns: their byte offsets into x are 32-bit).
    Every algorithm of table_ref.SPMV_ALGOS against oracle.csr_spmv on the compact twin:
    bit-identical for parity and exact, for a one-slab band layout (xband, auto), for the
    column-chunked ELL, for sliced-ELL rows up to 2048 terms and stream rows up to
    SM_SERIAL_ROW_MAX = 64; gpu_util's slab order with several slabs; within
    1e-6 * sum|terms| always."""
    torch = torch_dev()
    n_cols = WIDTHS_B[width]
    rp, ci, va, _, used, x_used, y0, lens = _wide(n_cols)
    if source == "device":
        M = sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), n_cols, opts=BUILDS_B[build])
    else:
        M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols, opts=BUILDS_B[build])
    info = M.info()
    note = f"{width} {build} {source}: {info}"
    x = torch.zeros(n_cols, dtype=torch.float32, device="cuda")
    try:
        assert info["n_cols"] == n_cols and info["nnz"] == ci.size, note
        if n_cols >= 1 << 30:
            assert info["has_xband"] == 0, note
        if info["has_xband"] and build in BAND_CODE_B:
            assert info["has_xband"] == BAND_CODE_B[build], note
        x[to_dev(used)] = to_dev(x_used)
        band, slabs = info["has_xband"] > 0, info["xband_slabs"]
        every, none = np.ones(ROWS_B, bool), np.zeros(ROWS_B, bool)
        if band:
            chain = every if slabs == 1 else None           # None: the slab order
            sell = lens <= 64                               # no sliced ELL beside bands: the stream kernel
        elif info["ccsell_chunks"] > 0:
            chain = sell = every
        elif info["sell_slices"] > 0:
            chain = sell = lens <= 2048
        else:
            chain = sell = lens <= 64
        masks = {"parity": every, "exact": every, "stream": lens <= 64, "vector": none, "merge": none,
                 "sell": sell, "xband": chain, "auto": chain}
        for alpha, beta in SCALARS:
            want, absum = _wide_ref(n_cols, alpha, beta)
            for algo in table_ref.SPMV_ALGOS:
                y = to_dev(y0)
                M.spmv(x, y, alpha, beta, algo=algo)
                got = to_host(y)
                tag = f"{algo} alpha {alpha} beta {beta} on {note}"
                assert_terms_close(got, want, absum)
                if masks[algo] is None:
                    _same(got, _wide_slab_ref(info, n_cols, alpha, beta), None, tag + " vs slab order")
                else:
                    _same(got, want, masks[algo], tag)
        used_dev = to_dev(used)
        assert np.array_equal(bits(to_host(x[used_dev])), bits(x_used)), "x was written at a column in use"
        assert int((x != 0).sum()) == int((x_used != 0).sum()), "x was written at a column not in use"
    finally:
        M.Destroy()
        del x
        torch.cuda.empty_cache()


# =========================================================================== part C
@pytest.mark.slow
def test_term_arrays_past_4gib(sm):
    """One matrix of 1.25 * 2^30 terms (big_operands: 2^20 rows of 1280 terms, 4096 columns; col
    and val are 5 GiB each), generated on the device and built with layout no_bands, sell 0,
    relabel 0, ccsell 0, so nothing goes through the host.  Checked on 280 sampled rows (the
    first 8, the 8 around the row that straddles term 2^30, 256 seeded rows above it, the last
    8) whose terms the host regenerates from the closed form; at least 264 of them lie wholly
    at or above term 2^30, and there (col, val) at term t differs from (col, val) at t - 2^30
    in every position (asserted here, before any product), so a 32-bit byte offset 4 t that
    wraps cannot go unseen.
      spmm auto / vector, N = 4, 32: bit-identical to oracle.csr_spmm ("auto" must leave the
        gather-pipelined kernel: its offsets into col / val are 32-bit);
      AddMatMat m = 3, auto: bit-identical on the sampled output columns;
      spmv parity bit-identical; stream, vector, merge, auto within 1e-6 * sum|terms| (1280 terms
        exceed SM_SERIAL_ROW_MAX); each bit-identical on a second call;
      sddmm N = 4: parity bit-identical to sddmm_ref.parity, auto within the header's bound;
      mfma N = 32: SM_ERR_NOT_SUPPORTED (status 4), Y unchanged.
    Measured once on an MI355X, inside a run of the whole suite (the times are pytest
    --durations' "call" figures, the memory is this test's own print): 0.75 s for creation and
    all products, 20.6 GiB of device memory at the peak (the caller's arrays beside the matrix's
    copy; 15 GiB later, with sddmm's out).  test_config5_rank0_slice_full_size_auto_vs_oracle
    was not among that run's 40 slowest calls, the last of which took 0.69 s, so it took less:
    hence the slow mark."""
    torch = torch_dev()
    t_start = time.perf_counter()
    free0 = torch.cuda.mem_get_info()[0]
    peak = [0]

    def note_memory():
        torch.cuda.synchronize()
        peak[0] = max(peak[0], free0 - torch.cuda.mem_get_info()[0])
    table = bo.big_table()
    rows = bo.big_sample_rows()
    above = bo.big_sampling_conditions(rows, table)
    assert above.size >= 264
    sub_rp, sub_ci, sub_va = bo.big_sub_csr(rows, table)
    rows_t = to_dev(rows)
    n, k, nnz = bo.BIG_ROWS, bo.BIG_COLS, bo.BIG_NNZ

    rp, col, val = bo.big_csr_device(table)
    M = sm.SparseMatrix.from_csr(rp, col, val, k, opts=dict(layout="no_bands", sell=0, relabel=0, ccsell=0))
    note_memory()        # the caller's arrays and the matrix's copy
    del rp, col, val
    torch.cuda.empty_cache()
    try:
        info = M.info()
        assert (info["n_rows"], info["n_cols"], info["nnz"]) == (n, k, nnz), info
        assert info["has_xband"] == 0 and info["sell_slices"] == 0 and info["ccsell_chunks"] == 0, info
        gen = torch.Generator(device="cuda").manual_seed(1280)
        rng = np.random.default_rng(1281)

        # ---- spmm
        for n_rhs, (alpha, beta) in ((4, SCALARS[0]), (32, SCALARS[1])):
            X = rng.uniform(-1, 1, (k, n_rhs)).astype(np.float32)
            Xd = to_dev(X)
            Y0 = torch.rand((n, n_rhs), device="cuda", generator=gen) * 2 - 1
            want = oracle.csr_spmm(sub_rp, sub_ci, sub_va, X, to_host(Y0[rows_t]), alpha, beta)
            for algo in ("auto", "vector"):
                Y = Y0.clone()
                M.spmm(Xd, Y, alpha, beta, algo=algo)
                _same(to_host(Y[rows_t]), want, None, f"spmm {algo} N {n_rhs}: sampled rows {rows[:3]}..")
                del Y
            if n_rhs == 32:
                Y = Y0.clone()
                with pytest.raises(sm.SparseMatrixError) as ei:
                    M.spmm(Xd, Y, alpha, beta, algo="mfma")
                assert ei.value.status == 4
                torch.cuda.synchronize()
                assert torch.equal(Y.view(torch.int32), Y0.view(torch.int32)), "mfma refused but wrote Y"
                del Y
            del Y0, Xd

        # ---- AddMatMat: C (3 x n) = alpha A (3 x k) S + beta C, S = B^T
        assert (M.NumRows(), M.NumCols()) == (k, n)
        m = 3
        alpha, beta = SCALARS[0]
        A = rng.uniform(-1, 1, (m, k)).astype(np.float32)
        C0 = torch.rand((m, n), device="cuda", generator=gen) * 2 - 1
        C, Ad = C0.clone(), to_dev(A)
        M.AddMatMat(Ad.reshape(-1), m, k, C.reshape(-1), n, alpha, beta, algo="auto")
        want = oracle.csr_spmm(sub_rp, sub_ci, sub_va, np.ascontiguousarray(A.T),
                               np.ascontiguousarray(to_host(C0[:, rows_t]).T), alpha, beta)
        _same(np.ascontiguousarray(to_host(C[:, rows_t]).T), want, None, "AddMatMat m 3 auto")
        del C, C0, Ad

        # ---- spmv
        x = rng.uniform(-1, 1, k).astype(np.float32)
        xd = to_dev(x)
        y0 = torch.rand(n, device="cuda", generator=gen) * 2 - 1
        y0h = to_host(y0[rows_t])
        for alpha, beta in SCALARS:
            want = oracle.csr_spmv(sub_rp, sub_ci, sub_va, x, y0h, alpha, beta)
            _, absum = oracle.csr_spmv_f64(sub_rp, sub_ci, sub_va, x, y0h, alpha, beta)
            for algo in ("parity", "stream", "vector", "merge", "auto"):
                y, y2 = y0.clone(), y0.clone()
                M.spmv(xd, y, alpha, beta, algo=algo)
                M.spmv(xd, y2, alpha, beta, algo=algo)
                got = to_host(y[rows_t])
                assert_terms_close(got, want, absum)
                if algo == "parity":
                    _same(got, want, None, f"spmv parity alpha {alpha} beta {beta}")
                assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), f"spmv {algo}: two calls differ"
                del y, y2
        del y0, xd

        # ---- sddmm: out has nnz floats; the sampled rows' terms are rows of out.view(n, 1280)
        n_rhs, (alpha, beta) = 4, (1.3, 0.0)
        X = rng.uniform(-1, 1, (k, n_rhs)).astype(np.float32)
        Xd = to_dev(X)
        G = torch.rand((n, n_rhs), device="cuda", generator=gen) * 2 - 1
        Gs = to_host(G[rows_t])
        zeros = np.zeros(sub_ci.size, np.float32)
        out = torch.zeros(nnz, dtype=torch.float32, device="cuda")
        for algo in ("parity", "auto"):
            out.zero_()
            M.sddmm(G, Xd, out, alpha, beta, algo=algo)
            note_memory()    # the matrix and out
            got = to_host(out.view(n, bo.BIG_ROW_TERMS)[rows_t]).reshape(-1)
            if algo == "parity":
                _same(got, sddmm_ref.parity(sub_rp, sub_ci, Gs, X, zeros, alpha, beta), None, "sddmm parity")
            else:
                val64, absum = sddmm_ref.exact(sub_rp, sub_ci, Gs, X, zeros, alpha, beta)
                assert_terms_close(got, val64, absum)
        del out, G, Xd
    finally:
        M.Destroy()
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"\nterm arrays past 4 GiB: {time.perf_counter() - t_start:.2f} s wall, "
          f"{peak[0] / 2 ** 30:.1f} GiB of device memory at the peak")
