"""Table matrices on the GPU (sm_create_from_csr_ids): the gradient of the table (sm_sddmm_table)
and in-place table updates (sm_set_table, sm_axpy_table, sm_build_opts.table_updatable).

Gradient: for every case d = M.sddmm(G, X, alpha=1, beta=0) comes from the GPU with the same
`algo`, and sddmm_table must equal the numpy restatement of the header's reduction order fed with
that d, bit for bit -- the fused kernel forms the same dots and adds them in the stated order.
Accuracy: |out - exact64| <= R_t * 2^-24 * sum|.| per id, R_t the header's rounding count.
Updates: M built from table1 and updated is what a fresh build from table2 is, bit for bit (the
scheme of test_gpu_update_values.py).
"""
import numpy as np
import pytest

import table_ref
from gpu_util import (assert_guards, assert_guards_2d, bits, placed, placed_2d, to_dev, to_host, torch_dev,
                      uniform_csr)
from sddmm_ref import GRID_AB, grid_inputs
from table_ref import Operands, assert_same_matrix, assert_same_products, axpy_reference, same_bits

pytestmark = pytest.mark.gpu

INVALID, NOT_SUPPORTED, INVALID_MATRIX = 1, 4, 6
AXPY_A = -0.37
U = 2.0 ** -24


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def pattern(n_rows, n_cols, per_row, seed=7, long_row=False):
    rp, ci, _ = uniform_csr(n_rows, n_cols, min(per_row, n_cols), seed)
    if long_row:   # row n_rows // 2 holds every column
        r = n_rows // 2
        a, b = int(rp[r]), int(rp[r + 1])
        ci = np.concatenate([ci[:a], np.arange(n_cols, dtype=np.int32), ci[b:]])
        rp = rp.astype(np.int64)
        rp[r + 1:] += n_cols - (b - a)
        rp = rp.astype(np.int32)
    return rp, ci


def make_table(T, seed=21):
    return np.random.default_rng(seed).uniform(-1, 1, T).astype(np.float32)


def uniform_ids(nnz, T, seed=22):
    return np.random.default_rng(seed).integers(0, T, nnz).astype(np.uint8)


def panel_taken(algo, N, G, X):
    """Whether sm_sddmm / sm_sddmm_table run the vector kernel for these operands."""
    if algo == "parity" or N < 4 or N % 4:
        return False
    ok = lambda t: t.data_ptr() % 16 == 0 and (t.dim() == 1 or t.stride(0) % 4 == 0)
    return ok(G) and ok(X)


def check_gradient(M, rp, ci, ids, T, G, X, out0, alpha, beta, algo, Gd=None, Xd=None, out_dev=None, p=None):
    """sddmm_table against the restatement fed with the GPU's own dots, bit for bit, and against
    float64 within the header's bound.  Returns the per-chunk partials (shared by the (alpha,
    beta) pairs of one (N, algo))."""
    Gd = to_dev(G) if Gd is None else Gd
    Xd = to_dev(X) if Xd is None else Xd
    if p is None:
        d = to_host(M.sddmm(Gd, Xd, alpha=1.0, beta=0.0, algo=algo))
        p = table_ref.chunk_partials(d, ids, T)
    want = table_ref.finish_partials(p, out0, alpha, beta)
    out = to_dev(out0.copy()) if out_dev is None else out_dev
    got = to_host(M.sddmm_table(Gd, Xd, out=out, alpha=alpha, beta=beta, algo=algo))
    tag = f"N={G.shape[1] if G.ndim == 2 else 1} algo={algo} alpha={alpha} beta={beta}"
    assert np.array_equal(bits(got), bits(want)), tag + ": not the stated order"
    val, absum, R = table_ref.exact_by_id(rp, ci, ids, T, G, X, out0, alpha, beta,
                                          panel_taken(algo, G.shape[1] if G.ndim == 2 else 1, Gd, Xd))
    err = np.abs(got.astype(np.float64) - val)
    assert np.all(err <= R * U * absum + 1e-37), f"{tag}: worst ratio {float((err / (R * U * absum + 1e-37)).max()):.3g}"
    return p


# ------------------------------------------------------------------------- gradient: the grid
PATTERNS = {"300x257": (300, 257, 6, False),          # one partial chunk
            "1000x777": (1000, 777, 5, False),        # three chunks, the last of 904 terms
            "5000x1000_long": (5000, 1000, 5, True)}  # 13 chunks, a 1000-term row


def id_cases(nnz):
    cases = {f"T{T}": (T, uniform_ids(nnz, T)) for T in (1, 7, 255)}   # T = 1: 2048 adds on one id per chunk
    rng = np.random.default_rng(23)
    cases["id3_unused"] = (7, np.array([0, 1, 2, 4, 5, 6], np.uint8)[rng.integers(0, 6, nnz)])
    run = uniform_ids(nnz, 7, seed=24)
    if nnz > 2100:
        run[2000:2100] = 2   # a run of equal ids across the first chunk boundary
    cases["run_over_boundary"] = (7, run)
    return cases


@pytest.mark.parametrize("ids_case", ["T1", "T7", "T255", "id3_unused", "run_over_boundary"])
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_gradient_grid(sm, pat, ids_case):
    n_rows, n_cols, per, long_row = PATTERNS[pat]
    rp, ci = pattern(n_rows, n_cols, per, long_row=long_row)
    T, ids = id_cases(ci.size)[ids_case]
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), n_cols)
    assert M.info()["table_size"] == T and M.info()["table_updatable"] == 0
    for N in (1, 4, 32, 33):
        G, X, _ = grid_inputs(n_rows, n_cols, ci.size, N)
        out0 = np.random.default_rng(600 + N).uniform(-1, 1, T).astype(np.float32)
        Gd, Xd = to_dev(G), to_dev(X)
        for algo in ("auto", "parity"):
            p = None
            for alpha, beta in GRID_AB:
                p = check_gradient(M, rp, ci, ids, T, G, X, out0, alpha, beta, algo, Gd, Xd, p=p)


def test_gradient_on_the_transposed_companion(sm):
    """The ids travel with the terms: sddmm_table on M.T with G and X swapped gives the gradient
    of the same table in B^T's term order."""
    n_rows, n_cols = 1000, 777
    rp, ci = pattern(n_rows, n_cols, 5)
    T, ids = 7, uniform_ids(ci.size, 7)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), n_cols)
    Mt = M.T
    assert Mt.info()["table_size"] == T
    t_rp, t_ci, t_val = Mt.csr()
    t_ids = to_host(Mt.term_ids_device())
    assert np.array_equal(bits(t_val), bits(make_table(T)[t_ids]))
    assert np.array_equal(bits(to_host(Mt.table_device())), bits(make_table(T)))
    G, X, _ = grid_inputs(n_cols, n_rows, ci.size, 32)
    check_gradient(Mt, t_rp, t_ci, t_ids, T, G, X, np.zeros(T, np.float32), 1.3, 0.0, "auto")


# -------------------------------------------------------------------- gradient: placement etc.
def test_out_unaligned_and_padded_operands(sm):
    n_rows, n_cols, N = 1000, 777, 32
    rp, ci = pattern(n_rows, n_cols, 5)
    T, ids = 7, uniform_ids(ci.size, 7)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), n_cols)
    G, X, _ = grid_inputs(n_rows, n_cols, ci.size, N)
    out0 = np.random.default_rng(5).uniform(-1, 1, T).astype(np.float32)
    # d_out 4 bytes past 16-byte alignment, guard words around it
    out, parent = placed(out0, 1)
    check_gradient(M, rp, ci, ids, T, G, X, out0, 1.3, 1.0, "auto", out_dev=out)
    assert_guards(parent, 1, T)
    # padded ldg / ldx, the padding holds NaN: ld 36 keeps the vector kernel, ld 35 does not
    for ld in (36, 35):
        Gp, g_par = placed_2d(G, ld, 0)
        Xp, x_par = placed_2d(X, ld, 0)
        for algo in ("auto", "parity"):
            check_gradient(M, rp, ci, ids, T, G, X, out0, -0.7, 0.5, algo, Gp, Xp)
        assert_guards_2d(g_par, 0, n_rows, N, ld)
        assert_guards_2d(x_par, 0, n_cols, N, ld)


def test_deterministic(sm):
    rp, ci = pattern(5000, 1000, 5, long_row=True)
    T, ids = 255, uniform_ids(ci.size, 255)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), 1000)
    G, X, _ = grid_inputs(5000, 1000, ci.size, 32)
    Gd, Xd = to_dev(G), to_dev(X)
    for algo in ("auto", "parity"):
        assert same_bits(M.sddmm_table(Gd, Xd, algo=algo), M.sddmm_table(Gd, Xd, algo=algo))


def test_sddmm_table_two_streams(sm):
    """sddmm_table calls on one matrix from two streams at once: the per-chunk partials belong to
    the matrix, so the library makes the calls take turns on the device and every result equals
    its one-stream result bit for bit (three chunks of partials, the last one partial)."""
    torch = torch_dev()
    n_rows, n_cols, N, T = 1000, 777, 4, 7
    rp, ci = pattern(n_rows, n_cols, 5)
    ids = uniform_ids(ci.size, T)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), n_cols)
    pairs = []
    for k in range(8):
        G, X, _ = grid_inputs(n_rows, n_cols, ci.size, N, seed=700 + 10 * k)
        pairs.append((to_dev(G), to_dev(X)))
    want = [bits(to_host(M.sddmm_table(Gd, Xd))) for Gd, Xd in pairs]   # on the default stream
    assert any(not np.array_equal(want[0], w) for w in want[1:])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [to_dev(np.zeros(T, np.float32)) for _ in pairs]
    torch.cuda.synchronize()
    for rep in range(3):
        for out in outs:
            out.fill_(1.0)   # (finite: beta = 0 still multiplies)
        torch.cuda.synchronize()
        for i, ((Gd, Xd), out) in enumerate(zip(pairs, outs)):
            with torch.cuda.stream(streams[i % 2]):
                M.sddmm_table(Gd, Xd, out=out)
        torch.cuda.synchronize()
        for i, out in enumerate(outs):
            assert np.array_equal(bits(to_host(out)), want[i]), (rep, i)


def test_alpha_zero_takes_no_operands(sm):
    rp, ci = pattern(300, 257, 6)
    T, ids = 7, uniform_ids(ci.size, 7)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), 257)
    out0 = np.random.default_rng(5).uniform(-1, 1, T).astype(np.float32)
    got = to_host(M.sddmm_table(None, None, out=to_dev(out0.copy()), alpha=0.0, beta=0.5))
    assert np.array_equal(bits(got), bits(np.float32(0.5) * out0))
    got = to_host(M.sddmm_table(None, None, out=to_dev(out0.copy()), alpha=0.0, beta=1.0))
    assert np.array_equal(bits(got), bits(out0))


def test_empty_matrix(sm):
    """nnz = 0: the finish step alone, every S[t] = -0.0."""
    torch = torch_dev()
    rp, none = np.zeros(6, np.int32), np.zeros(0, np.int32)
    T = 3
    M = sm.SparseMatrix.from_csr_ids(rp, none, np.zeros(0, np.uint8), make_table(T), 7,
                                     opts=dict(table_updatable=1))
    out0 = np.array([0.25, -0.0, 0.0], np.float32)
    G, X = torch.ones(5, 4, device="cuda"), torch.ones(7, 4, device="cuda")
    for alpha, beta in GRID_AB:
        got = to_host(M.sddmm_table(G, X, out=to_dev(out0.copy()), alpha=alpha, beta=beta))
        want = table_ref.reduce_by_id(np.zeros(0, np.float32), np.zeros(0, np.uint8), T, out0, alpha, beta)
        assert np.array_equal(bits(got), bits(want))
    M.set_table(to_dev(make_table(T, seed=9)))
    M.axpy_table(0.5, to_dev(make_table(T, seed=10)))
    want = axpy_reference(make_table(T, seed=9), 0.5, make_table(T, seed=10))
    assert np.array_equal(bits(to_host(M.table_device())), bits(want))
    assert M.T.info()["table_updatable"] == 1


# --------------------------------------------------------------------------------- autograd
def test_autograd_table_leaf(sm):
    torch = torch_dev()
    from sparsematrix_amd import autograd
    n_rows, n_cols, N, alpha = 300, 257, 32, 1.3
    rp, ci = pattern(n_rows, n_cols, 6)
    T, ids = 7, uniform_ids(ci.size, 7)
    table = make_table(T)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, n_cols)
    G, X, _ = grid_inputs(n_rows, n_cols, ci.size, N)
    Gd, Xd = to_dev(G), to_dev(X)
    leaf = M.table_device().requires_grad_()
    autograd.apply_table(M, Xd, alpha=alpha, table=leaf).backward(Gd)
    assert M._t is None   # X needs no gradient: the companion is not built
    assert same_bits(leaf.grad, M.sddmm_table(Gd, Xd, alpha=alpha))
    # torch's own gradient through a dense B built from (pattern, table[ids])
    tl = to_dev(table).requires_grad_()
    rows = to_dev(table_ref.term_rows(rp))
    B = torch.zeros(n_rows, n_cols, device="cuda").index_put((rows, to_dev(ci.astype(np.int64))),
                                                              tl[to_dev(ids.astype(np.int64))])
    (alpha * (B @ Xd)).backward(Gd)
    val, absum, R = table_ref.exact_by_id(rp, ci, ids, T, G, X, np.zeros(T, np.float32), alpha, 0.0, True)
    err = np.abs(to_host(leaf.grad).astype(np.float64) - to_host(tl.grad).astype(np.float64))
    assert np.all(err <= R * U * absum)
    with pytest.raises(ValueError):
        autograd.apply_table(M, Xd, table=leaf[:-1])


def test_sgd_steps_keep_leaf_and_matrix_equal(sm):
    """The docstring's step: axpy_table on the matrix and the same two roundings on the leaf."""
    torch = torch_dev()
    from sparsematrix_amd import autograd
    n_rows, n_cols, N, lr = 5000, 1000, 4, 0.05
    rp, ci = pattern(n_rows, n_cols, 5)
    T, ids = 200, uniform_ids(ci.size, 200)
    m = sm.SparseMatrix.from_csr_ids(rp, ci, ids, make_table(T), n_cols, opts=dict(table_updatable=1))
    leaf = m.table_device().requires_grad_()
    rng = np.random.default_rng(8)
    for step in range(3):
        X = to_dev(rng.uniform(-1, 1, (n_cols, N)).astype(np.float32))
        G = to_dev(rng.uniform(-1, 1, (n_rows, N)).astype(np.float32))
        autograd.apply_table(m, X, alpha=1.0, table=leaf).backward(G)
        m.axpy_table(-lr, leaf.grad)
        with torch.no_grad():
            leaf.add_(leaf.grad * (-lr))
            leaf.grad = None
        assert same_bits(m.table_device(), leaf.detach()), f"step {step}: leaf != table"
        assert np.array_equal(bits(m.csr()[2]), bits(to_host(leaf.detach())[ids])), f"step {step}: CSR values"
    assert not np.array_equal(bits(to_host(leaf.detach())), bits(make_table(T)))


# ------------------------------------------------------------------------ the unflagged matrix
@pytest.mark.parametrize("opts", [None, dict(layout="cband")], ids=["auto", "cband"])
def test_unflagged_is_the_matrix_from_the_expanded_values(sm, opts):
    n_rows, n_cols = 5000, 1000
    rp, ci = pattern(n_rows, n_cols, 5)
    T, ids = 200, uniform_ids(ci.size, 200)
    table = make_table(T)
    A = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, n_cols, opts=opts)
    B = sm.SparseMatrix.from_csr(rp, ci, table[ids], n_cols, opts=opts)
    ia, ib = A.info(), B.info()
    assert ia["table_size"] == T and ib["table_size"] == 0
    # the ids, the table and the gradient's partials are counted in device_bytes
    assert ia["device_bytes"] > ib["device_bytes"]
    assert dict(ia, table_size=0, device_bytes=0) == dict(ib, device_bytes=0)
    if opts:
        assert ia["has_xband"] == 5
    assert_same_products(A, B, Operands(n_rows, n_cols), "unflagged:")


# --------------------------------------------------------- set_table / axpy_table vs a fresh build
T_UPD = 200


def update_tables():
    """table1: 200 distinct entries.  table2: two equal entries, the SPECIAL_BITS patterns on a few
    entries; entry 199 is used by no term (ids_for_update)."""
    t1 = make_table(T_UPD, seed=31)
    assert np.unique(bits(t1)).size == T_UPD
    t2 = make_table(T_UPD, seed=32)
    t2[9] = t2[5]
    t2.view(np.uint32)[20:20 + table_ref.SPECIAL_BITS.size] = table_ref.SPECIAL_BITS
    return t1, t2, make_table(T_UPD, seed=33)


def ids_for_update(nnz):
    return np.random.default_rng(34).integers(0, T_UPD - 1, nnz).astype(np.uint8)


def check_case(sm, rp, ci, n_cols, opts, expect=None, companion=False):
    """set_table and axpy_table against fresh builds, for one pattern and one set of options."""
    n_rows, nnz = rp.size - 1, ci.size
    opts = dict(opts, table_updatable=1)
    t1, t2, delta = update_tables()
    ids = ids_for_update(nnz)
    ops = Operands(n_rows, n_cols)
    build = lambda t: sm.SparseMatrix.from_csr_ids(rp, ci, ids, t, n_cols, opts=opts)
    M, F = build(t1), build(t2)
    info = M.info()
    assert info["table_updatable"] == 1 and info["updatable"] == 0 and info["table_size"] == T_UPD
    for k, v in (expect or {}).items():
        assert info[k] == v, (k, info[k], v)
    assert F.info() == info
    T = M.T if companion else None
    M.set_table(to_dev(t2))
    assert np.array_equal(bits(M.csr()[2]), bits(t2[ids]))
    assert_same_matrix(M, F, ops, "set_table:")
    if companion:
        assert T.info()["table_updatable"] == 1
        assert_same_matrix(T, F.transposed(), Operands(n_cols, n_rows), "companion:")
    M2 = build(t1)
    M2.axpy_table(AXPY_A, to_dev(delta))
    F2 = build(axpy_reference(t1, AXPY_A, delta))
    assert_same_matrix(M2, F2, ops, "axpy_table:")
    M2.axpy_table(0.0, None)   # a == 0: nothing launched, delta not read
    assert_same_matrix(M2, F2, ops, "axpy a=0:")
    return M


@pytest.mark.parametrize("band_tall", [0, 6])
@pytest.mark.parametrize("band_slabs", [1, 0])
@pytest.mark.parametrize("shape", [(5000, 1000, 5), (9000, 70001, 40)], ids=lambda s: "x".join(map(str, s)))
def test_cband(sm, shape, band_slabs, band_tall):
    n_rows, n_cols, per = shape
    rp, ci = pattern(n_rows, n_cols, per)
    check_case(sm, rp, ci, n_cols, dict(layout="cband", band_slabs=band_slabs, band_tall=band_tall),
               expect=dict(has_xband=5), companion=(band_slabs == 0 and band_tall == 0))


def test_bands_take_cband(sm):
    """The shape test_bands_take_band2_not_cband shows falling to band2 with `updatable`."""
    rp, ci = pattern(50000, 60000, 8)
    check_case(sm, rp, ci, 60000, dict(layout="bands"), expect=dict(has_xband=5))


@pytest.mark.parametrize("extra", [dict(), dict(relabel=1), dict(exact_sell=1)],
                         ids=["plain", "relabel", "exact_sell"])
def test_sell(sm, extra):
    rp, ci = pattern(5000, 1000, 5, long_row=True)
    M = check_case(sm, rp, ci, 1000, dict(layout="no_bands", sell_max_len=64, **extra),
                   expect=dict(has_xband=0, sell_codebook=1), companion=not extra)
    info = M.info()
    assert info["sell_slices"] > 0
    if "relabel" in extra:
        assert info["col_relabel"] == 1
    if "exact_sell" in extra:
        assert info["exact_sell_slices"] > 0


def test_ccsell(sm):
    rp, ci = pattern(9000, 70001, 40)
    M = check_case(sm, rp, ci, 70001, dict(ccsell=1, ccsell_chunk_log2=8), expect=dict(sell_codebook=1))
    assert M.info()["ccsell_chunks"] > 0


def test_sweep(sm):
    rp, ci = pattern(5000, 70000, 40)
    M = check_case(sm, rp, ci, 70000, dict(layout="sweep"))
    assert M.info()["sweep_blocks"] > 0


def test_captured_axpy_then_spmv(sm):
    """One stream: axpy_table then spmv, captured (a serial capture: no parallel branches) and
    replayed three times, against three eager steps on a twin."""
    torch = torch_dev()
    rp, ci = pattern(9000, 70001, 40)
    t1, _, delta = update_tables()
    ids = ids_for_update(ci.size)
    opts = dict(layout="cband", table_updatable=1)
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, t1, 70001, opts=opts)
    twin = sm.SparseMatrix.from_csr_ids(rp, ci, ids, t1, 70001, opts=opts)
    d = to_dev(delta)
    x = to_dev(np.random.default_rng(4).uniform(-1, 1, 70001).astype(np.float32))
    y, yt = torch.zeros(9000, device="cuda"), torch.zeros(9000, device="cuda")
    M.spmv(x, y, 1.0, 0.0)   # one eager product first (module load, scratch event)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.axpy_table(AXPY_A, d)
        M.spmv(x, y, 1.0, 0.0)
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        twin.axpy_table(AXPY_A, d)
        twin.spmv(x, yt, 1.0, 0.0)
        torch.cuda.synchronize()
        assert same_bits(y, yt)
    want = t1
    for _ in range(3):
        want = axpy_reference(want, AXPY_A, delta)
    assert np.array_equal(bits(to_host(M.table_device())), bits(want))
    assert np.array_equal(bits(M.csr()[2]), bits(want[ids]))


# -------------------------------------------------------------------------------- refusals
def _status(call):
    from sparsematrix_amd import _lib
    with pytest.raises(_lib.SparseMatrixError) as e:
        call()
    return e.value.status


def _new_calls(m, G, X, t):
    return (lambda: m.table_device(), lambda: m.term_ids_device(), lambda: m.sddmm_table(G, X),
            lambda: m.set_table(t), lambda: m.axpy_table(0.5, t))


def test_refusals(sm):
    torch = torch_dev()
    from sparsematrix_amd import _lib
    rp, ci, val = uniform_csr(300, 257, 6, seed=9)
    T, ids = 7, uniform_ids(ci.size, 7)
    table = make_table(T)
    G, X = torch.ones(300, 4, device="cuda"), torch.ones(257, 4, device="cuda")
    t = to_dev(table)
    # every new call on a from_csr matrix
    plain = sm.SparseMatrix.from_csr(rp, ci, val, 257)
    for call in _new_calls(plain, G, X, t):
        assert _status(call) == NOT_SUPPORTED
    # ... and on a dense-index matrix, with the hint
    index = np.full((16, 8), 255, np.uint8)
    index[::3, ::2] = 1
    dense = sm.SparseMatrix(index, 16, 8, 8, np.arange(1, 9, dtype=np.float32), 8)
    Gd, Xd = torch.ones(dense.n_rows, 4, device="cuda"), torch.ones(dense.n_cols, 4, device="cuda")
    for call in _new_calls(dense, Gd, Xd, torch.ones(8, device="cuda")):
        assert _status(call) == NOT_SUPPORTED
        assert b"sm_create_from_csr_ids" in _lib.load().sm_last_error()
    assert _status(lambda: dense.transposed(opts=dict(table_updatable=1))) == INVALID
    # an unflagged table matrix takes the gradient but no update
    unflagged = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, 257)
    unflagged.sddmm_table(G, X)
    assert _status(lambda: unflagged.set_table(t)) == NOT_SUPPORTED
    assert _status(lambda: unflagged.axpy_table(0.5, t)) == NOT_SUPPORTED
    assert np.array_equal(bits(unflagged.csr()[2]), bits(table[ids]))
    # a flagged one: no reference stream, and the table's length is checked in Python
    flagged = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, 257, opts=dict(table_updatable=1))
    assert _status(lambda: flagged.build_ref_stream()) == NOT_SUPPORTED
    assert flagged.info()["has_ref_stream"] == 0
    with pytest.raises(ValueError):
        flagged.set_table(t[:-1])
    with pytest.raises(ValueError):
        flagged.axpy_table(0.5, torch.ones(T + 1, device="cuda"))
    assert _lib.load().sm_set_table(flagged._h, None, None) == INVALID   # a null array with T > 0
    # options
    mk = lambda **o: sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, 257, opts=dict(o, table_updatable=1))
    for layout in ("exact", "blocked", "gather", "band2", "gcb"):
        assert _status(lambda: mk(layout=layout)) == INVALID
        assert b"table_updatable" in _lib.load().sm_last_error()
    assert _status(lambda: mk(sell_codebook=0)) == INVALID
    assert _status(lambda: mk(updatable=1)) == INVALID
    assert _status(lambda: sm.SparseMatrix.from_csr(rp, ci, val, 257, opts=dict(table_updatable=1))) == INVALID
    assert _status(lambda: sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(val), 257,
                                                    opts=dict(table_updatable=1))) == INVALID
    bad = ids.copy()
    bad[17] = T
    assert _status(lambda: sm.SparseMatrix.from_csr_ids(rp, ci, bad, table, 257)) == INVALID_MATRIX


# ------------------------------------------------------ derived table matrices on a side stream
@pytest.mark.parametrize("opts", [{}, {"table_updatable": 1}], ids=["default", "table_updatable"])
def test_derived_table_matrices_on_a_side_stream(sm, opts):
    """transposed, masked and quantized of a table matrix, made on a non-blocking stream, hold
    the source's table bit for bit and the restated ids, and multiply as the oracle does.

    This guards the stream ordering of the table hand-on: the new matrix's table is zeroed on the
    default stream and filled on the caller's, and nothing but the hand-on orders the two on a
    stream such as this one.  A missing order is a race, so this test cannot be made to fail
    reliably on a library that lacks it, and it is not looped to try."""
    import oracle
    import prune_ref
    import quantize_ref
    torch = torch_dev()
    oracle.build()
    n_rows, n_cols, T = 5, 7, 3
    rp = np.array([0, 2, 4, 5, 7, 9], np.int32)
    ci = np.array([0, 3, 1, 3, 6, 2, 5, 0, 4], np.int32)
    ids = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], np.uint8)
    table = np.array([0.5, -1.25, 3.0], np.float32)
    va = table[ids]
    keep = np.ones(ci.size, np.uint8)
    keep[4] = 0
    # the restatements: a stable sort by column; the compaction; the assignment rule
    order = np.argsort(ci, kind="stable")
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n_cols))]).astype(np.int32)
    t_ci = np.repeat(np.arange(n_rows, dtype=np.int32), np.diff(rp))[order]
    m_rp, m_ci, _, m_ids, _ = prune_ref.compact(rp, ci, va, keep, ids)
    want = {"transposed": (t_rp, t_ci, ids[order], n_rows),
            "masked": (m_rp, m_ci, m_ids, n_cols),
            "quantized": (rp, ci, quantize_ref.assign(va, table), n_cols)}
    M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, n_cols, opts=opts)
    rng = np.random.default_rng(31)
    with torch.cuda.stream(torch.cuda.Stream()):
        made = {"transposed": M.transposed(opts=opts),
                "masked": M.masked(to_dev(keep), opts=opts),
                "quantized": M.quantized(table_size=T, iters=0, init=M.table_device(), opts=opts)}
        for name, D in made.items():
            w_rp, w_ci, w_ids, w_cols = want[name]
            assert np.array_equal(bits(to_host(D.table_device())), bits(table)), name + ": table"
            assert np.array_equal(to_host(D.term_ids_device()), w_ids), name + ": ids"
            assert D.info()["table_size"] == T and D.info()["table_updatable"] == opts.get("table_updatable", 0), name
            x = rng.uniform(-1, 1, w_cols).astype(np.float32)
            y0 = rng.uniform(-1, 1, w_rp.size - 1).astype(np.float32)
            y = to_dev(y0)
            D.spmv(to_dev(x), y, 1.3, 0.7, algo="parity")
            assert np.array_equal(bits(to_host(y)), bits(oracle.csr_spmv(w_rp, w_ci, table[w_ids], x, y0, 1.3, 0.7))), \
                name + ": spmv"
