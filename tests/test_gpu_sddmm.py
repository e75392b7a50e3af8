"""sm_sddmm on the GPU: out[e] = alpha * <G[r_e, :], X[c_e, :]> + beta * out[e] per stored term,
sm_copy_csr_device, and the gradient of the stored values through autograd.apply.

Oracles (tests/sddmm_ref.py): SM_ALGO_PARITY against the header's order restated in numpy float32,
bit for bit; SM_ALGO_AUTO against the float64 value within the project's 1e-6 * sum|terms| bound
(test_sddmm_cpu.py shows the float32 restatement itself sits inside it on these inputs).
"""
import ctypes as C

import numpy as np
import pytest

import sddmm_ref
from golden_util import bits_equal, load_case
from gpu_util import (assert_guards, assert_guards_2d, assert_terms_close, bits, placed, placed_2d,
                      skewed_csr, to_dev, to_host, torch_dev, uniform_csr)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


@pytest.fixture(scope="module")
def grid_case(sm):
    rp, ci, va = uniform_csr(300, 257, 6, seed=501)
    return sm.SparseMatrix.from_csr(rp, ci, va, 257), rp, ci, va


def run(m, G, X, out0, alpha, beta, algo):
    out = to_dev(np.asarray(out0, np.float32))
    res = m.sddmm(to_dev(G), to_dev(X), out, alpha, beta, algo=algo)
    assert res is out
    return to_host(out)


def check_both(m, rp, ci, G, X, out0, alpha, beta):
    """PARITY by bits, AUTO within the bound; returns (parity, auto)."""
    want32 = sddmm_ref.parity(rp, ci, G, X, out0, alpha, beta)
    want64, absum = sddmm_ref.exact(rp, ci, G, X, out0, alpha, beta)
    p = run(m, G, X, out0, alpha, beta, "parity")
    assert bits_equal(p, want32), "PARITY differs from the restated order"
    a = run(m, G, X, out0, alpha, beta, "auto")
    assert_terms_close(a, want64, absum)
    return p, a


# ------------------------------------------------------------------ 1. the (N, alpha, beta) grid
@pytest.mark.parametrize("ab", sddmm_ref.GRID_AB, ids=lambda ab: f"a{ab[0]}_b{ab[1]}")
@pytest.mark.parametrize("N", sddmm_ref.GRID_N)
def test_parity_is_the_restated_order(grid_case, N, ab):
    m, rp, ci, _ = grid_case
    G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, N)
    got = run(m, G, X, out0, ab[0], ab[1], "parity")
    assert bits_equal(got, sddmm_ref.parity(rp, ci, G, X, out0, ab[0], ab[1]))


@pytest.mark.parametrize("ab", sddmm_ref.GRID_AB, ids=lambda ab: f"a{ab[0]}_b{ab[1]}")
@pytest.mark.parametrize("N", sddmm_ref.GRID_N)
def test_auto_is_inside_the_bound_and_deterministic(grid_case, N, ab):
    m, rp, ci, _ = grid_case
    G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, N)
    want, absum = sddmm_ref.exact(rp, ci, G, X, out0, ab[0], ab[1])
    a1 = run(m, G, X, out0, ab[0], ab[1], "auto")
    a2 = run(m, G, X, out0, ab[0], ab[1], "auto")
    assert_terms_close(a1, want, absum)
    assert bits_equal(a1, a2), "two runs differ"
    if N == 1:
        assert bits_equal(a1, run(m, G, X, out0, ab[0], ab[1], "parity"))
    # every other sm_algo value runs as AUTO
    assert bits_equal(a1, run(m, G, X, out0, ab[0], ab[1], "sell"))


def test_one_dimensional_operands_are_n_rhs_1(grid_case):
    m, rp, ci, _ = grid_case
    G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, 1)
    out = m.sddmm(to_dev(G[:, 0]), to_dev(X[:, 0]), alpha=1.3)   # out=None: zeros, beta = 0
    assert tuple(out.shape) == (ci.size,) and out.dtype == torch_dev().float32
    assert bits_equal(to_host(out), sddmm_ref.parity(rp, ci, G, X, np.zeros(ci.size, np.float32), 1.3, 0.0))


# ---------------------------------------------------------------------- 2. pattern edge cases
# The vector kernel's workgroups take sddmm_ref.CHUNK = 2048 consecutive terms: the 5000-term row
# below starts at term 195, so chunk cuts fall at 2048 and 4096 inside it, and its end (5195)
# and the rows after it sit inside the third chunk.
SKEW_LENGTHS = np.array([0, 1, 2, 63, 64, 65, 5000, 0, 0, 3, 64, 1, 0], np.int64)


# N = 68: 32 lanes per term, 15 of them idle; N = 260: 64 lanes, two slots of the j axis per lane
@pytest.mark.parametrize("N", [3, 4, 32, 68, 260])
def test_skewed_rows_and_chunk_cuts(sm, N):
    assert SKEW_LENGTHS[:6].sum() == 195 and SKEW_LENGTHS.max() > 2 * sddmm_ref.CHUNK
    rp, ci, va = skewed_csr(SKEW_LENGTHS.size, 700, SKEW_LENGTHS, seed=502)
    assert (np.diff(ci[195:5195]) == 0).any()   # the long row repeats columns
    m = sm.SparseMatrix.from_csr(rp, ci, va, 700)
    G, X, out0 = sddmm_ref.grid_inputs(SKEW_LENGTHS.size, 700, ci.size, N, seed=510)
    check_both(m, rp, ci, G, X, out0, 1.3, 0.5)


def test_repeated_columns_within_a_row(sm):
    rp = np.array([0, 5, 5, 8], np.int32)
    ci = np.array([3, 3, 3, 7, 7, 0, 0, 9], np.int32)
    va = np.arange(1, 9, dtype=np.float32)
    m = sm.SparseMatrix.from_csr(rp, ci, va, 10)
    for N in (1, 8):
        G, X, out0 = sddmm_ref.grid_inputs(3, 10, 8, N, seed=520)
        check_both(m, rp, ci, G, X, out0, -0.7, 1.0)
        p, a = check_both(m, rp, ci, G, X, out0, -0.7, 0.0)
        for res in (p, a):   # equal (row, column) pairs give equal dots
            assert bits_equal(res[0:3], np.repeat(res[0], 3)) and bits_equal(res[5:7], np.repeat(res[5], 2))


def test_one_by_one(sm):
    rp, ci, va = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5], np.float32)
    m = sm.SparseMatrix.from_csr(rp, ci, va, 1)
    for N in (1, 4, 5):
        G, X, out0 = sddmm_ref.grid_inputs(1, 1, 1, N, seed=530)
        check_both(m, rp, ci, G, X, out0, 1.3, 0.5)


def test_no_terms(sm):
    torch = torch_dev()
    rp = np.zeros(5, np.int32)
    m = sm.SparseMatrix.from_csr(rp, np.zeros(0, np.int32), np.zeros(0, np.float32), 6)
    G, X, _ = sddmm_ref.grid_inputs(4, 6, 0, 4, seed=540)
    out = m.sddmm(to_dev(G), to_dev(X))
    torch.cuda.synchronize()
    assert out.numel() == 0
    assert m._L.sm_sddmm(m._h, 4, 1.0, None, 4, None, 4, 0.0, None, 0, None) == 0   # launches nothing
    rp_d, ci_d, va_d = m.csr_device()
    assert np.array_equal(to_host(rp_d), rp) and ci_d.numel() == 0 and va_d.numel() == 0


@pytest.mark.parametrize("name", ["sweep_257x300_0.001_t_T255", "sweep_300x256_0.25_n_T255"])
@pytest.mark.parametrize("transposed", [False, True], ids=["B", "BT"])
def test_golden_copyform_term_order_is_csr(sm, name, transposed):
    """A CopyForm-built matrix (and its .T): the terms are those of csr(), row by row in
    ascending column, which is the live mask of the index read row-major."""
    c = load_case(name)
    src = sm.SparseMatrix(c.dm, c.rows, c.cols, c.stride, c.table, c.table_size,
                          sm.SblasTrans if c.trans else sm.SblasNoTrans)
    m, live = src, c.live_mask_b()
    if transposed:   # src stays alive: the companion goes with it
        m, live = src.T, np.ascontiguousarray(live.T)
    rows, cols = np.nonzero(live)
    rp = np.zeros(live.shape[0] + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=live.shape[0]))
    got_rp, got_ci, _ = m.csr()
    assert np.array_equal(got_rp, rp) and np.array_equal(got_ci, cols)
    for N in (1, 32):
        G, X, out0 = sddmm_ref.grid_inputs(live.shape[0], live.shape[1], cols.size, N, seed=550)
        check_both(m, rp, cols.astype(np.int32), G, X, out0, 1.3, 0.5)


# ------------------------------------------------------------------------------- 3. placement
PLACE_N = 8
PLACE_OFFS = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (0, 0, 2), (1, 2, 3), (3, 3, 1), (2, 1, 0)]


@pytest.mark.parametrize("lds", [(8, 12), (12, 8), (9, 8), (8, 9), (12, 9), (9, 12)],
                         ids=lambda l: f"ldg{l[0]}_ldx{l[1]}")
def test_operand_placement(grid_case, lds):
    """G, X, out at float offsets 0..3, ld in {N, N+1, N+4} with ldg != ldx: guards and padding
    columns bit-unchanged, PARITY by bits, AUTO inside the bound.  The vector kernel takes the
    placements with both offsets 0 and both ld % 4 == 0; there AUTO uses fused multiply-adds and
    a tree, so it differs from PARITY in some bits, while everywhere else it is the PARITY
    kernel: both kernels ran, and they agree within the bound."""
    m, rp, ci, _ = grid_case
    N, (ldg, ldx) = PLACE_N, lds
    G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, N, seed=560)
    alpha, beta = 1.3, 0.5
    want32 = sddmm_ref.parity(rp, ci, G, X, out0, alpha, beta)
    want64, absum = sddmm_ref.exact(rp, ci, G, X, out0, alpha, beta)
    for og, ox, oo in PLACE_OFFS:
        vector = og == 0 and ox == 0 and ldg % 4 == 0 and ldx % 4 == 0
        for algo in ("parity", "auto"):
            Gv, Gp = placed_2d(G, ldg, og)
            Xv, Xp = placed_2d(X, ldx, ox)
            ov, op = placed(out0, oo)
            g_before, x_before = to_host(Gp.view(torch_dev().int32)), to_host(Xp.view(torch_dev().int32))
            m.sddmm(Gv, Xv, ov, alpha, beta, algo=algo)
            got = to_host(ov)
            assert_guards(op, oo, ci.size)
            assert_guards_2d(Gp, og, 300, N, ldg)
            assert_guards_2d(Xp, ox, 257, N, ldx)
            assert np.array_equal(to_host(Gp.view(torch_dev().int32)), g_before), "G written"
            assert np.array_equal(to_host(Xp.view(torch_dev().int32)), x_before), "X written"
            assert_terms_close(got, want64, absum)
            if algo == "parity" or not vector:
                assert bits_equal(got, want32), (og, ox, oo, algo)
            else:
                assert not bits_equal(got, want32), "the vector kernel did not run"


# --------------------------------------------------------------------------- 4. special values
def test_beta_zero_propagates_nan(grid_case):
    m, rp, ci, _ = grid_case
    for N in (1, 32):
        G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, N, seed=570)
        out0[[0, 7, ci.size - 1]] = np.nan
        out0[11] = np.inf
        for algo in ("parity", "auto"):
            got = run(m, G, X, out0, 1.3, 0.0, algo)
            assert np.isnan(got[[0, 7, ci.size - 1, 11]]).all()   # 0 * inf is NaN as well
            keep = np.isfinite(out0)
            want, absum = sddmm_ref.exact(rp, ci, G, X, np.where(keep, out0, 0), 1.3, 0.0)
            assert_terms_close(got[keep], want[keep], absum[keep])


@pytest.mark.parametrize("beta", [0.5, 1.0, 0.0])
def test_alpha_zero_only_scales(grid_case, beta):
    torch = torch_dev()
    m, rp, ci, _ = grid_case
    out0 = sddmm_ref.grid_inputs(300, 257, ci.size, 1, seed=580)[2]
    out, parent = placed(out0, 1)
    stream = int(torch.cuda.current_stream().cuda_stream)
    st = m._L.sm_sddmm(m._h, 32, 0.0, None, 32, None, 32, beta, C.c_void_p(out.data_ptr()), 0, stream)
    assert st == 0
    want = out0 if beta == 1.0 else (np.float32(beta) * out0).astype(np.float32)
    assert bits_equal(to_host(out), want)
    assert_guards(parent, 1, ci.size)


# ----------------------------------------------------------------------------- 5. graph capture
def test_graph_capture_and_replay(grid_case):
    """Two sddmm calls (vector kernel, N = 32; PARITY kernel, N = 3) captured serially into one
    graph and replayed three times onto fresh `out`: the eager bits every time."""
    torch = torch_dev()
    m, rp, ci, _ = grid_case
    Ga, Xa, oa = sddmm_ref.grid_inputs(300, 257, ci.size, 32, seed=590)
    Gb, Xb, ob = sddmm_ref.grid_inputs(300, 257, ci.size, 3, seed=591)
    eager = [run(m, Ga, Xa, oa, 1.3, 0.5, "auto"), run(m, Gb, Xb, ob, -0.7, 1.0, "auto")]
    dGa, dXa, dGb, dXb = to_dev(Ga), to_dev(Xa), to_dev(Gb), to_dev(Xb)
    outs = [to_dev(oa), to_dev(ob)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.sddmm(dGa, dXa, outs[0], 1.3, 0.5)
        m.sddmm(dGb, dXb, outs[1], -0.7, 1.0)
    torch.cuda.synchronize()
    for _ in range(3):
        outs[0].copy_(torch.from_numpy(oa))
        outs[1].copy_(torch.from_numpy(ob))
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(to_host(outs[0]), eager[0]) and bits_equal(to_host(outs[1]), eager[1])


# -------------------------------------------------------------------------------- 6. csr_device
def test_csr_device_round_trip(sm, grid_case):
    torch = torch_dev()
    m, rp, ci, va = grid_case
    d = m.csr_device()
    assert [t.dtype for t in d] == [torch.int32, torch.int32, torch.float32]
    assert all(t.is_cuda for t in d)
    host = m.csr()
    assert np.array_equal(to_host(d[0]), host[0]) and np.array_equal(to_host(d[1]), host[1])
    assert np.array_equal(bits(to_host(d[2])), bits(host[2]))
    assert np.array_equal(to_host(d[0]), rp) and np.array_equal(bits(to_host(d[2])), bits(va))
    assert sm.SparseMatrix.from_csr(*d, 257) == m
    # a CopyForm-built matrix too
    c = load_case("sweep_257x300_0.001_t_T255")
    g = sm.SparseMatrix(c.dm, c.rows, c.cols, c.stride, c.table, c.table_size,
                        sm.SblasTrans if c.trans else sm.SblasNoTrans)
    dg, hg = g.csr_device(), g.csr()
    assert all(np.array_equal(to_host(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(dg, hg))


# ---------------------------------------------------------------------------------- 7. autograd
@pytest.mark.parametrize("N", [1, 4])
def test_autograd_values(sm, grid_case, N):
    torch = torch_dev()
    from sparsematrix_amd import autograd
    _, rp, ci, va = grid_case
    m = sm.SparseMatrix.from_csr(rp, ci, va, 257)   # its own matrix: m._t is watched below
    rng = np.random.default_rng(600 + N)
    tail = () if N == 1 else (N,)
    Xh = rng.uniform(-1, 1, (257,) + tail).astype(np.float32)
    Gh = rng.uniform(-1, 1, (300,) + tail).astype(np.float32)
    G = to_dev(Gh)
    if N > 1:
        G = to_dev(np.ascontiguousarray(Gh.T)).t()   # a non-contiguous grad_Y
        assert not G.is_contiguous()
    want_vals = to_host(m.sddmm(G.contiguous(), to_dev(Xh), alpha=1.3))
    want64, absum = sddmm_ref.exact(rp, ci, Gh, Xh, np.zeros(ci.size), 1.3, 0.0)

    # only the values: no transposed companion is built
    X = to_dev(Xh)
    vals = m.csr_device()[2].requires_grad_()
    Y = autograd.apply(m, X, alpha=1.3, values=vals)
    Y.backward(G)
    assert m._t is None
    assert X.grad is None and vals.grad.shape == vals.shape
    assert bits_equal(to_host(vals.grad), want_vals)
    assert_terms_close(to_host(vals.grad), want64, absum)
    Y_plain = autograd.apply(m, to_dev(Xh), alpha=1.3)
    assert bits_equal(to_host(Y), to_host(Y_plain))

    # X alone, the call as it was before `values` existed
    X0 = to_dev(Xh).requires_grad_()
    autograd.apply(m, X0, alpha=1.3).backward(G)
    # both
    X1 = to_dev(Xh).requires_grad_()
    vals1 = m.csr_device()[2].requires_grad_()
    autograd.apply(m, X1, alpha=1.3, values=vals1).backward(G)
    assert m._t is not None
    assert bits_equal(to_host(vals1.grad), want_vals)
    assert X1.grad.shape == X1.shape and bits_equal(to_host(X1.grad), to_host(X0.grad))

    with pytest.raises(ValueError):
        autograd.apply(m, X, alpha=1.3, values=torch.zeros(ci.size + 1, device="cuda"))
    with pytest.raises(TypeError):
        autograd.apply(m, X, alpha=1.3, values=torch.zeros(ci.size, device="cuda", dtype=torch.float64))
    with pytest.raises(TypeError):
        autograd.apply(m, X, alpha=1.3, values=torch.zeros(ci.size))


def test_python_operand_guards(grid_case):
    torch = torch_dev()
    m, rp, ci, _ = grid_case
    G, X, out0 = (to_dev(a) for a in sddmm_ref.grid_inputs(300, 257, ci.size, 4, seed=610))
    with pytest.raises(ValueError):
        m.sddmm(G, X[:, :3])                      # column counts differ
    with pytest.raises(ValueError):
        m.sddmm(G[:299], X)                       # wrong number of rows
    with pytest.raises(ValueError):
        m.sddmm(G.t().contiguous().t(), X)        # column-major
    with pytest.raises(ValueError):
        m.sddmm(G, X, out0[:-1])                  # out too short
    with pytest.raises(TypeError):
        m.sddmm(G.double(), X)
    with pytest.raises(TypeError):
        m.sddmm(G.cpu(), X)
    with pytest.raises(ValueError):
        m.sddmm(G, X, algo="fastest")
    torch.cuda.synchronize()
