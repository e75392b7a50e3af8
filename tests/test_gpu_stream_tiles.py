"""The CSR kernels at every tile size and lane width (sparsematrix_amd/csrc/kernels.hip:
spmv_stream_kernel<256, 1024 / 2048 / 4096 / 8192>, spmv_long_finalize_kernel,
spmv_vector_kernel<2 .. 64>), on matrices that sit on the tile's own edges (stream_ref.edges) and
on the thresholds of the lane width (stream_ref.vector_cases).

Expected values come from outside the kernels: stream_ref.stream_spmv / vector_spmv restate the
two summation orders in numpy and are compared bit for bit on every row; oracle.csr_spmv is the
target of PARITY and EXACT and of STREAM's rows up to SM_SERIAL_ROW_MAX; everything is within
1e-6 * sum|terms| of the oracle; and the plan sm_info reports is the one the sanitizer-checked
planner program prints (tests/test_stream_plan_cpu.py).  Every matrix has at most 59 k terms.
"""
import numpy as np
import pytest

import oracle
import stream_ref as sr
from gpu_util import assert_guards, assert_terms_close, bits, placed, to_dev, to_host, torch_dev
from layout_specs import _same

pytestmark = pytest.mark.gpu

SCALARS = [(1.3, 0.7), (0.5, 0.0), (1.0, 1.0)]      # the second with y_in's NaNs
CSR_ONLY = dict(layout="no_bands", sell=0)
ALGO_PARITY, ALGO_STREAM = 1, 2                      # sm_algo


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _build(sm, c, **opts):
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=opts)
    info = M.info()
    assert info["has_xband"] == 0 and info["sell_slices"] == 0 and info["ccsell_chunks"] == 0 \
        and info["sweep_blocks"] == 0, info
    return M, info


def _plan_reported(info, c, tile):
    p = sr.plan(c.rp, tile)
    got = (info["n_tiles"], info["n_long_rows"], info["max_row_nnz"])
    assert got == (len(p.tiles), len(p.long_rows), p.max_row_nnz), (tile, got)


def _twice(M, c, xd, alpha, beta, algo):
    """The product run twice from the same y: equal bits; returns the host copy."""
    y0 = c.y_in(beta)
    outs = []
    for _ in range(2):
        y = to_dev(y0)
        M.spmv(xd, y, alpha, beta, algo=algo)
        outs.append(to_host(y).copy())
    _same(outs[1], outs[0], None, f"{algo} alpha {alpha} beta {beta}: second run")
    return outs[0]


def _stream_want(c, alpha, beta, tile):
    return sr.stream_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, tile)


def _check_stream_matrix(M, c, tile, algos=("stream", "auto")):
    """STREAM and AUTO against the restated order of `tile`, PARITY and EXACT against the oracle,
    all four within the bound, for the three scalar pairs.  The NaNs y_in plants for beta = 0 must
    be NaNs (gpu_util.assert_terms_close); every other output is compared in bits."""
    xd = to_dev(c.x)
    for alpha, beta in SCALARS:
        want, absum = c.ref(alpha, beta)
        ok = ~np.isnan(want)
        restated = _stream_want(c, alpha, beta, tile)
        for algo in algos + ("parity", "exact"):
            got = _twice(M, c, xd, alpha, beta, algo)
            tag = f"tile {tile} {algo} alpha {alpha} beta {beta}"
            assert_terms_close(got, want, absum)
            _same(got, want if algo in ("parity", "exact") else restated, ok, tag)


# ---------------------------------------------------------------------------- 1. every tile size
@pytest.mark.parametrize("T", sr.TILES)
def test_every_tile_size(sm, T):
    """edges(T) built with tile_nnz = T: the plan in sm_info is stream_ref.plan's; STREAM and AUTO
    give the restated bits on every row (the full one-row tile that starts at term 3, the tile cut
    by the 1024-row cap, the tile filled to exactly T, the wave-summed row behind 256 others, the
    long rows with an unaligned chunk and at the end of the arrays); PARITY and EXACT the
    oracle's.  Then STREAM with x and y one float past 16-byte alignment between guard words, and
    the same matrix with the column relabeling: the same bits."""
    c = sr.edges(T)
    M, info = _build(sm, c, relabel=0, tile_nnz=T, **CSR_ONLY)
    _plan_reported(info, c, T)
    assert info["col_relabel"] == 0 and info["exact_algo"] == ALGO_PARITY, info
    _check_stream_matrix(M, c, T)
    alpha, beta = SCALARS[0]
    restated = _stream_want(c, alpha, beta, T)
    xv, xp = placed(c.x, 1)
    yv, yp = placed(c.y_in(beta), 1)
    M.spmv(xv, yv, alpha, beta, algo="stream")
    _same(to_host(yv), restated, None, f"tile {T} stream, x and y one float off alignment")
    assert_guards(yp, 1, c.n_rows)
    assert_guards(xp, 1, c.n_cols)
    assert np.array_equal(bits(to_host(xv)), bits(c.x)), "x was written"
    R, rinfo = _build(sm, c, relabel=1, tile_nnz=T, **CSR_ONLY)
    _plan_reported(rinfo, c, T)
    assert rinfo["col_relabel"] == 1, rinfo
    for alpha, beta in SCALARS:
        got = _twice(R, c, to_dev(c.x), alpha, beta, "stream")
        _same(got, _stream_want(c, alpha, beta, T), ~np.isnan(c.y_in(beta)), f"tile {T} stream relabel=1")


# ---------------------------------------------------------------------------- 2. tile_nnz = 0
@pytest.mark.parametrize("name", ["longest=64mean", "longest=64mean+1", "edges4096"])
def test_automatic_tile_choice(sm, name):
    """tile_nnz = 0: upload_plan takes 4096, or 2048 when the longest row is strictly above 64 x the
    mean.  The plan reported and the bits are those of stream_ref.auto_tile's size (the other
    size gives another plan and other bits: tests/test_stream_plan_cpu.py)."""
    c, tile = sr.auto_cases()[name]
    M, info = _build(sm, c, relabel=0, tile_nnz=0, **CSR_ONLY)
    _plan_reported(info, c, tile)
    _check_stream_matrix(M, c, tile)


# ---------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("tile", [512, 3000, 16384, -1])
def test_tile_nnz_refused(sm, tile):
    """A tile size with no kernel instantiation is SM_ERR_INVALID_ARG; nothing is built."""
    c, _ = sr.vector_cases()["mean8"]
    with pytest.raises(sm.SparseMatrixError) as ei:
        sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=dict(tile_nnz=tile, **CSR_ONLY))
    assert ei.value.status == 1   # SM_ERR_INVALID_ARG
    assert "tile_nnz" in str(ei.value)


# ---------------------------------------------------------------------------- 4. two streams
def test_long_row_partials_from_two_streams(sm):
    """Eight STREAM products with different x on the T = 1024 matrix, issued alternately on two
    streams with no host synchronisation between them.  The long rows' chunk sums live in one
    scratch array of the matrix; the library orders the products on the device, so every result
    is the restated one."""
    torch = torch_dev()
    c = sr.edges(1024)
    M, info = _build(sm, c, relabel=0, tile_nnz=1024, **CSR_ONLY)
    assert info["n_long_rows"] == 3, info
    rng = np.random.default_rng(33)
    xh = [rng.uniform(-1, 1, c.n_cols).astype(np.float32) for _ in range(8)]
    want = [sr.stream_spmv(c.rp, c.ci, c.va, x, c.y0, 1.0, 0.5, 1024) for x in xh]
    assert len({bits(w)[info["n_rows"] - 1] for w in want}) == 8     # the last long row tells the x apart
    xs = [to_dev(x) for x in xh]
    ys = [to_dev(c.y0) for _ in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(xs, ys)):
        with torch.cuda.stream(streams[i % 2]):
            M.spmv(x, y, 1.0, 0.5, algo="stream")
    torch.cuda.synchronize()
    for i, y in enumerate(ys):
        _same(to_host(y), want[i], None, f"product {i} of 8 on two streams")


# ---------------------------------------------------------------------------- 5. vector
@pytest.mark.parametrize("name", [n for n, _, _ in sr._vector_shapes()])
def test_vector_every_width(sm, name):
    """SM_ALGO_VECTOR with the mean row length on and just past each threshold of the lane width:
    bit-identical to stream_ref.vector_spmv at L = vector_lanes (L/2 and 2L give other bits:
    tests/test_stream_plan_cpu.py), within the bound, the same bits on a second run."""
    c, L = sr.vector_cases()[name]
    M, info = _build(sm, c, **CSR_ONLY)
    assert (info["n_rows"], info["nnz"]) == (c.n_rows, int(c.rp[-1]))
    xd = to_dev(c.x)
    for alpha, beta in SCALARS:
        want, absum = c.ref(alpha, beta)
        got = _twice(M, c, xd, alpha, beta, "vector")
        assert_terms_close(got, want, absum)
        restated = sr.vector_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, L)
        _same(got, restated, ~np.isnan(want), f"{name} vector L {L} alpha {alpha} beta {beta}")


# ---------------------------------------------------------------------------- 6. EXACT's switch
def test_exact_switches_at_serial_row_max(sm):
    """Longest row 64: EXACT is the stream kernel, bit-identical to the oracle at each tile size.
    One row grown to 65: EXACT is PARITY, still bit-identical."""
    at64, at65 = sr.exact_cases()
    for c, algo in ((at64, ALGO_STREAM), (at65, ALGO_PARITY)):
        xd = to_dev(c.x)
        for T in sr.TILES:
            M, info = _build(sm, c, tile_nnz=T, **CSR_ONLY)
            _plan_reported(info, c, T)
            assert info["exact_algo"] == algo and info["max_row_nnz"] == int(c.lens.max()), info
            for alpha, beta in SCALARS:
                want, _ = c.ref(alpha, beta)
                got = _twice(M, c, xd, alpha, beta, "exact")
                _same(got, want, ~np.isnan(want), f"exact, longest row {c.lens.max()}, tile {T}")
                assert np.array_equal(np.isnan(got), np.isnan(want))
