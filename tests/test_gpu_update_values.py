"""In-place updates of the stored values (sm_build_opts.updatable, sm_set_values,
sm_axpy_values): after an update the matrix is what a fresh build from the new values gives.

Pattern of every case: M from (rp, ci, val1) with opts + updatable=1, F fresh from (rp, ci, val2)
with the same opts, update M, compare bit for bit -- the CSR values, ==, the layout digests and
every product of every algorithm.  No tolerance is involved anywhere: both sides run the same
kernels on what must be the same bytes.
"""
import numpy as np
import pytest

from gpu_util import bits, to_dev, to_host, torch_dev, uniform_csr

pytestmark = pytest.mark.gpu

NOT_SUPPORTED = 4
AXPY_A = -0.37
SPMV_ALGOS = ("auto", "parity", "stream", "vector", "xband", "sell", "merge", "exact")
ALPHA_BETA = ((1.0, 1.0), (1.3, 0.7), (0.5, 0.0))
# NaNs with payloads (quiet and signalling), +-0.0, +-inf, denormals
SPECIAL_BITS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000,
                         0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def new_values(nnz, seed, special=True):
    """Random fp32 values (more than 255 bit patterns); `special`: a few terms spread over the
    matrix carry SPECIAL_BITS, so most outputs stay finite and a stale slot would show."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, nnz).astype(np.float32)
    if special and nnz:
        at = rng.choice(nnz, min(nnz, SPECIAL_BITS.size), replace=False)
        v.view(np.uint32)[at] = SPECIAL_BITS[: at.size]
    return v


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


def build(sm, rp, ci, val, n_cols, opts, device_arrays=False):
    if device_arrays:
        return sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(val), n_cols, opts=opts)
    return sm.SparseMatrix.from_csr(rp, ci, val, n_cols, opts=opts)


def same_bits(a, b):
    torch = torch_dev()
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Operands:
    """One set of dense operands per shape, shared by every comparison of a case."""

    def __init__(self, n_rows, n_cols, seed=11):
        rng = np.random.default_rng(seed)
        u = lambda *s: to_dev(rng.uniform(-1, 1, s).astype(np.float32))
        self.x, self.y0 = u(n_cols), u(n_rows)
        self.X = {n: u(n_cols, n) for n in (4, 32)}
        self.Y0 = {n: u(n_rows, n) for n in (4, 32)}
        self.G4 = u(n_rows, 4)


def assert_same_matrix(M, F, ops, tag=""):
    """M is what F is: CSR (values by bits), ==, digests, and every product bit for bit."""
    m_csr, f_csr = M.csr(), F.csr()
    assert np.array_equal(m_csr[0], f_csr[0]) and np.array_equal(m_csr[1], f_csr[1]), tag + " pattern"
    assert np.array_equal(bits(m_csr[2]), bits(f_csr[2])), tag + " CSR values (bits)"
    assert M == F, tag + " =="
    assert M.layout_digest() == F.layout_digest(), tag + " layout digest"
    for algo in SPMV_ALGOS:
        for alpha, beta in ALPHA_BETA:
            ym, yf = ops.y0.clone(), ops.y0.clone()
            M.spmv(ops.x, ym, alpha, beta, algo=algo)
            F.spmv(ops.x, yf, alpha, beta, algo=algo)
            assert same_bits(ym, yf), f"{tag} spmv {algo} alpha={alpha} beta={beta}"
    for n, algo in ((4, "auto"), (32, "auto"), (32, "mfma")):
        Ym, Yf = ops.Y0[n].clone(), ops.Y0[n].clone()
        M.spmm(ops.X[n], Ym, 1.3, 0.7, algo=algo)
        F.spmm(ops.X[n], Yf, 1.3, 0.7, algo=algo)
        assert same_bits(Ym, Yf), f"{tag} spmm N={n} {algo}"
    assert same_bits(M.sddmm(ops.G4, ops.X[4]), F.sddmm(ops.G4, ops.X[4])), tag + " sddmm"


def axpy_reference(val, a, delta):
    """fl(val + fl(a * delta)) in float32 numpy: two separately rounded operations."""
    with np.errstate(invalid="ignore", over="ignore"):   # val may hold NaN / inf on purpose
        return (val + (np.float32(a) * delta)).astype(np.float32)


def check_case(sm, rp, ci, n_cols, opts, expect=None, companion=False):
    """set_values and axpy_values against fresh builds, for one pattern and one set of options."""
    n_rows, nnz = rp.size - 1, ci.size
    opts = dict(opts, updatable=1)
    val1, val2 = new_values(nnz, 1, special=False), new_values(nnz, 2)
    delta = new_values(nnz, 3, special=False)
    ops = Operands(n_rows, n_cols)
    M = build(sm, rp, ci, val1, n_cols, opts)
    # F through sm_create_from_csr_device_ex, except where the option is one only the host
    # constructors honour (exact_sell = 1 beside a CSR-built matrix)
    F = build(sm, rp, ci, val2, n_cols, opts, device_arrays="exact_sell" not in opts)
    info = M.info()
    assert info["updatable"] == 1 and info["sell_codebook"] == 0 and info["has_xband"] != 5
    for k, v in (expect or {}).items():
        assert info[k] == v, (k, info[k], v)
    assert F.info() == dict(info, device_bytes=F.info()["device_bytes"])
    T = M.T if companion else None
    M.set_values(to_dev(val2))
    assert np.array_equal(bits(M.csr()[2]), bits(val2))
    assert_same_matrix(M, F, ops, "set_values:")
    if companion:
        Ft = F.transposed()
        ops_t = Operands(n_cols, n_rows)
        assert T.info()["updatable"] == 1
        assert_same_matrix(T, Ft, ops_t, "companion:")
    # axpy on a matrix holding val1
    M2 = build(sm, rp, ci, val1, n_cols, opts)
    M2.axpy_values(AXPY_A, to_dev(delta))
    F2 = build(sm, rp, ci, axpy_reference(val1, AXPY_A, delta), n_cols, opts)
    assert_same_matrix(M2, F2, ops, "axpy_values:")
    M2.axpy_values(0.0, None)   # a == 0: nothing launched, delta not read
    assert_same_matrix(M2, F2, ops, "axpy a=0:")
    return M, F


# ------------------------------------------------------------------------------ layouts
BAND2_SHAPES = [(5000, 1000, 5), (9000, 70001, 40), (1, 50000, 30), (16384, 8192, 1), (40000, 20000, 3)]


@pytest.mark.parametrize("band_tall", [0, 6])
@pytest.mark.parametrize("band_slabs", [1, 0])
@pytest.mark.parametrize("shape", BAND2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_band2(sm, shape, band_slabs, band_tall):
    n_rows, n_cols, per = shape
    rp, ci = pattern(n_rows, n_cols, per)
    check_case(sm, rp, ci, n_cols, dict(layout="band2", band_slabs=band_slabs, band_tall=band_tall),
               expect=dict(has_xband=4))


@pytest.mark.parametrize("layout,kind", [("exact", 1), ("blocked", 2), ("gather", 3)])
def test_xband_kinds(sm, layout, kind):
    rp, ci = pattern(9000, 70001, 40)
    check_case(sm, rp, ci, 70001, dict(layout=layout), expect=dict(has_xband=kind))


@pytest.mark.parametrize("band_slabs", [1, 2])
def test_gcb(sm, band_slabs):
    rp, ci = pattern(9000, 70001, 40)
    check_case(sm, rp, ci, 70001, dict(layout="gcb", band_slabs=band_slabs), expect=dict(has_xband=6))


@pytest.mark.parametrize("extra", [dict(), dict(relabel=1), dict(exact_sell=1)],
                         ids=["plain", "relabel", "exact_sell"])
def test_sell(sm, extra):
    """One row of 1000 terms cut into 64-term segments; with the column relabeling; with the
    unsegmented sliced ELL beside it (a second copy of the values to refresh)."""
    rp, ci = pattern(5000, 1000, 5, long_row=True)
    M, _ = check_case(sm, rp, ci, 1000, dict(layout="no_bands", sell_max_len=64, **extra),
                      expect=dict(has_xband=0), companion=not extra)
    info = M.info()
    assert info["sell_slices"] > 0
    if "relabel" in extra:
        assert info["col_relabel"] == 1
    if "exact_sell" in extra:
        assert info["exact_sell_slices"] > 0


def test_ccsell(sm):
    rp, ci = pattern(9000, 70001, 40)
    M, _ = check_case(sm, rp, ci, 70001, dict(layout="no_bands", ccsell=1, ccsell_chunk_log2=8))
    assert M.info()["ccsell_chunks"] > 0


def test_bands_take_band2_not_cband(sm):
    """Values from a 200-entry table: without the option the bands are codebook words; with it
    no layout decision reads the values."""
    n_rows, n_cols, per = 50000, 60000, 8
    rp, ci = pattern(n_rows, n_cols, per)
    table = np.random.default_rng(5).uniform(-1, 1, 200).astype(np.float32)
    val1 = table[np.random.default_rng(6).integers(0, 200, ci.size)]
    M = build(sm, rp, ci, val1, n_cols, dict(layout="bands", updatable=1))
    info = M.info()
    assert info["has_xband"] == 4 and info["sell_codebook"] == 0
    val2 = new_values(ci.size, 2)
    F = build(sm, rp, ci, val2, n_cols, dict(layout="bands", updatable=1))
    M.set_values(to_dev(val2))
    assert_same_matrix(M, F, Operands(n_rows, n_cols), "bands:")


def test_auto_sell_takes_the_plain_form(sm):
    """AUTO on a small matrix with codebook values: the sliced ELL in its plain (d_val) form."""
    rp, ci, val1 = uniform_csr(5000, 1000, 5, seed=3)
    plain = build(sm, rp, ci, val1, 1000, None)
    assert plain.info()["sell_codebook"] == 1
    check_case(sm, rp, ci, 1000, dict(), expect=dict(sell_codebook=0))


# ------------------------------------------------------------------- transposed companion
def test_companion_follows_on_band2(sm):
    rp, ci = pattern(9000, 70001, 40)
    check_case(sm, rp, ci, 70001, dict(layout="band2"), expect=dict(has_xband=4), companion=True)


def test_source_order_through_the_c_abi(sm):
    """sm_set_values / sm_axpy_values(T, values in M's order, SM_VALUES_SOURCE) directly, T built
    from a matrix that is not updatable itself; SM_VALUES_SOURCE on a matrix that was not
    transposed is refused."""
    from sparsematrix_amd import _lib
    torch = torch_dev()
    L = _lib.load()
    rp, ci = pattern(5000, 1000, 5, long_row=True)
    nnz = ci.size
    val1, val2, delta = new_values(nnz, 1, False), new_values(nnz, 2), new_values(nnz, 3, False)
    opts = dict(layout="no_bands", sell_max_len=64)
    src = build(sm, rp, ci, val1, 1000, opts)            # not updatable
    T = src.transposed(opts=dict(opts, updatable=1))
    assert src.info()["updatable"] == 0 and T.info()["updatable"] == 1
    stream = torch.cuda.current_stream().cuda_stream
    d2, dd = to_dev(val2), to_dev(delta)
    assert L.sm_set_values(T._h, d2.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    ops_t = Operands(1000, 5000)
    F = build(sm, rp, ci, val2, 1000, dict(opts, updatable=1))
    assert_same_matrix(T, F.transposed(opts=opts), ops_t, "C ABI set, source order:")
    assert L.sm_axpy_values(T._h, AXPY_A, dd.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    F2 = build(sm, rp, ci, axpy_reference(val2, AXPY_A, delta), 1000, dict(opts, updatable=1))
    assert_same_matrix(T, F2.transposed(opts=opts), ops_t, "C ABI axpy, source order:")
    # own order on T: its own CSR order
    t_val = F.transposed(opts=opts).csr()[2]
    assert L.sm_set_values(T._h, to_dev(t_val).data_ptr(), _lib.SM_VALUES_OWN, stream) == 0
    assert_same_matrix(T, F.transposed(opts=opts), ops_t, "C ABI set, own order on T:")
    assert L.sm_set_values(F._h, d2.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == NOT_SUPPORTED
    assert L.sm_axpy_values(F._h, 1.0, dd.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == NOT_SUPPORTED
    torch.cuda.synchronize()


def test_unaligned_and_odd_sizes(sm):
    """An array 4 bytes past 16-byte alignment (the one-term-per-lane CSR kernel) and an nnz that
    is no multiple of 4 (the vector kernel's tail)."""
    torch = torch_dev()
    rp, ci = pattern(1000, 777, 3)
    rp, ci = rp.copy(), ci[:-1].copy()                 # drop the last term: nnz = 2999
    rp[-1] = ci.size
    assert ci.size % 4 == 3
    opts = dict(layout="no_bands", updatable=1)
    val1, val2 = new_values(ci.size, 1, False), new_values(ci.size, 2)
    ops = Operands(rp.size - 1, 777)
    F = build(sm, rp, ci, val2, 777, opts)
    for off in (0, 1):
        M = build(sm, rp, ci, val1, 777, opts)
        buf = torch.zeros(ci.size + 8, dtype=torch.float32, device="cuda")
        v = buf[off: off + ci.size]
        v.copy_(to_dev(val2))
        assert v.data_ptr() % 16 == 4 * off
        M.set_values(v)
        assert_same_matrix(M, F, ops, f"offset {off}:")


# ---------------------------------------------------------------------------- graph capture
def test_captured_axpy_then_spmv(sm):
    """One stream: axpy_values then spmv, captured (a serial capture: no parallel branches) and
    replayed three times, against three eager steps on a twin."""
    torch = torch_dev()
    rp, ci = pattern(9000, 70001, 40)
    nnz = ci.size
    opts = dict(layout="band2", updatable=1)
    val1, delta = new_values(nnz, 1, False), new_values(nnz, 3, False)
    M, twin = build(sm, rp, ci, val1, 70001, opts), build(sm, rp, ci, val1, 70001, opts)
    d = to_dev(delta)
    x = to_dev(np.random.default_rng(4).uniform(-1, 1, 70001).astype(np.float32))
    y, yt = torch.zeros(9000, device="cuda"), torch.zeros(9000, device="cuda")
    M.spmv(x, y, 1.0, 0.0)   # one eager product first (module load, scratch event)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.axpy_values(AXPY_A, d)
        M.spmv(x, y, 1.0, 0.0)
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        twin.axpy_values(AXPY_A, d)
        twin.spmv(x, yt, 1.0, 0.0)
        torch.cuda.synchronize()
        assert same_bits(y, yt)
    assert np.array_equal(bits(M.csr()[2]), bits(twin.csr()[2]))
    want = val1
    for _ in range(3):
        want = axpy_reference(want, AXPY_A, delta)
    assert np.array_equal(bits(M.csr()[2]), bits(want))


# -------------------------------------------------------------------------------- refusals
def test_refusals(sm):
    from sparsematrix_amd import _lib
    rp, ci, val = uniform_csr(300, 257, 6, seed=9)
    plain = build(sm, rp, ci, val, 257, None)
    v2 = to_dev(new_values(ci.size, 2))
    for call in (lambda: plain.set_values(v2), lambda: plain.axpy_values(0.5, v2)):
        with pytest.raises(_lib.SparseMatrixError) as e:
            call()
        assert e.value.status == NOT_SUPPORTED
    assert np.array_equal(bits(plain.csr()[2]), bits(val))
    upd = build(sm, rp, ci, val, 257, dict(updatable=1))
    with pytest.raises(_lib.SparseMatrixError) as e:
        upd.build_ref_stream()
    assert e.value.status == NOT_SUPPORTED
    assert upd.info()["has_ref_stream"] == 0
    with pytest.raises(_lib.SparseMatrixError) as e:   # a null array with nnz > 0
        _lib.check(_lib.load().sm_set_values(upd._h, None, 0, None), "sm_set_values")
    assert e.value.status == 1
    with pytest.raises(ValueError):
        upd.set_values(v2[:-1])
    # a dense-index matrix: its values are its codebook
    index = np.full((16, 8), 255, np.uint8)
    index[::3, ::2] = 1
    table = np.arange(1, 9, dtype=np.float32)
    dense = sm.SparseMatrix(index, 16, 8, 8, table, 8)
    with pytest.raises(_lib.SparseMatrixError) as e:
        dense.transposed(opts=dict(updatable=1))
    assert e.value.status == NOT_SUPPORTED
    assert dense.transposed().info()["updatable"] == 0


def test_empty_matrix(sm):
    torch = torch_dev()
    rp = np.zeros(6, np.int32)
    empty = np.zeros(0, np.int32)
    M = build(sm, rp, empty, np.zeros(0, np.float32), 7, dict(updatable=1))
    M.set_values(torch.zeros(0, device="cuda"))
    M.axpy_values(1.5, torch.zeros(0, device="cuda"))
    T = M.T
    M.set_values(torch.zeros(0, device="cuda"))   # the companion in source order: SM_OK too
    assert T.info()["updatable"] == 1 and M.info()["nnz"] == 0


def test_default_is_unchanged(sm):
    rp, ci, val = uniform_csr(5000, 1000, 5, seed=3)
    a = build(sm, rp, ci, val, 1000, None)
    b = build(sm, rp, ci, val, 1000, dict(updatable=0))
    assert a.info() == b.info() and a.info()["updatable"] == 0
    assert a.layout_digest() == b.layout_digest()


# -------------------------------------------------------------------------------- autograd
def test_sgd_steps_keep_leaf_and_matrix_equal(sm):
    torch = torch_dev()
    from sparsematrix_amd import autograd
    n_rows, n_cols, N, lr = 5000, 1000, 4, 0.05
    rp, ci = pattern(n_rows, n_cols, 5)
    val0 = new_values(ci.size, 1, special=False)
    m = build(sm, rp, ci, val0, n_cols, dict(updatable=1))
    val = m.csr_device()[2].requires_grad_()
    rng = np.random.default_rng(8)
    ops = Operands(n_rows, n_cols)
    for step in range(3):
        X = to_dev(rng.uniform(-1, 1, (n_cols, N)).astype(np.float32))
        G = to_dev(rng.uniform(-1, 1, (n_rows, N)).astype(np.float32))
        Y = autograd.apply(m, X, alpha=1.0, values=val)
        Y.backward(G)
        m.axpy_values(-lr, val.grad)
        with torch.no_grad():
            val.add_(val.grad * (-lr))   # the same two roundings
            val.grad = None
        assert same_bits(m.csr_device()[2], val.detach()), f"step {step}: leaf != matrix"
        fresh = build(sm, rp, ci, to_host(val.detach()), n_cols, dict(updatable=1))
        Ym, Yf = ops.Y0[N].clone(), ops.Y0[N].clone()
        m.spmm(ops.X[N], Ym, 1.3, 0.7)
        fresh.spmm(ops.X[N], Yf, 1.3, 0.7)
        assert same_bits(Ym, Yf), f"step {step}: spmm"
    assert not np.array_equal(bits(to_host(val.detach())), bits(val0))
