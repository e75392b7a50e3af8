"""The quantiser on the GPU: sm_quantize_assign, sm_quantize_update, sm_create_quantized and the
device table constructor sm_create_from_csr_ids_device.

Everything is compared bit for bit with quantize_ref, the numpy restatement of the header's rules
(the assignment rule, the chunked double sums, the linear start, the Lloyd loop), and the device
constructor with the host one (from_csr_ids on numpy arrays).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_specs
import quantize_ref as qr
import table_ref
from gpu_util import bits, to_dev, to_host, torch_dev, uniform_csr

pytestmark = pytest.mark.gpu

INVALID_MATRIX = 6
GUARD = 64


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


# ------------------------------------------------------------------------------- inputs
PATTERNS = {"300x257": (300, 257, 6, 1),            # one partial chunk, nnz = 1799 (3 mod 4)
            "1000x777": (1000, 777, 5, 2),          # three chunks, nnz = 4998 (2 mod 4)
            "1000x777_whole": (1000, 777, 5, 0)}    # nnz = 5000 (0 mod 4)


def pattern(n_rows, n_cols, per, drop):
    """uniform_csr's pattern with the last `drop` terms of the last row removed."""
    rp, ci, _ = uniform_csr(n_rows, n_cols, per, seed=7)
    rp = rp.copy()
    rp[-1] -= drop
    return rp, ci[:ci.size - drop]


def tables():
    rng = np.random.default_rng(31)
    t7 = rng.uniform(-1, 1, 7).astype(np.float32)
    t7[5] = t7[1]                                   # unsorted, with a duplicate
    tn = rng.uniform(-1, 1, 9).astype(np.float32)
    tn[0] = np.nan                                  # a NaN entry (and id 0 is what a NaN value gets)
    tn[4], tn[7] = -0.0, 0.0
    return {"T1": np.array([0.25], np.float32), "T2": np.array([0.5, -0.5], np.float32), "T7_dup": t7,
            "T255": rng.uniform(-1, 1, 255).astype(np.float32), "nan_entry": tn}


def values_for(nnz, table, seed=32):
    """Uniform values in (-1, 1) with the hand-made cases spliced in at the front, the back and
    across the first chunk boundary: every entry itself, the midpoints of neighbouring candidates
    (ties), values below and above every entry, both zeros, NaN and the infinities."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, nnz).astype(np.float32)
    cand = np.sort(table[~np.isnan(table)])
    mids = ((cand[:-1].astype(np.float64) + cand[1:]) / 2).astype(np.float32)
    special = np.concatenate([cand, mids, [-3.0, 3.0, 0.0, -0.0, np.nan, np.inf, -np.inf]]).astype(np.float32)
    special = special[:min(special.size, nnz // 3)]
    v[:special.size] = special
    v[nnz - special.size:] = special[::-1]
    if nnz > 2048 + special.size:
        v[2048 - special.size // 2: 2048 - special.size // 2 + special.size] = special
    return v


def guarded_ids(nnz, off):
    """(view, parent): nnz uint8 at `off` bytes past 4-byte alignment, GUARD bytes of 0xA5 around."""
    torch = torch_dev()
    parent = torch.full((GUARD + off + nnz + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = parent[GUARD + off: GUARD + off + nnz]
    assert view.data_ptr() % 4 == off
    return view, parent


def assert_ids_guards(parent, off, nnz):
    w = to_host(parent)
    assert (w[:GUARD + off] == 0xA5).all() and (w[GUARD + off + nnz:] == 0xA5).all(), "guard bytes written"


def status_of(call):
    from sparsematrix_amd._lib import SparseMatrixError
    with pytest.raises(SparseMatrixError) as ei:
        call()
    return ei.value.status


# ------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("tab", ["T1", "T2", "T7_dup", "T255", "nan_entry"])
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_assign(sm, pat, tab):
    n_rows, n_cols, per, drop = PATTERNS[pat]
    rp, ci = pattern(n_rows, n_cols, per, drop)
    table = tables()[tab]
    va = values_for(ci.size, table)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    want = qr.assign(va, table)
    d_table = to_dev(table)
    assert np.array_equal(to_host(M.quantize_assign(d_table)), want)
    L = sm._lib.load()
    for off in (0, 1, 3):      # packed 32-bit stores, and bytewise ones
        view, parent = guarded_ids(ci.size, off)
        sm._lib.check(L.sm_quantize_assign(M._h, d_table.data_ptr(), table.size, view.data_ptr(), None), "assign")
        assert np.array_equal(to_host(view), want), f"ids at offset {off}"
        assert_ids_guards(parent, off, ci.size)


# ------------------------------------------------------------------------------- update
UPDATE_PATTERNS = {"300x257": (300, 257, 6, 1, False), "1000x777": (1000, 777, 5, 2, False),
                   "5000x1000_long": (5000, 1000, 5, 0, True)}   # 13 chunks, a 1000-term row


def update_pattern(name):
    n_rows, n_cols, per, drop, long_row = UPDATE_PATTERNS[name]
    rp, ci = pattern(n_rows, n_cols, per, drop)
    if long_row:   # row n_rows // 2 holds every column
        r = n_rows // 2
        a, b = int(rp[r]), int(rp[r + 1])
        ci = np.concatenate([ci[:a], np.arange(n_cols, dtype=np.int32), ci[b:]])
        rp = rp.astype(np.int64)
        rp[r + 1:] += n_cols - (b - a)
        rp = rp.astype(np.int32)
    return rp, ci, n_cols


def id_cases(nnz):
    rng = np.random.default_rng(23)
    u = lambda T, seed: np.random.default_rng(seed).integers(0, T, nnz).astype(np.uint8)
    cases = {"T1": (1, u(1, 1)), "T7": (7, u(7, 2)), "T255": (255, u(255, 3)),
             "id3_unused": (7, np.array([0, 1, 2, 4, 5, 6], np.uint8)[rng.integers(0, 6, nnz)])}
    run = u(7, 4)
    if nnz > 2100:
        run[2000:2100] = 2   # a run of one id across the first chunk boundary
    cases["run_over_boundary"] = (7, run)
    return cases


@pytest.mark.parametrize("ids_case", ["T1", "T7", "T255", "id3_unused", "run_over_boundary"])
@pytest.mark.parametrize("pat", list(UPDATE_PATTERNS))
def test_update(sm, pat, ids_case):
    rp, ci, n_cols = update_pattern(pat)
    rng = np.random.default_rng(41)
    va = rng.uniform(-1, 1, ci.size).astype(np.float32)
    T, ids = id_cases(ci.size)[ids_case]
    old = rng.uniform(-1, 1, T).astype(np.float32)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    want_tab, want_n, want_sse = qr.update(va, ids, old)
    d_tab = to_dev(old.copy())
    counts, sse = M.quantize_update(to_dev(ids), d_tab)
    assert np.array_equal(bits(to_host(d_tab)), bits(want_tab)), "table bits"
    assert np.array_equal(to_host(counts), want_n), "counts"
    assert to_host(sse).view(np.uint64)[0] == np.float64(want_sse).view(np.uint64), "sse bits"
    if ids_case == "id3_unused":
        assert want_n[3] == 0 and bits(to_host(d_tab))[3] == bits(old)[3]
    # ids at an odd address, counts and sse not wanted
    view, parent = guarded_ids(ci.size, 1)
    view.copy_(to_dev(ids))
    d_tab2 = to_dev(old.copy())
    L = sm._lib.load()
    sm._lib.check(L.sm_quantize_update(M._h, view.data_ptr(), T, d_tab2.data_ptr(), None, None, None), "update")
    assert np.array_equal(bits(to_host(d_tab2)), bits(want_tab))


def test_update_bad_id_and_empty(sm):
    rp, ci, n_cols = update_pattern("1000x777")
    va = np.random.default_rng(42).uniform(-1, 1, ci.size).astype(np.float32)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    ids = np.zeros(ci.size, np.uint8)
    ids[3001] = 7
    assert status_of(lambda: M.quantize_update(to_dev(ids), to_dev(np.zeros(7, np.float32)))) == INVALID_MATRIX
    # no term: the table unchanged, counts 0, sse 0.0, and assign launches nothing
    E = sm.SparseMatrix.from_csr(np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5)
    old = np.array([1.5, -2.0], np.float32)
    d_tab = to_dev(old.copy())
    torch = torch_dev()
    counts, sse = E.quantize_update(torch.empty(0, dtype=torch.uint8, device="cuda"), d_tab)
    assert np.array_equal(bits(to_host(d_tab)), bits(old)) and not to_host(counts).any() and to_host(sse)[0] == 0.0
    assert E.quantize_assign(d_tab).numel() == 0
    Q = E.quantized(table_size=3, iters=2)
    assert Q.info()["table_size"] == 3 and Q.nnz == 0 and to_host(Q.table_device()).tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------- quantized
@functools.lru_cache(maxsize=None)
def plain_lloyd(T, iters):
    c = layout_specs._plain()
    return qr.lloyd(c.va, T, iters)


@pytest.fixture(scope="module")
def plain_src(sm):
    c = layout_specs._plain()
    return sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts={"updatable": 1})


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("T", [2, 16, 255])
def test_quantized_equals_the_restated_loop(sm, plain_src, T, iters):
    c = layout_specs._plain()
    want_ids, want_tab = plain_lloyd(T, iters)
    Q = plain_src.quantized(table_size=T, iters=iters)
    assert np.array_equal(bits(to_host(Q.table_device())), bits(want_tab)), "table"
    assert np.array_equal(to_host(Q.term_ids_device()), want_ids), "ids"
    q_rp, q_ci, q_va = Q.csr()
    assert np.array_equal(q_rp, c.rp) and np.array_equal(q_ci, c.ci)
    assert np.array_equal(bits(q_va), bits(want_tab[want_ids])), "CSR values = table[ids]"
    assert Q.info()["table_size"] == T and Q.info()["updatable"] == 0
    assert np.array_equal(bits(plain_src.csr()[2]), bits(c.va)), "the source is untouched"


def test_quantized_bands_and_products(sm):
    """The gain the feature buys: the updatable source holds band2's 8-byte entries, the quantised
    matrix cband's 4-byte words, and its products are those of the host-built table matrix."""
    c = layout_specs._plain()
    opts = {"layout": "bands"}
    src = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=dict(opts, updatable=1))
    assert src.info()["has_xband"] == 4
    Q = src.quantized(table_size=255, iters=3, opts=opts)
    assert Q.info()["has_xband"] == 5
    ids, tab = plain_lloyd(255, 3)
    H = sm.SparseMatrix.from_csr_ids(c.rp, c.ci, ids, tab, c.n_cols, opts=opts)
    x, y0 = to_dev(c.x), to_dev(c.y0)
    yq, yh = y0.clone(), y0.clone()
    Q.spmv(x, yq, 1.3, 0.7)
    H.spmv(x, yh, 1.3, 0.7)
    assert table_ref.same_bits(yq, yh)
    assert Q == H and Q.layout_digest() == H.layout_digest()


def test_quantized_from_a_given_start(sm, plain_src):
    c = layout_specs._plain()
    init = np.random.default_rng(51).uniform(-0.8, 0.8, 16).astype(np.float32)
    init[3] = init[9]                 # a duplicate start entry: id 9 is empty in the first step and keeps its entry
    first = qr.assign(c.va, init)
    assert not np.any(first == 9) and bits(qr.update(c.va, first, init)[0])[9] == bits(init)[9]
    want_ids, want_tab = qr.lloyd(c.va, 16, 2, init=init)
    Q = plain_src.quantized(table_size=16, iters=2, init=to_dev(init))
    assert np.array_equal(bits(to_host(Q.table_device())), bits(want_tab))
    assert np.array_equal(to_host(Q.term_ids_device()), want_ids)


def test_quantized_refuses_a_non_finite_value(sm):
    c = layout_specs._plain()
    va = c.va.copy()
    va[12345] = np.inf
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, va, c.n_cols)
    assert status_of(lambda: M.quantized(table_size=16, iters=1)) == INVALID_MATRIX
    assert status_of(lambda: M.quantized(table_size=16, iters=1, init=to_dev(np.zeros(16, np.float32)))) \
        == INVALID_MATRIX


def test_quantized_table_updatable_takes_axpy_table(sm, plain_src):
    c = layout_specs._plain()
    opts = {"table_updatable": 1}
    ids, tab = plain_lloyd(16, 3)
    Q = plain_src.quantized(table_size=16, iters=3, opts=opts)
    assert Q.info()["table_updatable"] == 1
    delta = np.random.default_rng(52).uniform(-1, 1, 16).astype(np.float32)
    Q.axpy_table(-0.37, to_dev(delta))
    new_tab = table_ref.axpy_reference(tab, -0.37, delta)
    F = sm.SparseMatrix.from_csr_ids(c.rp, c.ci, ids, new_tab, c.n_cols, opts=opts)
    table_ref.assert_same_matrix(Q, F, table_ref.Operands(c.n_rows, c.n_cols), "quantized + axpy_table")


# ------------------------------------------------------------------------------- device constructor
@functools.lru_cache(maxsize=None)
def base_ids():
    """(ids, table) of layout_specs._base(): its values come from a 200-entry table."""
    c = layout_specs._base()
    table = layout_specs._table(layout_specs.N_COLS)
    tb = bits(table)
    assert np.unique(tb).size == tb.size
    order = np.argsort(tb)
    ids = order[np.searchsorted(tb[order], bits(c.va))].astype(np.uint8)
    assert np.array_equal(bits(table[ids]), bits(c.va))
    return ids, table


@pytest.mark.parametrize("opts", [{}, {"layout": "cband", "band_slabs": 3}, {"layout": "no_bands"},
                                  {"table_updatable": 1}],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_device_constructor_equals_the_host_one(sm, opts):
    c = layout_specs._base()
    ids, table = base_ids()
    H = sm.SparseMatrix.from_csr_ids(c.rp, c.ci, ids, table, c.n_cols, opts=opts)
    d_rp, d_ci = to_dev(c.rp), to_dev(c.ci)
    D = sm.SparseMatrix.from_csr_ids(d_rp, d_ci, to_dev(ids), to_dev(table), c.n_cols, opts=opts)
    assert D == H and D.layout_digest() == H.layout_digest()
    hi, di = H.info(), D.info()
    hi.pop("device_bytes"), di.pop("device_bytes")
    assert di == hi
    assert np.array_equal(bits(to_host(D.table_device())), bits(table))
    assert np.array_equal(to_host(D.term_ids_device()), ids)
    assert np.array_equal(bits(D.csr()[2]), bits(c.va))
    x, y0 = to_dev(c.x), to_dev(c.y0)
    yd, yh = y0.clone(), y0.clone()
    D.spmv(x, yd, 1.3, 0.7)
    H.spmv(x, yh, 1.3, 0.7)
    assert table_ref.same_bits(yd, yh), "spmv"
    rng = np.random.default_rng(61)
    X = to_dev(rng.uniform(-1, 1, (c.n_cols, 32)).astype(np.float32))
    Y0 = to_dev(rng.uniform(-1, 1, (c.n_rows, 32)).astype(np.float32))
    Yd, Yh = Y0.clone(), Y0.clone()
    D.spmm(X, Yd, 1.3, 0.7)
    H.spmm(X, Yh, 1.3, 0.7)
    assert table_ref.same_bits(Yd, Yh), "spmm"
    if opts.get("table_updatable"):
        assert D.built_on_device() == 0          # the host builders take the given ids and table
    else:
        V = sm.SparseMatrix.from_csr(d_rp, d_ci, to_dev(c.va), c.n_cols, opts=opts)
        assert D.built_on_device() == V.built_on_device()


def test_device_constructor_refuses_a_bad_id(sm):
    c = layout_specs._base()
    ids, table = base_ids()
    bad = ids.copy()
    bad[70001] = 200                             # T = 200: the first id outside the table
    call = lambda: sm.SparseMatrix.from_csr_ids(to_dev(c.rp), to_dev(c.ci), to_dev(bad), to_dev(table), c.n_cols)
    assert status_of(call) == INVALID_MATRIX
