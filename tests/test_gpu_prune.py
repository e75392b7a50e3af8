"""Pruning on the GPU: sm_prune_mask, sm_create_masked, sm_create_pruned and
sm_copy_source_terms_device.

Every mask is compared byte for byte with prune_ref.mask, the numpy restatement of the header's
rule on the values' bits, and every pruned matrix with SparseMatrix.from_csr (from_csr_ids for a
table source) of prune_ref.compact's arrays: ==, digests, info, products, bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_specs
import prune_ref as pr
import quantize_ref as qr
import table_ref
from gpu_util import assert_terms_close, bits, messy_csr, skewed_csr, to_dev, to_host, torch_dev, uniform_csr

pytestmark = pytest.mark.gpu

NOT_SUPPORTED = 4
GUARD = 64
CHUNK = 2048


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


@functools.lru_cache(maxsize=None)
def pattern(name):
    """uniform_csr's pattern with the last `drop` terms of the last row removed."""
    n_rows, n_cols, per, drop = PATTERNS[name]
    rp, ci, _ = uniform_csr(n_rows, n_cols, per, seed=7)
    rp = rp.copy()
    rp[-1] -= drop
    return rp, ci[:ci.size - drop], n_cols


SPECIAL = np.array([0.5, -0.5, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 0.5, -0.0, np.nan],
                   np.float32)


def from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


def value_set(name, nnz):
    rng = np.random.default_rng(71)
    i = np.arange(nnz, dtype=np.uint64)
    sign = (rng.integers(0, 2, nnz).astype(np.uint32) << np.uint32(31))
    if name == "uniform":
        return rng.uniform(-1, 1, nnz).astype(np.float32)
    if name == "all_half":                         # every term ties
        return from_bits(np.uint32(0x3F000000) | sign)
    if name == "low_byte":                         # only the last radix pass tells the keys apart
        return from_bits((np.uint32(0x3F000000) + ((i * 37) % 256).astype(np.uint32)) | sign)
    if name == "mid_byte":
        return from_bits((np.uint32(0x3F000000) + (((i * 101) % 256).astype(np.uint32) << np.uint32(8))) | sign)
    if name == "top_byte":                         # only the first pass: 0, then 2^(2b - 127), b = 1..127
        return from_bits((((i * 29) % 128).astype(np.uint32) << np.uint32(24)) | sign)
    if name == "powers_of_two":                    # the whole exponent range, the subnormal ones included
        s = (i * 53) % 277                         # 0..22: 2^(s - 149); 23..276: exponent field s - 22
        key = np.where(s < 23, np.uint64(1) << s, (s - np.uint64(22)) << np.uint64(23)).astype(np.uint32)
        return from_bits(key | sign)
    if name == "specials":                         # at the front, the back and across the chunk boundary
        v = rng.uniform(-1, 1, nnz).astype(np.float32)
        n = SPECIAL.size
        v[:n] = SPECIAL
        v[nnz - n:] = SPECIAL[::-1]
        if nnz > CHUNK + n:
            v[CHUNK - n // 2: CHUNK - n // 2 + n] = SPECIAL
        return v
    raise KeyError(name)


VALUE_SETS = ("uniform", "all_half", "low_byte", "mid_byte", "top_byte", "powers_of_two", "specials")


def guarded_keep(nnz, off):
    """(view, parent): nnz uint8 at `off` bytes past 4-byte alignment, GUARD bytes of 0xA5 around."""
    torch = torch_dev()
    parent = torch.full((GUARD + off + nnz + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = parent[GUARD + off: GUARD + off + nnz]
    assert view.data_ptr() % 4 == off
    return view, parent


def assert_keep_guards(parent, off, nnz):
    w = to_host(parent)
    assert (w[:GUARD + off] == 0xA5).all() and (w[GUARD + off + nnz:] == 0xA5).all(), "guard bytes written"


def status_of(call):
    from sparsematrix_amd._lib import SparseMatrixError
    with pytest.raises(SparseMatrixError) as ei:
        call()
    return ei.value.status


def same_mask(got, want, what):
    got = to_host(got)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} mask bytes differ, first at {bad[:6].tolist()}"


# ------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("values", VALUE_SETS)
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_global_mask(sm, pat, values):
    rp, ci, n_cols = pattern(pat)
    nnz = ci.size
    va = value_set(values, nnz)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    counts = [0, 1, 3, nnz // 2, nnz - 1, nnz, nnz + 7]
    if nnz > CHUNK + 1:
        counts.append(CHUNK + 1)                   # a tie group straddling the chunk boundary
    for count in counts:
        want = pr.mask(rp, va, pr.GLOBAL_TOPK, count)
        same_mask(M.prune_mask(keep=count), want, f"keep={count}")
        if values == "all_half":
            assert np.array_equal(np.flatnonzero(want), np.arange(min(count, nnz)))   # exactly the first terms
    L = sm._lib.load()
    count = nnz // 2
    want = pr.mask(rp, va, pr.GLOBAL_TOPK, count)
    for off in (0, 1, 3):                          # packed 32-bit stores, and bytewise ones
        view, parent = guarded_keep(nnz, off)
        kept = C.c_int64(-1)
        sm._lib.check(L.sm_prune_mask(M._h, pr.GLOBAL_TOPK, count, 0.0, view.data_ptr(), C.byref(kept), None), "mask")
        same_mask(view, want, f"keep at offset {off}")
        assert kept.value == int(want.sum()) == count
        assert_keep_guards(parent, off, nnz)


@pytest.mark.parametrize("values", ["uniform", "specials", "all_half"])
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_threshold_mask(sm, pat, values):
    rp, ci, n_cols = pattern(pat)
    nnz = ci.size
    va = value_set(values, nnz)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    stored = np.abs(va[nnz // 3 + 40])             # a stored magnitude: kept at it, dropped just above
    assert np.isfinite(stored) and stored > 0
    L = sm._lib.load()
    for thr in (stored, np.nextafter(stored, np.float32(0)), np.nextafter(stored, np.float32(2)), 0.0, -0.0,
                np.inf, np.float32(1e-45)):
        want = pr.mask(rp, va, pr.THRESHOLD, threshold=thr)
        same_mask(M.prune_mask(threshold=float(thr)), want, f"threshold={thr!r}")
        for off in (0, 1, 3):
            view, parent = guarded_keep(nnz, off)
            kept = C.c_int64(-1)
            sm._lib.check(L.sm_prune_mask(M._h, pr.THRESHOLD, -9, float(thr), view.data_ptr(), C.byref(kept), None),
                          "mask")                  # count is ignored
            same_mask(view, want, f"threshold={thr!r} at offset {off}")
            assert kept.value == int(want.sum())
            assert_keep_guards(parent, off, nnz)
    assert pr.mask(rp, va, pr.THRESHOLD, threshold=0.0).all()
    at, above = pr.mask(rp, va, pr.THRESHOLD, threshold=stored), pr.mask(rp, va, pr.THRESHOLD,
                                                                         threshold=np.nextafter(stored, np.float32(2)))
    assert at[nnz // 3 + 40] == 1 and above[nnz // 3 + 40] == 0


ROW_LENGTHS = np.array([0, 1, 2, 63, 64, 65, 300, 0, 64, 5000, 65, 1, 63, 129, 2, 0], np.int64)
ROW_TABLE = np.array([0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 0.125], np.float32)


@functools.lru_cache(maxsize=None)
def row_case(values):
    """Rows of 0, 1, 2, 63, 64, 65 and 300 terms and one of 5000 (the workgroup path over twenty
    steps), in an order that puts short and long rows side by side."""
    rp, ci, va = skewed_csr(ROW_LENGTHS.size, 6000, ROW_LENGTHS, seed=81)
    rng = np.random.default_rng(82)
    if values == "ties7":                          # heavy ties: the rank among equals decides everywhere
        va = ROW_TABLE[rng.integers(0, 7, va.size)]
    elif values == "low_byte":                     # the row select's last pass decides
        va = value_set("low_byte", va.size)
    elif values == "specials":
        va = value_set("specials", va.size)
    return rp, ci, np.ascontiguousarray(va, np.float32)


@pytest.mark.parametrize("values", ["ties7", "uniform", "low_byte", "specials"])
def test_row_mask(sm, values):
    rp, ci, va = row_case(values)
    M = sm.SparseMatrix.from_csr(rp, ci, va, 6000)
    L = sm._lib.load()
    for count in (0, 1, 2, 63, 64, 65, 10 ** 9):
        want = pr.mask(rp, va, pr.ROW_TOPK, count)
        same_mask(M.prune_mask(per_row=count), want, f"per_row={count}")
        view, parent = guarded_keep(va.size, 1)
        kept = C.c_int64(-1)
        sm._lib.check(L.sm_prune_mask(M._h, pr.ROW_TOPK, count, 0.0, view.data_ptr(), C.byref(kept), None), "mask")
        same_mask(view, want, f"per_row={count} at offset 1")
        assert kept.value == int(want.sum()) == int(np.minimum(ROW_LENGTHS, count).sum())
        assert_keep_guards(parent, 1, va.size)


def test_row_mask_many_rows(sm):
    """More rows than one wave stride of a small grid, every row short: the 1000 x 777 pattern."""
    rp, ci, n_cols = pattern("1000x777")
    va = ROW_TABLE[np.random.default_rng(83).integers(0, 7, ci.size)]
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    for count in (1, 4, 5):
        same_mask(M.prune_mask(per_row=count), pr.mask(rp, va, pr.ROW_TOPK, count), f"per_row={count}")


def test_python_argument_checks(sm):
    rp, ci, n_cols = pattern("300x257")
    M = sm.SparseMatrix.from_csr(rp, ci, value_set("uniform", ci.size), n_cols)
    torch = torch_dev()
    for kw in ({}, {"keep": 1, "per_row": 1}, {"keep": 1, "threshold": 0.5}):
        with pytest.raises(ValueError):
            M.prune_mask(**kw)
        with pytest.raises(ValueError):
            M.pruned(**kw)
    with pytest.raises(ValueError):
        M.masked(torch.ones(ci.size - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        M.masked(torch.ones(2 * ci.size, dtype=torch.uint8, device="cuda")[::2])
    with pytest.raises(TypeError):
        M.masked(torch.ones(ci.size, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        M.masked(np.ones(ci.size, np.uint8))
    assert status_of(lambda: M.prune_mask(keep=-1)) == 1 and status_of(lambda: M.pruned(threshold=-1.0)) == 1


# ------------------------------------------------------------------------------- the constructor
SPMV_ALGOS = ("auto", "parity", "stream", "sell", "merge")


def same_products(P, F, ops, tag):
    """spmv under five algorithms, spmm at N = 32 and sddmm of P and F, bit for bit."""
    for algo in SPMV_ALGOS:
        yp, yf = ops.y0.clone(), ops.y0.clone()
        P.spmv(ops.x, yp, 1.3, 0.7, algo=algo)
        F.spmv(ops.x, yf, 1.3, 0.7, algo=algo)
        assert table_ref.same_bits(yp, yf), f"{tag}: spmv {algo}"
    Yp, Yf = ops.Y0[32].clone(), ops.Y0[32].clone()
    P.spmm(ops.X[32], Yp, 1.3, 0.7)
    F.spmm(ops.X[32], Yf, 1.3, 0.7)
    assert table_ref.same_bits(Yp, Yf), f"{tag}: spmm"
    assert table_ref.same_bits(P.sddmm(ops.G4, ops.X[4]), F.sddmm(ops.G4, ops.X[4])), f"{tag}: sddmm"


def same_as_fresh(sm, P, F, keep, ops, tag, D=None):
    """P (pruned on the device) is F (built from the compacted arrays): CSR, ==, digests, info but
    for device_bytes, products; its source map is the kept terms' indices; with D (the compacted
    arrays ingested from device tensors) also where the layouts were built."""
    p_csr, f_csr = P.csr(), F.csr()
    assert np.array_equal(p_csr[0], f_csr[0]) and np.array_equal(p_csr[1], f_csr[1]), tag + ": pattern"
    assert np.array_equal(bits(p_csr[2]), bits(f_csr[2])), tag + ": CSR values (bits)"
    assert P == F, tag + ": =="
    assert P.layout_digest() == F.layout_digest(), tag + ": layout digest"
    pi, fi = P.info(), F.info()
    assert pi.pop("device_bytes") >= 4 * pi["nnz"] and fi.pop("device_bytes") > 0
    assert pi == fi, tag + ": info"
    if D is not None:
        assert P.built_on_device() == D.built_on_device(), tag + ": built_on_device"
    src = to_host(P.source_terms_device())
    assert src.dtype == np.int32 and np.array_equal(src, np.flatnonzero(keep)), tag + ": source terms"
    same_products(P, F, ops, tag)


def hand_mask(rp, seed=91):
    """A random mask that empties some rows entirely, the first and the last among them."""
    rng = np.random.default_rng(seed)
    nnz = int(rp[-1])
    keep = (rng.uniform(0, 1, nnz) < 0.45).astype(np.uint8)
    keep[keep != 0] = rng.integers(1, 256, int((keep != 0).sum()))   # any non-zero byte keeps
    n_rows = rp.size - 1
    for r in (0, 1, 17, n_rows // 2, n_rows - 1):
        keep[rp[r]:rp[r + 1]] = 0
    return keep


MODES = ("global", "row", "threshold", "mask")


def prune_by(M, rp, va, mode, opts):
    """(P, keep): the pruned matrix by `mode` and the restated mask."""
    nnz = va.size
    if mode == "global":
        return M.pruned(keep=nnz // 2, opts=opts), pr.mask(rp, va, pr.GLOBAL_TOPK, nnz // 2)
    if mode == "row":
        return M.pruned(per_row=3, opts=opts), pr.mask(rp, va, pr.ROW_TOPK, 3)
    if mode == "threshold":
        return M.pruned(threshold=0.5, opts=opts), pr.mask(rp, va, pr.THRESHOLD, threshold=0.5)
    keep = hand_mask(rp)
    return M.masked(to_dev(keep), opts=opts), keep


@pytest.mark.parametrize("opts", [{}, {"layout": "no_bands"}], ids=["defaults", "no_bands"])
@pytest.mark.parametrize("mode", MODES)
def test_pruned_equals_a_fresh_build(sm, mode, opts):
    rp, ci, n_cols = pattern("1000x777")
    va = value_set("uniform", ci.size)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    P, keep = prune_by(M, rp, va, mode, opts)
    n_rp, n_ci, n_va, _, _ = pr.compact(rp, ci, va, keep)
    F = sm.SparseMatrix.from_csr(n_rp, n_ci, n_va, n_cols, opts=opts)
    D = sm.SparseMatrix.from_csr(to_dev(n_rp), to_dev(n_ci), to_dev(n_va), n_cols, opts=opts)
    same_as_fresh(sm, P, F, keep, table_ref.Operands(rp.size - 1, n_cols), f"{mode} {opts}", D)
    assert np.array_equal(bits(M.csr()[2]), bits(va)), "the source is untouched"


@pytest.mark.parametrize("layout,mode", [("cband", "row"), ("cband", "mask"), ("band2", "global"), ("band2", "mask")])
def test_pruned_bands(sm, layout, mode):
    """A strictly ascending source wide enough for bands (layout_specs' base case: 20011 x 120001,
    values from a 200-entry table), the balanced bands forced on the pruned matrix."""
    c = layout_specs._base()
    opts = {"layout": layout, "band_slabs": 1}
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts={"layout": "no_bands"})
    P, keep = prune_by(M, c.rp, c.va, mode, opts)
    assert P.info()["has_xband"] == layout_specs.BAND_CODE[layout]
    n_rp, n_ci, n_va, _, _ = pr.compact(c.rp, c.ci, c.va, keep)
    F = sm.SparseMatrix.from_csr(n_rp, n_ci, n_va, c.n_cols, opts=opts)
    D = sm.SparseMatrix.from_csr(to_dev(n_rp), to_dev(n_ci), to_dev(n_va), c.n_cols, opts=opts)
    same_as_fresh(sm, P, F, keep, table_ref.Operands(c.n_rows, c.n_cols), f"{layout} {mode}", D)


def test_everything_and_nothing(sm):
    rp, ci, n_cols = pattern("300x257")
    va = value_set("specials", ci.size)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    for P in (M.pruned(keep=ci.size), M.pruned(keep=ci.size + 5), M.pruned(per_row=6), M.pruned(threshold=0.0)):
        assert P == M and P.layout_digest() == M.layout_digest()
        assert np.array_equal(to_host(P.source_terms_device()), np.arange(ci.size))
    torch = torch_dev()
    n_rows = rp.size - 1
    empty_src = sm.SparseMatrix.from_csr(np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32),
                                         np.zeros(0, np.float32), n_cols)
    assert empty_src.prune_mask(keep=3).numel() == 0 and empty_src.prune_mask(per_row=1).numel() == 0
    empties = [M.pruned(keep=0), M.pruned(per_row=0), M.masked(torch.zeros(ci.size, dtype=torch.uint8, device="cuda")),
               empty_src.pruned(keep=4), empty_src.pruned(threshold=0.0),
               empty_src.masked(torch.zeros(0, dtype=torch.uint8, device="cuda"))]
    rng = np.random.default_rng(92)
    x, y0 = rng.uniform(-1, 1, n_cols).astype(np.float32), rng.uniform(-1, 1, n_rows).astype(np.float32)
    for E in empties:
        assert E.nnz == 0 and E == empty_src and E.source_terms_device().numel() == 0
        assert not E.csr()[0].any()
        y = to_dev(y0)
        E.spmv(to_dev(x), y, 1.3, 0.7)
        assert np.array_equal(bits(to_host(y)), bits(y0 * np.float32(0.7))), "beta only"


# ------------------------------------------------------------------------------- sources
def test_table_source(sm):
    rp, ci, n_cols = pattern("1000x777")
    rng = np.random.default_rng(93)
    table = rng.uniform(-1, 1, 7).astype(np.float32)
    table[5] = table[2]                            # a duplicate entry: the ids, not the values, tell them apart
    ids = rng.integers(0, 7, ci.size).astype(np.uint8)
    va = table[ids]
    ops = table_ref.Operands(rp.size - 1, n_cols)
    for opts in ({}, {"table_updatable": 1}):
        M = sm.SparseMatrix.from_csr_ids(rp, ci, ids, table, n_cols, opts=opts)
        for mode in ("global", "mask"):
            P, keep = prune_by(M, rp, va, mode, opts)
            n_rp, n_ci, _, n_ids, src = pr.compact(rp, ci, va, keep, ids)
            assert P.info()["table_size"] == 7 and P.info()["table_updatable"] == opts.get("table_updatable", 0)
            assert np.array_equal(to_host(P.term_ids_device()), ids[keep != 0])
            assert np.array_equal(bits(to_host(P.table_device())), bits(table))
            assert np.array_equal(to_host(P.source_terms_device()), src)
            F = sm.SparseMatrix.from_csr_ids(n_rp, n_ci, n_ids, table, n_cols, opts=opts)
            table_ref.assert_same_matrix(P, F, ops, f"table source {mode} {opts}")
            pi, fi = P.info(), F.info()
            pi.pop("device_bytes"), fi.pop("device_bytes")
            assert pi == fi
            if opts:
                new = rng.uniform(-1, 1, 7).astype(np.float32)
                P.set_table(to_dev(new))
                F2 = sm.SparseMatrix.from_csr_ids(n_rp, n_ci, n_ids, new, n_cols, opts=opts)
                table_ref.assert_same_matrix(P, F2, ops, f"table source {mode}, set_table")


def test_dense_index_source(sm):
    rng = np.random.default_rng(94)
    rows, cols, T = 300, 257, 63
    dm = np.where(rng.random((rows, cols)) < 0.05, rng.integers(0, T, (rows, cols)), 255).astype(np.uint8)
    table = rng.uniform(-1, 1, T).astype(np.float32)
    Dx = sm.SparseMatrix(dm, rows, cols, cols, table, T)
    assert Dx.info()["has_ref_stream"] == 1 and Dx.info()["table_size"] == T
    rp, ci, va = Dx.csr()
    P = Dx.pruned(keep=va.size // 2)
    keep = pr.mask(rp, va, pr.GLOBAL_TOPK, va.size // 2)
    same_mask(Dx.prune_mask(keep=va.size // 2), keep, "dense-index mask")
    n_rp, n_ci, n_va, _, _ = pr.compact(rp, ci, va, keep)
    pi = P.info()
    assert pi["has_ref_stream"] == 0 and pi["table_size"] == 0 and pi["n_entries"] == 0   # an ordinary matrix
    F = sm.SparseMatrix.from_csr(n_rp, n_ci, n_va, pi["n_cols"])
    same_as_fresh(sm, P, F, keep, table_ref.Operands(pi["n_rows"], pi["n_cols"]), "dense-index source")


@pytest.mark.parametrize("variant", ["shuffled_repeated", "reversed"])
def test_messy_source_keeps_stored_order(sm, variant):
    import oracle
    rp, ci, va = messy_csr(variant, seed=95)
    n_cols = 40000
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    for mode in ("row", "mask"):
        P, keep = prune_by(M, rp, va, mode, None)
        n_rp, n_ci, n_va, _, src = pr.compact(rp, ci, va, keep)
        p_rp, p_ci, p_va = P.csr()
        assert np.array_equal(p_rp, n_rp) and np.array_equal(p_ci, n_ci) and np.array_equal(bits(p_va), bits(n_va))
        assert np.array_equal(to_host(P.source_terms_device()), src)
        F = sm.SparseMatrix.from_csr(n_rp, n_ci, n_va, n_cols)
        assert P == F and P.layout_digest() == F.layout_digest()
        rng = np.random.default_rng(96)
        x, y0 = rng.uniform(-1, 1, n_cols).astype(np.float32), rng.uniform(-1, 1, rp.size - 1).astype(np.float32)
        want, absum = oracle.csr_spmv_f64(n_rp.astype(np.int64), n_ci, n_va, x, y0, 1.3, 0.7)
        for algo in ("auto", "parity", "stream"):
            y = to_dev(y0)
            P.spmv(to_dev(x), y, 1.3, 0.7, algo=algo)
            assert_terms_close(to_host(y), want, absum)


def test_transposed_source(sm):
    rp, ci, n_cols = pattern("1000x777")
    va = value_set("uniform", ci.size)
    T = sm.SparseMatrix.from_csr(rp, ci, va, n_cols).transposed()
    t_rp, t_ci, t_va = T.csr()
    P, keep = prune_by(T, t_rp, t_va, "global", None)
    n_rp, n_ci, n_va, _, _ = pr.compact(t_rp, t_ci, t_va, keep)
    F = sm.SparseMatrix.from_csr(n_rp, n_ci, n_va, rp.size - 1)
    same_as_fresh(sm, P, F, keep, table_ref.Operands(n_cols, rp.size - 1), "transposed source")


# ------------------------------------------------------------------------------- updatable
@pytest.mark.parametrize("layout", ["auto", "band2"])
def test_updatable_takes_values_in_source_order(sm, layout):
    from sparsematrix_amd import _lib
    torch = torch_dev()
    if layout == "auto":
        rp, ci, n_cols = pattern("1000x777")
        va = value_set("uniform", ci.size)
        opts = {"updatable": 1}
    else:
        c = layout_specs._plain()
        rp, ci, va, n_cols = c.rp, c.ci, c.va, c.n_cols
        opts = {"updatable": 1, "layout": "band2", "band_slabs": 1}
    nnz = ci.size
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)           # the source itself need not be updatable
    P = M.pruned(keep=nnz // 2, opts=opts)
    keep = pr.mask(rp, va, pr.GLOBAL_TOPK, nnz // 2) != 0
    n_rp, n_ci, n_va, _, _ = pr.compact(rp, ci, va, keep)
    assert P.info()["updatable"] == 1
    ops = table_ref.Operands(rp.size - 1, n_cols)
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(97)
    new = rng.uniform(-1, 1, nnz).astype(np.float32)           # laid out for the unpruned matrix
    new[:table_ref.SPECIAL_BITS.size] = table_ref.SPECIAL_BITS.view(np.float32)
    delta = rng.uniform(-1, 1, nnz).astype(np.float32)
    d_new, d_delta = to_dev(new), to_dev(delta)
    assert L.sm_set_values(P._h, d_new.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    F = sm.SparseMatrix.from_csr(n_rp, n_ci, new[keep], n_cols, opts=opts)
    table_ref.assert_same_products(P, F, ops, f"{layout}: set, source order")
    assert L.sm_axpy_values(P._h, -0.37, d_delta.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    after = table_ref.axpy_reference(new[keep], -0.37, delta[keep])
    F2 = sm.SparseMatrix.from_csr(n_rp, n_ci, after, n_cols, opts=opts)
    table_ref.assert_same_products(P, F2, ops, f"{layout}: axpy, source order")
    own = rng.uniform(-1, 1, n_va.size).astype(np.float32)     # SM_VALUES_OWN: the pruned matrix's own order
    P.set_values(to_dev(own))
    F3 = sm.SparseMatrix.from_csr(n_rp, n_ci, own, n_cols, opts=opts)
    table_ref.assert_same_products(P, F3, ops, f"{layout}: set, own order")
    torch.cuda.synchronize()


def test_refusals(sm):
    from sparsematrix_amd import _lib
    torch = torch_dev()
    rp, ci, n_cols = pattern("300x257")
    va = value_set("uniform", ci.size)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols, opts={"updatable": 1})
    P = M.pruned(keep=ci.size // 2)                            # no updatable: the map is there, the refresh maps are not
    L = _lib.load()
    d = to_dev(va)
    assert L.sm_set_values(P._h, d.data_ptr(), _lib.SM_VALUES_SOURCE, None) == NOT_SUPPORTED
    assert L.sm_axpy_values(P._h, 1.0, d.data_ptr(), _lib.SM_VALUES_SOURCE, None) == NOT_SUPPORTED
    assert L.sm_set_values(M._h, d.data_ptr(), _lib.SM_VALUES_SOURCE, None) == NOT_SUPPORTED   # M was not made from another
    assert b"sm_create_masked" in L.sm_last_error()
    assert status_of(M.source_terms_device) == NOT_SUPPORTED   # a plain from_csr matrix holds no map
    t = torch.empty(ci.size, dtype=torch.int32, device="cuda")
    assert L.sm_copy_source_terms_device(M._h, t.data_ptr(), None) == NOT_SUPPORTED
    assert L.sm_copy_source_terms_device(P._h, None, None) == 1
    assert L.sm_create_masked(M._h, None, None, None, C.byref(C.c_void_p())) == 1   # a null mask with nnz > 0
    # a transposed updatable matrix already holds the same map
    Tm = M.transposed()
    t_src = to_host(Tm.source_terms_device())
    assert np.array_equal(np.sort(t_src), np.arange(ci.size))
    assert np.array_equal(bits(Tm.csr()[2]), bits(va[t_src]))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the pipeline
def test_prune_then_quantise(sm):
    rp, ci, n_cols = pattern("1000x777")
    va = value_set("uniform", ci.size)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols, opts={"updatable": 1})
    Q = M.pruned(per_row=4, opts={"updatable": 1}).quantized(15, iters=2)
    keep = pr.mask(rp, va, pr.ROW_TOPK, 4)
    n_rp, n_ci, n_va, _, _ = pr.compact(rp, ci, va, keep)
    ids, tab = qr.lloyd(n_va, 15, 2)
    assert np.array_equal(bits(to_host(Q.table_device())), bits(tab)), "table"
    assert np.array_equal(to_host(Q.term_ids_device()), ids), "ids"
    F = sm.SparseMatrix.from_csr_ids(n_rp, n_ci, ids, tab, n_cols)
    table_ref.assert_same_matrix(Q, F, table_ref.Operands(rp.size - 1, n_cols), "prune -> quantise")
