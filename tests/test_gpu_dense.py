"""From and to dense weights on the GPU: sm_create_from_dense_device and sm_to_dense_device.

Every from_dense result is compared bit for bit with dense_ref.select, the numpy restatement of
the header's rule (sm_prune_mask's on the full matrix), and with SparseMatrix.from_csr of the
restated arrays: ==, digests, info, where the layouts were built, products.  The operands sit at
both 16-byte offsets, contiguous and padded; padding and guards hold a NaN, which the rule keeps
first, so any read of them changes the result.  Every dense_device result is compared with the
host CopyTo's bits or with the stored terms, its padding and guards with what they held before.
"""
import functools

import numpy as np
import pytest

import dense_ref as dr
import prune_ref as pr
import quantize_ref as qr
import table_ref
from gpu_util import (GUARD_BITS, assert_guards_2d, bits, messy_csr, placed_2d, to_dev, to_host, torch_dev,
                      uniform_csr)

pytestmark = pytest.mark.gpu

INVALID = 1
SUB = float(np.float32(1e-45))     # the smallest subnormal, key 1
GiB = 1 << 30


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


# ------------------------------------------------------------------------------- inputs
# The smallest shapes at which each path can go wrong: one element, one row, one column; rows at
# the wavefront kernel's limit of 64 and on either side; a chunk of 2048 elements less one and plus
# one; rows and columns past one workgroup step; more rows than one chunk with rows that straddle
# the chunks; and no elements at all.
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 63), (3, 64), (3, 65), (300, 255), (5, 257), (2, 2047), (2, 2049), (1, 5000),
          (5000, 1), (65, 2049), (0, 5), (5, 0)]
VALUE_SETS = ("uniform", "ties7", "low_byte", "specials", "zeros")
PLACEMENTS = [(0, 0), (0, 1), (3, 0), (3, 1)]          # (padding columns, floats past 16-byte alignment)
TIE_TABLE = np.array([0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 0.125], np.float32)
SPECIAL = np.array([0.5, -0.5, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 0.5, -0.0, np.nan],
                   np.float32)


def value_set(name, shape):
    E = shape[0] * shape[1]
    rng = np.random.default_rng(71)
    i = np.arange(E, dtype=np.uint64)
    sign = rng.integers(0, 2, E).astype(np.uint32) << np.uint32(31)
    if name == "uniform":
        v = rng.uniform(-1, 1, E).astype(np.float32)
    elif name == "ties7":                          # heavy ties: the rank among equals decides everywhere
        v = TIE_TABLE[rng.integers(0, 7, E)]
    elif name == "low_byte":                       # only the last radix pass tells the keys apart
        v = ((np.uint32(0x3F000000) + ((i * 37) % 256).astype(np.uint32)) | sign).view(np.float32)
    elif name == "specials":                       # at the front, the back and across the chunk boundary
        v = rng.uniform(-1, 1, E).astype(np.float32)
        n = min(SPECIAL.size, E)
        v[:n] = SPECIAL[:n]
        v[E - n:] = SPECIAL[:n][::-1]
        if E > 2048 + n:
            v[2048 - n // 2: 2048 - n // 2 + n] = SPECIAL
    elif name == "zeros":
        v = np.zeros(E, np.float32)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, np.float32).reshape(shape)


def tie_cut(W):
    """A global count that cuts inside a group of equal keys near the middle (E // 2 without one)."""
    k = np.sort(pr.keys(W))[::-1]
    E = k.size
    for j in list(range(max(E // 2, 1), E)) + list(range(1, max(E // 2, 1))):
        if k[j - 1] == k[j]:
            return j
    return E // 2


def selectors(W):
    """[(keyword arguments of from_dense, arguments of dense_ref.select)]."""
    n_rows, n_cols = W.shape
    E = n_rows * n_cols
    out = []
    for count in sorted({0, 1, tie_cut(W), max(E - 1, 0), E, E + 1}):
        out.append(({"keep": count}, (pr.GLOBAL_TOPK, count, 0.0)))
    for count in sorted({0, 1, max(n_cols - 1, 0), n_cols, n_cols + 1}):
        out.append(({"per_row": count}, (pr.ROW_TOPK, count, 0.0)))
    for thr in (0.0, SUB, 0.5, float("inf")):
        out.append(({"threshold": thr}, (pr.THRESHOLD, 0, thr)))
    return out


def same_csr(M, want, tag):
    rp, ci, va = (to_host(t) for t in M.csr_device())
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, want[0]), f"{tag}: row_ptr"
    assert np.array_equal(ci, want[1]), f"{tag}: col_idx"
    assert np.array_equal(bits(va), bits(want[2])), f"{tag}: values (bits)"


def same_as_from_csr(sm, M, want, n_cols, opts, tag, products=True):
    """M is the matrix from_csr builds from the restated arrays on the device."""
    D = sm.SparseMatrix.from_csr(to_dev(want[0]), to_dev(want[1]), to_dev(want[2]), n_cols, opts=opts)
    assert M == D, tag + ": =="
    assert M.layout_digest() == D.layout_digest(), tag + ": layout digest"
    mi, di = M.info(), D.info()
    mi.pop("device_bytes"), di.pop("device_bytes")
    assert mi == di, tag + ": info"
    assert M.built_on_device() == D.built_on_device(), tag + ": built_on_device"
    n_rows = want[0].size - 1
    if products and n_rows and n_cols:
        rng = np.random.default_rng(5)
        x, y0 = to_dev(rng.uniform(-1, 1, n_cols).astype(np.float32)), to_dev(rng.uniform(-1, 1, n_rows).astype(np.float32))
        for algo in ("auto", "parity"):
            ym, yd = y0.clone(), y0.clone()
            M.spmv(x, ym, 1.3, 0.7, algo=algo)
            D.spmv(x, yd, 1.3, 0.7, algo=algo)
            assert table_ref.same_bits(ym, yd), f"{tag}: spmv {algo}"
    return D


@pytest.mark.parametrize("values", VALUE_SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_from_dense(sm, shape, values):
    W = value_set(values, shape)
    n_rows, n_cols = shape
    placements = PLACEMENTS if W.size else [(0, 0), (3, 0)]       # an empty tensor has no address to place
    views = [placed_2d(W, n_cols + pad, off) if W.size else (to_dev(np.zeros((n_rows, n_cols + pad), np.float32))[:, :n_cols], None)
             for pad, off in placements]
    heavy = placements[-1]                                          # the scalar path; the others by their CSR
    for kw, ref_args in selectors(W):
        want = dr.select(W, *ref_args)
        for (pad, off), (view, parent) in zip(placements, views):
            tag = f"{kw} pad={pad} off={off}"
            M = sm.SparseMatrix.from_dense(view, **kw)
            same_csr(M, want, tag)
            with pytest.raises(sm._lib.SparseMatrixError):         # no source map: a term's origin is its (row, column)
                M.source_terms_device()
            if (pad, off) == heavy:
                same_as_from_csr(sm, M, want, n_cols, None, tag)
    for (pad, off), (view, parent) in zip(placements if W.size else [], views):   # W is never written
        assert np.array_equal(bits(to_host(view)), bits(W))
        assert_guards_2d(parent, off, n_rows, n_cols, n_cols + pad)


def test_from_dense_vector_loads_in_padded_rows(sm):
    """ld and n_cols multiples of four at a 16-byte aligned base: the padded 16-byte path."""
    W = value_set("specials", (37, 260))
    view, parent = placed_2d(W, 264, 0)
    for kw, ref_args in selectors(W):
        same_csr(sm.SparseMatrix.from_dense(view, **kw), dr.select(W, *ref_args), f"{kw}")
    assert_guards_2d(parent, 0, 37, 260, 264)


def test_row_sliced_view_and_python_checks(sm):
    W = value_set("uniform", (40, 100))
    d = to_dev(W)
    M = sm.SparseMatrix.from_dense(d[5:17, :64], per_row=3)         # rows and columns sliced: no copy
    same_csr(M, dr.select(W[5:17, :64], pr.ROW_TOPK, 3), "sliced view")
    with pytest.raises(ValueError, match="contiguous"):
        sm.SparseMatrix.from_dense(d.t(), keep=5)
    with pytest.raises(ValueError, match="contiguous"):
        sm.SparseMatrix.from_dense(d[:, ::2], keep=5)
    with pytest.raises(ValueError, match="contiguous"):
        sm.SparseMatrix.from_dense(d[0:1].expand(4, 100), keep=5)
    with pytest.raises(ValueError, match="2-D"):
        sm.SparseMatrix.from_dense(d.reshape(-1), keep=5)
    with pytest.raises(TypeError, match="float32"):
        sm.SparseMatrix.from_dense(d.half(), keep=5)
    with pytest.raises(TypeError, match="from_csr"):
        sm.SparseMatrix.from_dense(W, keep=5)
    with pytest.raises(ValueError):
        sm.SparseMatrix.from_dense(d, keep=5, threshold=0.5)
    with pytest.raises(sm._lib.SparseMatrixError) as ei:
        sm.SparseMatrix.from_dense(d, keep=-1)
    assert ei.value.status == INVALID
    with pytest.raises(sm._lib.SparseMatrixError) as ei:
        sm.SparseMatrix.from_dense(d, keep=5, opts={"table_updatable": 1})
    assert ei.value.status == INVALID


@functools.lru_cache(maxsize=None)
def wide_case():
    """600 x 20000, wide enough for a band layout to be asked for; eight kept terms a row."""
    rng = np.random.default_rng(31)
    W = rng.uniform(-1, 1, (600, 20000)).astype(np.float32)
    return W, dr.select(W, pr.ROW_TOPK, 8)


def test_band2_option(sm):
    W, want = wide_case()
    opts = {"layout": "band2", "band_slabs": 1}
    M = sm.SparseMatrix.from_dense(to_dev(W), per_row=8, opts=opts)
    same_csr(M, want, "band2")
    same_as_from_csr(sm, M, want, W.shape[1], opts, "band2")


def test_updatable_option(sm):
    W, want = wide_case()
    opts = {"updatable": 1}
    M = sm.SparseMatrix.from_dense(to_dev(W), per_row=8, opts=opts)
    assert M.info()["updatable"] == 1
    same_as_from_csr(sm, M, want, W.shape[1], opts, "updatable")
    rng = np.random.default_rng(32)
    delta = rng.uniform(-1, 1, want[2].size).astype(np.float32)
    M.axpy_values(-0.37, to_dev(delta))
    after = table_ref.axpy_reference(want[2], -0.37, delta)
    same_csr(M, (want[0], want[1], after), "after axpy_values")
    same_as_from_csr(sm, M, (want[0], want[1], after), W.shape[1], opts, "after axpy_values")


def test_pipeline_from_dense_to_dense(sm):
    """dense -> from_dense -> pruned -> quantized -> dense_device, all on the device."""
    W = value_set("uniform", (300, 255))
    M = sm.SparseMatrix.from_dense(to_dev(W), per_row=6, opts={"updatable": 1})
    rp, ci, va, _ = dr.select(W, pr.ROW_TOPK, 6)
    P = M.pruned(per_row=4, opts={"updatable": 1})
    keep = pr.mask(rp, va, pr.ROW_TOPK, 4)
    n_rp, n_ci, n_va, _, src = pr.compact(rp, ci, va, keep)
    same_csr(P, (n_rp, n_ci, n_va), "pruned")
    assert np.array_equal(to_host(P.source_terms_device()), src)
    Q = P.quantized(15, iters=2)
    ids, tab = qr.lloyd(n_va, 15, 2)
    assert np.array_equal(bits(to_host(Q.table_device())), bits(tab)) and np.array_equal(to_host(Q.term_ids_device()), ids)
    F = sm.SparseMatrix.from_csr_ids(n_rp, n_ci, ids, tab, 255)
    table_ref.assert_same_matrix(Q, F, table_ref.Operands(300, 255), "from_dense -> prune -> quantise")
    back = np.zeros((300, 255), np.float32)
    back[np.repeat(np.arange(300), np.diff(n_rp)), n_ci] = tab[ids]
    assert np.array_equal(bits(to_host(Q.dense_device())), bits(back))


# ------------------------------------------------------------------------------- dense_device
@functools.lru_cache(maxsize=None)
def sorted_case():
    rp, ci, va = uniform_csr(300, 257, 6, seed=7)
    va = np.random.default_rng(8).uniform(-1, 1, va.size).astype(np.float32)
    va[:table_ref.SPECIAL_BITS.size] = table_ref.SPECIAL_BITS.view(np.float32)
    va[va == 0] = 1.0                              # no explicit zeros: the round trip gives the matrix back
    return rp, ci, va


def test_dense_device_orientations_match_copyto(sm):
    rp, ci, va = sorted_case()
    M = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    B = M.dense_device()
    S = M.dense_device(trans=False)
    assert tuple(B.shape) == (300, 257) and tuple(S.shape) == (257, 300)
    assert np.array_equal(bits(to_host(B)), bits(M.CopyTo(None, 257, 1)[:300 * 257]))
    assert np.array_equal(bits(to_host(S)), bits(M.CopyTo(None, 300, 0)[:257 * 300]))
    want = np.zeros((300, 257), np.float32)
    want[np.repeat(np.arange(300), 6), ci] = va
    assert np.array_equal(bits(to_host(B)), bits(want)) and np.array_equal(bits(to_host(S)), bits(want.T))
    # a device-built matrix decides the ascending-rows flag by the validation kernel
    Dm = sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), 257)
    assert np.array_equal(bits(to_host(Dm.dense_device())), bits(want))


@pytest.mark.parametrize("pad,off", PLACEMENTS + [(4, 0)])
@pytest.mark.parametrize("trans", [True, False])
def test_dense_device_out_keeps_padding_and_guards(sm, trans, pad, off):
    rp, ci, va = sorted_case()
    M = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    want = np.zeros((300, 257), np.float32)
    want[np.repeat(np.arange(300), 6), ci] = va
    want = want if trans else np.ascontiguousarray(want.T)
    rows, cols = want.shape
    view, parent = placed_2d(np.full((rows, cols), 7.0, np.float32), cols + pad, off)
    got = M.dense_device(out=view, trans=trans)
    assert got is view
    assert np.array_equal(bits(to_host(view)), bits(want))
    assert_guards_2d(parent, off, rows, cols, cols + pad)


def test_dense_device_larger_out_and_checks(sm):
    torch = torch_dev()
    rp, ci, va = sorted_case()
    M = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    big = torch.full((310, 300), 7.0, device="cuda")
    M.dense_device(out=big)                                         # enough rows and columns: the leading part
    h = to_host(big)
    assert np.array_equal(bits(h[:300, :257]), bits(to_host(M.dense_device())))
    assert (h[300:] == 7.0).all() and (h[:, 257:] == 7.0).all()
    with pytest.raises(ValueError):
        M.dense_device(out=torch.zeros(299, 257, device="cuda"))
    with pytest.raises(ValueError):
        M.dense_device(out=torch.zeros(257, 300, device="cuda").t())
    with pytest.raises(TypeError):
        M.dense_device(out=np.zeros((300, 257), np.float32))
    L = sm._lib.load()
    out = torch.zeros(300, 257, device="cuda")
    assert L.sm_to_dense_device(M._h, out.data_ptr(), 257, 2, None) == INVALID and b"trans" in L.sm_last_error()
    assert L.sm_to_dense_device(M._h, out.data_ptr(), 256, 1, None) == INVALID and b"ld" in L.sm_last_error()
    assert L.sm_to_dense_device(M._h, out.data_ptr(), 299, 0, None) == INVALID and b"ld" in L.sm_last_error()
    assert L.sm_to_dense_device(M._h, None, 257, 1, None) == INVALID and b"null output" in L.sm_last_error()
    empty = sm.SparseMatrix.from_dense(torch.zeros(0, 5, device="cuda"), keep=3)
    assert L.sm_to_dense_device(empty._h, None, 0, 1, None) == 0                 # an empty output: nothing launched
    assert tuple(empty.dense_device().shape) == (0, 5) and tuple(empty.dense_device(trans=False).shape) == (5, 0)
    torch.cuda.synchronize()
    assert not (to_host(out) != 0).any()


@pytest.mark.parametrize("variant", ["shuffled_repeated", "reversed", "repeated"])
def test_dense_device_last_stored_term_wins(sm, variant):
    torch = torch_dev()
    rp, ci, va = messy_csr(variant, seed=95, codebook=False)
    n_rows, n_cols = rp.size - 1, 40000
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    key = rows.astype(np.int64) * n_cols + ci
    order = np.argsort(key, kind="stable")
    last = np.ones(key.size, bool)
    last[:-1] = key[order][1:] != key[order][:-1]                  # the last stored term of every (row, column)
    win_key, win_val = key[order][last], va[order][last]
    assert win_key.size < key.size or variant == "reversed"
    for make in (lambda: sm.SparseMatrix.from_csr(rp, ci, va, n_cols),
                 lambda: sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), n_cols)):
        M = make()
        for trans in (True, False):
            d = M.dense_device(trans=trans)
            r_t, c_t = to_dev(win_key // n_cols), to_dev(win_key % n_cols)
            got = d[r_t, c_t] if trans else d[c_t, r_t]
            assert np.array_equal(bits(to_host(got)), bits(win_val)), f"{variant} trans={trans}"
            assert int(torch.count_nonzero(d)) == int((win_val != 0).sum()), "zeros everywhere else"
            del d


def test_dense_device_in_a_graph(sm):
    torch = torch_dev()
    rp, ci, va = sorted_case()
    M = sm.SparseMatrix.from_csr(rp, ci, va, 257)
    eager = M.dense_device()
    view, parent = placed_2d(np.full((300, 257), 7.0, np.float32), 260, 1)
    M.dense_device(out=view)                                        # the kernels of this placement are loaded
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            M.dense_device(out=view)
    for _ in range(2):
        view.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        assert table_ref.same_bits(view, eager)
        assert_guards_2d(parent, 1, 300, 257, 260)


def test_round_trip(sm):
    rp, ci, va = sorted_case()
    for opts in (None, {"layout": "no_bands"}):
        M = sm.SparseMatrix.from_csr(to_dev(rp), to_dev(ci), to_dev(va), 257, opts=opts)
        R = sm.SparseMatrix.from_dense(M.dense_device(), threshold=SUB, opts=opts)
        assert R == M and R.layout_digest() == M.layout_digest() and R.built_on_device() == M.built_on_device()
        same_csr(R, (rp, ci, va), "round trip")
        view, parent = placed_2d(np.zeros((300, 257), np.float32), 259, 1)
        R2 = sm.SparseMatrix.from_dense(M.dense_device(out=view), threshold=SUB, opts=opts)   # through a padded buffer
        assert R2 == M and R2.layout_digest() == M.layout_digest()


# ------------------------------------------------------------------------------- past 2^31
def need_free(n_bytes):
    torch = torch_dev()
    free = torch.cuda.mem_get_info()[0]
    if free < n_bytes:
        pytest.skip(f"needs {n_bytes / GiB:.1f} GiB of free device memory, {free / GiB:.1f} GiB are free")


def test_rows_past_4gib(sm):
    """3 x 5 with ld = 2^29 + 3: rows 1 and 2 start past 2 GiB and 4 GiB."""
    torch = torch_dev()
    need_free(10 * GiB)
    ld, g = (1 << 29) + 3, 8
    W = value_set("specials", (3, 5))

    def strided():
        parent = torch.empty(g + 1 + 2 * ld + 5 + g, dtype=torch.float32, device="cuda")
        view = parent.as_strided((3, 5), (ld, 1), g + 1)           # one float past 16-byte alignment
        for r in range(3):                                          # the guards: eight words either side of every row
            a = g + 1 + r * ld
            parent[a - g: a + 5 + g].view(torch.int32).fill_(GUARD_BITS)
        return parent, view

    def guards_ok(parent):
        for r in range(3):
            a = g + 1 + r * ld
            w = parent[a - g: a + 5 + g].view(torch.int32).cpu().numpy().view(np.uint32)
            assert (w[:g] == GUARD_BITS).all() and (w[g + 5:] == GUARD_BITS).all(), f"guards of row {r}"

    parent, view = strided()
    view.copy_(to_dev(W))
    for kw, ref_args in selectors(W):
        same_csr(sm.SparseMatrix.from_dense(view, **kw), dr.select(W, *ref_args), f"{kw}")
    guards_ok(parent)
    assert np.array_equal(bits(to_host(view)), bits(W))
    M = sm.SparseMatrix.from_dense(view, threshold=0.0)
    parent2, out = strided()
    out.fill_(7.0)
    M.dense_device(out=out)
    assert np.array_equal(bits(to_host(out)), bits(W))
    guards_ok(parent2)


def test_more_than_2_31_elements(sm):
    """32769 x 65536 zeros (E = 2^31 + 65536, 8 GiB) with seven non-zeros, three of them past
    element 2^31; the expectations are written out and nothing E-sized comes down."""
    torch = torch_dev()
    need_free(13 * GiB)
    n_rows, n_cols = 32769, 65536
    W = torch.zeros((n_rows, n_cols), dtype=torch.float32, device="cuda")
    placed = [(0, 5, 1.0), (100, 7, -2.0), (20000, 30000, 1.5), (32767, 65535, 3.0),   # the last: i = 2^31 - 1
              (32768, 0, -4.0), (32768, 1234, -1.0), (32768, 65535, 5.0)]              # i = 2^31, ..., E - 1
    for r, c, v in placed:
        W[r, c] = v

    def expect(terms):
        rp = np.zeros(n_rows + 1, np.int64)
        for r, _, _ in terms:
            rp[r + 1] += 1
        return (np.cumsum(rp).astype(np.int32), np.array([c for _, c, _ in terms], np.int32),
                np.array([v for _, _, v in terms], np.float32))

    same_csr(sm.SparseMatrix.from_dense(W, threshold=1.0), expect(placed), "threshold=1.0")
    # ten: the seven, then zeros by lowest index -- (0, 0), (0, 1), (0, 2): the tie base of the
    # chunks past 2^31 equal keys
    ten = sorted(placed + [(0, 0, 0.0), (0, 1, 0.0), (0, 2, 0.0)])
    same_csr(sm.SparseMatrix.from_dense(W, keep=10), expect(ten), "keep=10")
    same_csr(sm.SparseMatrix.from_dense(W, keep=3), expect([placed[3], placed[4], placed[6]]), "keep=3")
    per_row = sm.SparseMatrix.from_dense(W[32760:], per_row=2)
    want = []
    for r in range(9):
        mine = sorted([(c, v) for rr, c, v in placed if rr == 32760 + r], key=lambda t: -abs(t[1]))[:2]
        cols = sorted([c for c, _ in mine] + [c for c in (0, 1) if c not in [m[0] for m in mine]][:2 - len(mine)])
        want += [(r, c, dict(mine).get(c, 0.0)) for c in cols]
    same_csr(per_row, (np.arange(10, dtype=np.int32) * 2, np.array([c for _, c, _ in want], np.int32),
                       np.array([v for _, _, v in want], np.float32)), "per_row=2 on the last rows")
