"""CPU-side checks of the pruning calls (sm_prune_mask, sm_create_masked, sm_create_pruned,
sm_copy_source_terms_device): the library exports them and the Python mirror carries them, the
argument checks run before any device work, and the numpy restatement the GPU tests compare against
follows the header -- against a brute-force argsort of |v|, on hand-made ties with the kept
positions written out, and against np.add.reduceat / np.bincount for the compacted row pointer."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import prune_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # SM_ERR_INVALID_ARG
NEW = ("sm_prune_mask", "sm_create_masked", "sm_create_pruned", "sm_copy_source_terms_device")
P = 64        # stands for a device pointer: the checks below return before any is read
GLOBAL, ROW, THRESHOLD = pr.GLOBAL_TOPK, pr.ROW_TOPK, pr.THRESHOLD


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def _pruned(lib, mode=GLOBAL, count=1, threshold=0.0, **opts):
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    return lib.sm_create_pruned(None, mode, count, threshold, C.byref(o), None, C.byref(h)), h


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert (_lib.SM_PRUNE_GLOBAL_TOPK, _lib.SM_PRUNE_ROW_TOPK, _lib.SM_PRUNE_THRESHOLD) == (0, 1, 2)
    import sparsematrix_amd as smd
    sig = lambda f: list(inspect.signature(f).parameters)
    S = smd.SparseMatrix
    assert sig(S.prune_mask)[1:] == ["keep", "per_row", "threshold", "stream"]
    assert sig(S.masked)[1:] == ["keep", "opts", "stream"]
    assert sig(S.pruned)[1:] == ["keep", "per_row", "threshold", "opts", "stream"]
    assert sig(S.source_terms_device)[1:] == ["stream"]
    for f in (S.prune_mask, S.pruned):
        d = inspect.signature(f).parameters
        assert all(d[k].default is None for k in ("keep", "per_row", "threshold"))


def test_exactly_one_selection_argument():
    import sparsematrix_amd as smd
    S = smd.SparseMatrix
    assert S._prune_args(5, None, None) == (GLOBAL, 5, 0.0)
    assert S._prune_args(None, 3, None) == (ROW, 3, 0.0)
    assert S._prune_args(None, None, 0.25) == (THRESHOLD, 0, 0.25)
    for bad in ((None, None, None), (1, 2, None), (1, None, 0.5), (None, 2, 0.5), (1, 2, 0.5)):
        with pytest.raises(ValueError):
            S._prune_args(*bad)


def test_mask_checks_come_before_the_device(lib):
    kept = C.c_int64(-1)
    call = lambda mode, count, thr: lib.sm_prune_mask(None, mode, count, thr, P, C.byref(kept), None)
    for mode in (-1, 3, 100):
        assert call(mode, 1, 0.0) == INVALID and b"sm_prune_mode" in lib.sm_last_error()
    for mode in (GLOBAL, ROW):
        assert call(mode, -1, 0.0) == INVALID and b"count" in lib.sm_last_error()
        assert call(mode, 1, float("nan")) == INVALID and b"null matrix" in lib.sm_last_error()   # threshold ignored
    for thr in (float("nan"), -1.0, -1e-45, float("-inf")):
        assert call(THRESHOLD, 0, thr) == INVALID and b"threshold" in lib.sm_last_error()
    for thr in (0.0, -0.0, 1.0, float("inf")):      # legal thresholds reach the matrix check
        assert call(THRESHOLD, -5, thr) == INVALID and b"null matrix" in lib.sm_last_error()
    assert call(GLOBAL, 0, 0.0) == INVALID and b"null matrix" in lib.sm_last_error()            # count = 0 is legal
    assert kept.value == -1                         # nothing was written on the way out


def test_constructor_checks_come_before_the_device(lib):
    assert lib.sm_create_pruned(None, GLOBAL, 1, 0.0, None, None, None) == INVALID and b"out" in lib.sm_last_error()
    assert lib.sm_create_masked(None, P, None, None, None) == INVALID and b"out" in lib.sm_last_error()
    st, h = _pruned(lib, mode=7)
    assert st == INVALID and not h.value and b"sm_prune_mode" in lib.sm_last_error()
    for mode in (GLOBAL, ROW):
        st, h = _pruned(lib, mode=mode, count=-3)
        assert st == INVALID and not h.value and b"count" in lib.sm_last_error()
    for thr in (float("nan"), -0.5):
        st, h = _pruned(lib, mode=THRESHOLD, threshold=thr)
        assert st == INVALID and not h.value and b"threshold" in lib.sm_last_error()
    st, h = _pruned(lib)
    assert st == INVALID and not h.value and b"null matrix" in lib.sm_last_error()
    h = C.c_void_p()
    assert lib.sm_create_masked(None, P, None, None, C.byref(h)) == INVALID and b"null matrix" in lib.sm_last_error()
    assert lib.sm_copy_source_terms_device(None, P, None) == INVALID and b"null matrix" in lib.sm_last_error()


# ------------------------------------------------------------------ the restatement itself
def test_keys():
    v = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.0, -1.0, np.inf, -np.inf, np.nan], np.float32)
    k = pr.keys(v)
    assert k.dtype == np.uint32
    assert k[0] == k[1] == 0 and k[2] == k[3] == 1 and k[4] > k[2] and k[5] == k[6] == 0x3F800000
    assert k[7] == k[8] == 0x7F800000 and k[9] > k[7]
    assert np.all(np.diff(pr.keys(np.array([0, 1e-45, 1e-40, 1e-38, 1e-30, 1, 3e38, np.inf], np.float32)).astype(np.int64)) > 0)


def test_global_topk_is_the_largest_magnitudes():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 5000).astype(np.float32)
    assert np.unique(np.abs(v)).size == v.size                     # tie-free
    rp = np.arange(0, 5001, 5)
    order = np.argsort(-np.abs(v), kind="stable")
    for count in (0, 1, 17, 2500, 4999, 5000, 5001):
        keep = pr.mask(rp, v, GLOBAL, count)
        assert keep.dtype == np.uint8 and set(np.flatnonzero(keep)) == set(order[:count].tolist())
        assert int(keep.sum()) == min(count, v.size)
    # per row: the same within every row
    keep = pr.mask(rp, v, ROW, 2)
    for r in (0, 1, 999):
        row = np.abs(v[5 * r: 5 * r + 5])
        assert set(np.flatnonzero(keep[5 * r: 5 * r + 5])) == set(np.argsort(-row)[:2].tolist())
    assert int(keep.sum()) == 2000 and pr.mask(rp, v, ROW, 5).all() and pr.mask(rp, v, ROW, 10 ** 9).all()
    assert not pr.mask(rp, v, ROW, 0).any()


SUB = np.float32(1e-45)     # the smallest subnormal, key 1
TIES = np.array([0.5, -0.5, 0.0, -0.0, np.nan, -np.inf, 0.5, np.inf, -0.5, SUB, -SUB, 0.25], np.float32)
#   index         0     1    2     3      4       5     6     7      8    9    10    11
TIE_ORDER = [4, 5, 7, 0, 1, 6, 8, 11, 9, 10, 2, 3]   # NaN, the infinities, the 0.5 group, 0.25, subnormals, zeros


def test_hand_made_ties():
    nnz = TIES.size
    rp = np.array([0, nnz])
    for count in range(nnz + 2):
        want = np.zeros(nnz, np.uint8)
        want[TIE_ORDER[:count]] = 1
        assert np.array_equal(pr.mask(rp, TIES, GLOBAL, count), want), count
        assert np.array_equal(pr.mask(rp, TIES, ROW, count), want), count
    # written out: the cut inside the 0.5 group takes the lower indices whatever the signs
    assert np.flatnonzero(pr.mask(rp, TIES, GLOBAL, 5)).tolist() == [0, 1, 4, 5, 7]
    assert np.flatnonzero(pr.mask(rp, TIES, GLOBAL, 1)).tolist() == [4]                   # the NaN first
    assert np.flatnonzero(pr.mask(rp, TIES, GLOBAL, 9)).tolist() == [0, 1, 4, 5, 6, 7, 8, 9, 11]
    assert np.flatnonzero(pr.mask(rp, TIES, GLOBAL, 11)).tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]   # +0.0 before -0.0
    # two rows: ties to the earlier stored position of each row
    rp2 = np.array([0, 4, 4, nnz])
    assert np.flatnonzero(pr.mask(rp2, TIES, ROW, 1)).tolist() == [0, 4]
    assert np.flatnonzero(pr.mask(rp2, TIES, ROW, 3)).tolist() == [0, 1, 2, 4, 5, 7]
    # counts 0, 1, nnz, nnz + 1
    assert not pr.mask(rp, TIES, GLOBAL, 0).any() and pr.mask(rp, TIES, GLOBAL, nnz).all()
    assert pr.mask(rp, TIES, GLOBAL, nnz + 1).all()


def test_threshold():
    rp = np.array([0, TIES.size])
    assert pr.mask(rp, TIES, THRESHOLD, threshold=0.0).all()       # explicit zeros included
    assert pr.mask(rp, TIES, THRESHOLD, threshold=-0.0).all()
    assert np.flatnonzero(pr.mask(rp, TIES, THRESHOLD, threshold=0.5)).tolist() == [0, 1, 4, 5, 6, 7, 8]
    up = np.nextafter(np.float32(0.5), np.float32(1))
    assert np.flatnonzero(pr.mask(rp, TIES, THRESHOLD, threshold=up)).tolist() == [4, 5, 7]
    down = np.nextafter(np.float32(0.5), np.float32(0))
    assert np.flatnonzero(pr.mask(rp, TIES, THRESHOLD, threshold=down)).tolist() == [0, 1, 4, 5, 6, 7, 8]
    assert np.flatnonzero(pr.mask(rp, TIES, THRESHOLD, threshold=np.inf)).tolist() == [4, 5, 7]
    assert np.flatnonzero(pr.mask(rp, TIES, THRESHOLD, threshold=SUB)).tolist() == [0, 1, 4, 5, 6, 7, 8, 9, 10, 11]
    with pytest.raises(AssertionError):
        pr.mask(rp, TIES, THRESHOLD, threshold=-1.0)
    with pytest.raises(AssertionError):
        pr.mask(rp, TIES, THRESHOLD, threshold=np.nan)


def test_compact_row_pointer_and_source_terms():
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 9, 400)
    lens[[0, 7, 399]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, 1000, nnz).astype(np.int32)
    v = rng.uniform(-1, 1, nnz).astype(np.float32)
    ids = rng.integers(0, 7, nnz).astype(np.uint8)
    keep = (rng.uniform(0, 1, nnz) < 0.4).astype(np.uint8)
    keep[rp[3]:rp[4]] = 0                                          # a row emptied entirely
    n_rp, n_ci, n_v, n_ids, src = pr.compact(rp, ci, v, keep, ids)
    rows = np.repeat(np.arange(400), lens)
    want_lens = np.bincount(rows[keep != 0], minlength=400)
    assert np.array_equal(np.diff(n_rp), want_lens) and n_rp[0] == 0 and n_rp.dtype == np.int32
    nonempty = np.flatnonzero(lens > 0)
    by_row = np.add.reduceat(keep.astype(np.int64), rp[:-1][nonempty])
    assert np.array_equal(np.diff(n_rp)[nonempty], by_row) and not np.diff(n_rp)[lens == 0].any()
    assert np.array_equal(src, np.flatnonzero(keep)) and src.dtype == np.int32
    assert np.array_equal(n_ci, ci[src]) and np.array_equal(n_ids, ids[src])
    assert np.array_equal(n_v.view(np.uint32), v[src].view(np.uint32))
    assert pr.compact(rp, ci, v, keep)[3] is None
    e_rp, e_ci, e_v, _, e_src = pr.compact(rp, ci, v, np.zeros(nnz, np.uint8))
    assert not e_rp.any() and e_ci.size == e_v.size == e_src.size == 0
    a_rp, a_ci, _, _, a_src = pr.compact(rp, ci, v, np.full(nnz, 255, np.uint8))   # any non-zero byte keeps
    assert np.array_equal(a_rp, rp) and np.array_equal(a_ci, ci) and np.array_equal(a_src, np.arange(nnz))
