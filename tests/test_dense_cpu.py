"""CPU-side checks of the dense entrance and exit (sm_create_from_dense_device, sm_to_dense_device):
the library exports them and the Python mirror carries them, every argument check returns its
status in the header's order before any device work (a null d_w is the last of them, so a call that
reaches it has passed all the others without a device), and dense_ref, the numpy restatement the
GPU tests compare against, gives the written-out selections on hand-made ties."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import dense_ref as dr
import prune_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = 1, 5
NEW = ("sm_create_from_dense_device", "sm_to_dense_device")
P = 64        # stands for a device pointer: the checks below return before any is read
GLOBAL, ROW, THRESHOLD = pr.GLOBAL_TOPK, pr.ROW_TOPK, pr.THRESHOLD


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def create(lib, d_w=P, n_rows=3, n_cols=5, ld=5, mode=GLOBAL, count=1, threshold=0.0, out=True, **opts):
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p(77)
    st = lib.sm_create_from_dense_device(d_w, n_rows, n_cols, ld, mode, count, threshold, 0, None, C.byref(o),
                                         C.byref(h) if out else None)
    assert not out or st == 0 or not h.value, "a failed call leaves *out null"
    create.handle = h
    return st, lib.sm_last_error()


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "sparsematrix.h")).read()
    for name in NEW:
        assert f"SM_API sm_status {name}(" in header
    import sparsematrix_amd as smd
    sig = lambda f: list(inspect.signature(f).parameters)
    S = smd.SparseMatrix
    assert sig(S.from_dense) == ["W", "keep", "per_row", "threshold", "opts", "stream"]
    assert sig(S.dense_device)[1:] == ["out", "trans", "stream"]
    d = inspect.signature(S.from_dense).parameters
    assert all(d[k].default is None for k in ("keep", "per_row", "threshold", "opts", "stream"))
    d = inspect.signature(S.dense_device).parameters
    assert d["out"].default is None and d["trans"].default is True and d["stream"].default is None


def test_python_selector_and_operand_checks():
    import torch
    import sparsematrix_amd as smd
    S = smd.SparseMatrix
    W = torch.zeros(3, 5)
    for bad in ({}, {"keep": 1, "per_row": 2}, {"keep": 1, "threshold": 0.5}, {"per_row": 1, "threshold": 0.5}):
        with pytest.raises(ValueError, match="exactly one"):
            S.from_dense(W, **bad)
    with pytest.raises(TypeError, match="from_csr"):          # a host array names the host route
        S.from_dense(np.zeros((3, 5), np.float32), keep=1)
    with pytest.raises(TypeError, match="from_csr"):
        S.from_dense([[0.0, 1.0]], keep=1)
    with pytest.raises(TypeError, match="cuda"):              # a host tensor says what to do
        S.from_dense(W, keep=1)


def test_create_checks_come_before_the_device_in_order(lib):
    st, _ = create(lib, out=False)
    assert st == INVALID and b"out" in lib.sm_last_error()
    # a null out is reported before a bad mode; a bad mode before a bad shape
    assert create(lib, mode=9, out=False)[0] == INVALID and b"out" in lib.sm_last_error()
    for mode in (-1, 3, 100):
        st, err = create(lib, mode=mode, n_rows=-1)
        assert st == INVALID and b"sm_prune_mode" in err
    for mode in (GLOBAL, ROW):
        st, err = create(lib, mode=mode, count=-1, n_cols=-1)
        assert st == INVALID and b"count" in err
    for thr in (float("nan"), -1.0, -1e-45, float("-inf")):
        st, err = create(lib, mode=THRESHOLD, threshold=thr, ld=4)
        assert st == INVALID and b"threshold" in err
    # the shape before the options
    for kw in ({"n_rows": -1}, {"n_cols": -2}):
        st, err = create(lib, table_updatable=1, **kw)
        assert st == INVALID and b"negative" in err
    st, err = create(lib, ld=4, table_updatable=1)
    assert st == INVALID and b"ld 4 < n_cols 5" in err
    # the options before the sizes
    st, err = create(lib, n_rows=2 ** 31, ld=5, table_updatable=1)
    assert st == INVALID and b"table_updatable" in err
    st, err = create(lib, n_rows=2 ** 31, layout=99)
    assert st == INVALID and b"layout" in err
    # the sizes before the pointer
    st, err = create(lib, d_w=None, n_rows=2 ** 31)
    assert st == TOO_LARGE
    # and the pointer last: everything else about these calls is in order
    for kw in ({}, {"mode": ROW, "count": 0}, {"mode": THRESHOLD, "threshold": 0.0}, {"mode": THRESHOLD, "threshold": -0.0},
               {"mode": THRESHOLD, "threshold": float("inf")}, {"count": 0}, {"count": 10 ** 12}, {"ld": 2 ** 40},
               {"updatable": 1}, {"layout": 4}, {"mode": GLOBAL, "threshold": float("nan")},
               {"n_rows": 1, "ld": 0}, {"n_rows": 1, "ld": -7}):          # ld is not looked at for one row
        st, err = create(lib, d_w=None, **kw)
        assert st == INVALID and b"null matrix pointer" in err, kw


def test_too_large_is_decided_on_the_host(lib):
    big = dict(d_w=None)                                       # never reached: the sizes come first
    for kw in ({"n_rows": 2 ** 31, "n_cols": 1, "ld": 1}, {"n_rows": 1, "n_cols": 2 ** 31, "ld": 2 ** 31},
               {"n_rows": 2 ** 40, "n_cols": 2 ** 40, "ld": 2 ** 40}):
        st, err = create(lib, **big, **kw)
        assert st == TOO_LARGE and b"2^31" in err, kw
    # E = 2^32 is one too many for the 32-bit bins; E = 2^32 - 1 = 65535 * 65537 fits
    st, err = create(lib, **big, n_rows=65536, n_cols=65536, ld=65536, count=5)
    assert st == TOO_LARGE and b"2^32 - 1" in err
    edge = dict(n_rows=65535, n_cols=65537, ld=65537)
    st, err = create(lib, **big, **edge, count=5)
    assert st == INVALID and b"null matrix pointer" in err
    # the kept count where the arguments give it
    for kw in ({"mode": GLOBAL, "count": 2 ** 31}, {"mode": GLOBAL, "count": 2 ** 40},
               {"mode": ROW, "count": 32769}, {"mode": ROW, "count": 10 ** 9}):
        st, err = create(lib, **big, **edge, **kw)
        assert st == TOO_LARGE, kw
    for kw in ({"mode": GLOBAL, "count": 2 ** 30}, {"mode": ROW, "count": 16384},
               {"mode": THRESHOLD, "threshold": 0.0}):         # THRESHOLD is counted on the device
        st, err = create(lib, **big, **edge, **kw)
        assert st == INVALID and b"null matrix pointer" in err, kw


def test_empty_shapes_need_no_pointer_check(lib):
    """E = 0 passes every check with a null d_w; only the device is missing after that."""
    for kw in ({"n_rows": 0, "n_cols": 5}, {"n_rows": 5, "n_cols": 0, "ld": 0}, {"n_rows": 0, "n_cols": 0, "ld": 0}):
        st, err = create(lib, d_w=None, **kw)
        assert st in (0, 7), (kw, err)                         # SM_OK, or SM_ERR_NO_DEVICE
        if st == 0:
            lib.sm_destroy(create.handle)


def test_to_dense_device_checks(lib):
    assert lib.sm_to_dense_device(None, P, 5, 0, None) == INVALID and b"null matrix" in lib.sm_last_error()
    assert lib.sm_to_dense_device(None, None, -1, 7, None) == INVALID and b"null matrix" in lib.sm_last_error()


# ------------------------------------------------------------------ the restatement itself
SUB = np.float32(1e-45)     # the smallest subnormal, key 1
TIES = np.array([[0.5, -0.5, 0.0, -0.0],
                 [np.nan, -np.inf, 0.5, np.inf],
                 [-0.5, SUB, -SUB, 0.25]], np.float32)
#   i:             0     1    2     3 /  4       5     6     7 /   8    9   10    11
TIE_ORDER = [4, 5, 7, 0, 1, 6, 8, 11, 9, 10, 2, 3]   # NaN, the infinities, the 0.5 group, 0.25, subnormals, zeros


def test_full_csr():
    rp, ci = dr.full_csr(3, 4)
    assert rp.tolist() == [0, 4, 8, 12] and ci.tolist() == [0, 1, 2, 3] * 3 and ci.dtype == np.int32
    rp, ci = dr.full_csr(0, 4)
    assert rp.tolist() == [0] and ci.size == 0
    rp, ci = dr.full_csr(2, 0)
    assert rp.tolist() == [0, 0, 0] and ci.size == 0


def test_hand_made_ties_global():
    flat = TIES.reshape(-1)
    for count in range(14):
        rp, ci, va, keep = dr.select(TIES, GLOBAL, count)
        kept = sorted(TIE_ORDER[:count])
        assert np.flatnonzero(keep).tolist() == kept, count
        assert ci.tolist() == [i % 4 for i in kept] and rp.dtype == np.int32 and ci.dtype == np.int32
        assert rp.tolist() == [0] + [sum(i // 4 <= r for i in kept) for r in range(3)]
        assert np.array_equal(va.view(np.uint32), flat[kept].view(np.uint32))
    # written out: the NaN first; the cut inside the 0.5 group takes the lower i whatever the signs
    assert dr.select(TIES, GLOBAL, 1)[0].tolist() == [0, 0, 1, 1] and dr.select(TIES, GLOBAL, 1)[1].tolist() == [0]
    rp, ci, va, _ = dr.select(TIES, GLOBAL, 5)
    assert rp.tolist() == [0, 2, 5, 5] and ci.tolist() == [0, 1, 0, 1, 3]
    # a count past the non-zeros keeps zeros, lowest index first: +0.0 at i = 2 before -0.0 at i = 3
    rp, ci, va, _ = dr.select(TIES, GLOBAL, 11)
    assert rp.tolist() == [0, 3, 7, 11] and ci[:3].tolist() == [0, 1, 2]


def test_hand_made_ties_rows_and_threshold():
    rp, ci, va, _ = dr.select(TIES, ROW, 1)
    assert rp.tolist() == [0, 1, 2, 3] and ci.tolist() == [0, 0, 0]          # 0.5 before -0.5; the NaN; -0.5
    rp, ci, va, _ = dr.select(TIES, ROW, 3)
    assert rp.tolist() == [0, 3, 6, 9] and ci.tolist() == [0, 1, 2, 0, 1, 3, 0, 1, 3]
    assert dr.select(TIES, ROW, 0)[0].tolist() == [0, 0, 0, 0]
    for count in (4, 5, 10 ** 9):
        assert dr.select(TIES, ROW, count)[3].all()
    # threshold 0 keeps every element, the smallest subnormal exactly the non-zeros
    assert dr.select(TIES, THRESHOLD, threshold=0.0)[3].all() and dr.select(TIES, THRESHOLD, threshold=-0.0)[3].all()
    rp, ci, va, keep = dr.select(TIES, THRESHOLD, threshold=SUB)
    assert np.flatnonzero(keep).tolist() == [0, 1, 4, 5, 6, 7, 8, 9, 10, 11] and rp.tolist() == [0, 2, 6, 10]
    assert np.array_equal(keep != 0, (TIES.reshape(-1) != 0) | np.isnan(TIES.reshape(-1)))
    rp, ci, va, _ = dr.select(TIES, THRESHOLD, threshold=0.5)
    assert rp.tolist() == [0, 2, 6, 7] and ci.tolist() == [0, 1, 0, 1, 2, 3, 0]
    assert dr.select(TIES, THRESHOLD, threshold=np.inf)[1].tolist() == [0, 1, 3]   # the NaN and both infinities
    e = dr.select(np.zeros((0, 5), np.float32), GLOBAL, 3)
    assert e[0].tolist() == [0] and e[1].size == 0
    e = dr.select(np.zeros((5, 0), np.float32), ROW, 3)
    assert e[0].tolist() == [0] * 6 and e[1].size == 0
