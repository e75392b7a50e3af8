"""CPU-side checks of sm_create_sum and sm_copy_sum_terms_device: the library exports them and the
Python mirror carries them, the first argument checks return before any device is touched, and the
numpy restatement the GPU tests compare against follows the header -- against a brute-force union
over dictionaries on random ragged rows, and on hand-written cases with the expected arrays spelled
out."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import sum_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # SM_ERR_INVALID_ARG
NEW = ("sm_create_sum", "sm_copy_sum_terms_device")
P = 64        # stands for a pointer: the checks below return before any is read


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    import sparsematrix_amd as smd
    S = smd.SparseMatrix
    p = inspect.signature(S.sum).parameters
    assert list(p)[1:] == ["other", "alpha", "beta", "opts", "stream"]
    assert p["alpha"].default == 1.0 and p["beta"].default == 1.0
    assert p["opts"].default is None and p["stream"].default is None
    assert list(inspect.signature(S.sum_terms_device).parameters)[1:] == ["stream"]
    assert not hasattr(S, "__add__") and not hasattr(S, "__sub__")   # no operator overloading


def test_checks_come_before_the_device(lib):
    assert lib.sm_create_sum(P, 1.0, P, 1.0, None, None, None) == INVALID and b"out" in lib.sm_last_error()
    for a, b in ((None, None), (None, P), (P, None)):
        h = C.c_void_p(7)
        assert lib.sm_create_sum(a, 1.0, b, 1.0, None, None, C.byref(h)) == INVALID
        assert b"null matrix" in lib.sm_last_error() and not h.value
    assert lib.sm_copy_sum_terms_device(None, P, P, None) == INVALID and b"null matrix" in lib.sm_last_error()


# ------------------------------------------------------------------ the restatement itself
def f32(*v):
    return np.array(v, np.float32)


def i32(*v):
    return np.array(v, np.int32)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def brute(rp_a, ci_a, rp_b, ci_b):
    """The union by one dictionary per row: (rp_c, ci_c, terms_a, terms_b)."""
    rp_c, ci_c, ta, tb = [0], [], [], []
    for r in range(len(rp_a) - 1):
        da = {int(ci_a[e]): e for e in range(rp_a[r], rp_a[r + 1])}
        db = {int(ci_b[e]): e for e in range(rp_b[r], rp_b[r + 1])}
        for c in sorted(set(da) | set(db)):
            ci_c.append(c)
            ta.append(da.get(c, -1))
            tb.append(db.get(c, -1))
        rp_c.append(len(ci_c))
    return i32(*rp_c), i32(*ci_c), i32(*ta), i32(*tb)


def ragged(rng, n_rows, n_cols, max_len, empty_every):
    lens = rng.integers(0, min(max_len, n_cols) + 1, n_rows)
    if empty_every:
        lens[::empty_every] = 0
    rows = [np.sort(rng.choice(n_cols, int(k), replace=False)) for k in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return rp, ci


@pytest.mark.parametrize("seed,n_rows,n_cols,max_len", [(1, 200, 40, 12), (2, 150, 9, 9), (3, 64, 1, 1), (4, 97, 1000, 30)])
def test_union_against_dictionaries(seed, n_rows, n_cols, max_len):
    rng = np.random.default_rng(seed)
    rp_a, ci_a = ragged(rng, n_rows, n_cols, max_len, 7)
    rp_b, ci_b = ragged(rng, n_rows, n_cols, max_len, 5)
    for (pa, ca), (pb, cb) in (((rp_a, ci_a), (rp_b, ci_b)), ((rp_a, ci_a), (rp_a, ci_a)),      # full overlap
                               ((rp_a, ci_a), (np.zeros(n_rows + 1, np.int32), i32())),             # B empty
                               ((np.zeros(n_rows + 1, np.int32), i32()), (rp_b, ci_b))):            # A empty
        got = sr.union(pa, ca, pb, cb, n_cols)
        want = brute(pa, ca, pb, cb)
        for g, w, name in zip(got, want, ("row_ptr", "col_idx", "terms_a", "terms_b")):
            assert g.dtype == np.int32 and np.array_equal(g, w), name
    e = sr.union(i32(0), i32(), i32(0), i32(), 5)   # 0 rows
    assert np.array_equal(e[0], [0]) and all(x.size == 0 for x in e[1:])


def test_the_restatement_refuses_rows_that_do_not_ascend():
    with pytest.raises(AssertionError):
        sr.union(i32(0, 2), i32(3, 3), i32(0, 0), i32(), 5)
    with pytest.raises(AssertionError):
        sr.union(i32(0, 0), i32(), i32(0, 2), i32(4, 1), 5)


# 4 x 6.  Row 0: a column only in A (1), only in B (2), in both at column 0 and at n_cols - 1.
# Row 1: empty in A.  Row 2: empty in B.  Row 3: empty in both.
RP_A, CI_A = i32(0, 3, 3, 5, 5), i32(0, 1, 5, 2, 4)
RP_B, CI_B = i32(0, 3, 5, 5, 5), i32(0, 2, 5, 1, 3)
VA_A, VA_B = f32(1.5, -2.0, 0.25, 3.0, -0.0), f32(-1.5, 8.0, 0.5, 1e-40, np.inf)
WANT_RP, WANT_CI = i32(0, 4, 6, 8, 8), i32(0, 1, 2, 5, 1, 3, 2, 4)
WANT_TA, WANT_TB = i32(0, 1, -1, 2, -1, -1, 3, 4), i32(0, -1, 1, 2, 3, 4, -1, -1)
SUB = np.float32(1e-40)


def test_hand_written_pattern_and_maps():
    rp, ci, ta, tb = sr.union(RP_A, CI_A, RP_B, CI_B, 6)
    assert np.array_equal(rp, WANT_RP) and np.array_equal(ci, WANT_CI)
    assert np.array_equal(ta, WANT_TA) and np.array_equal(tb, WANT_TB)


@pytest.mark.parametrize("alpha,beta,want", [
    # a + (-a) = +0.0 stays a stored term; -0.0 alone keeps its sign; the subnormal survives
    (1.0, 1.0, f32(0.0, -2.0, 8.0, 0.75, SUB, np.inf, 3.0, -0.0)),
    (1.0, 0.0, f32(1.5, -2.0, 0.0, 0.25, 0.0, 0.0, 3.0, -0.0)),                # the regrow step: B only adds positions
    (0.0, 1.0, f32(-1.5, 0.0, 8.0, 0.5, SUB, np.inf, 0.0, 0.0)),
    (0.0, 0.0, f32(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    (-0.5, 3.0, f32(-5.25, 1.0, 24.0, 1.375, np.float32(3.0) * SUB, np.inf, -1.5, 0.0)),
    (1.0, -1.0, f32(3.0, -2.0, -8.0, -0.25, -SUB, -np.inf, 3.0, -0.0)),
])
def test_hand_written_values(alpha, beta, want):
    rp, ci, va, ta, tb = sr.sum_csr(RP_A, CI_A, VA_A, alpha, RP_B, CI_B, VA_B, beta, 6)
    assert va.dtype == np.float32 and np.array_equal(bits(va), bits(want)), (va, want)


def test_hand_written_specials():
    rp, ci = i32(0, 6), i32(0, 1, 2, 3, 4, 5)
    a = f32(np.inf, np.inf, -0.0, 1e-45, np.nan, 3e38)
    b = f32(np.inf, -np.inf, -0.0, -1e-45, 1.0, 3e38)
    va = sr.sum_csr(rp, ci, a, 1.0, rp, ci, b, 1.0, 6)[2]
    assert np.array_equal(bits(va[[0, 2, 3, 5]]), bits(f32(np.inf, -0.0, 0.0, np.inf)))
    assert np.isnan(va[1]) and np.isnan(va[4])                                 # Inf - Inf, a NaN operand
    # a coefficient of 0 leaves the operand unread: its NaN and Inf do not reach C (0 * Inf would be NaN)
    va = sr.sum_csr(rp, ci, a, 0.0, rp, ci, b, 1.0, 6)[2]
    assert np.array_equal(bits(va), bits(b))
    va = sr.sum_csr(rp, ci, a, 1.0, rp, ci, np.full(6, np.nan, np.float32), 0.0, 6)[2]
    assert np.array_equal(bits(va), bits(a))                                   # A's bits as they are, the NaN's payload too
    # every other coefficient multiplies, one rounding each: 0.1 * 3e38 twice, then one add
    va = sr.sum_csr(rp, ci, a, 0.1, rp, ci, b, 0.1, 6)[2]
    p = np.float32(0.1) * np.float32(3e38)
    assert bits(va[5:6])[0] == bits(f32(p + p))[0] and np.isnan(va[1])
    # a subnormal product is kept: 0.5 * 1e-40
    va = sr.sum_csr(rp, ci, f32(1e-40, 0, 0, 0, 0, 0), 0.5, i32(0, 0), i32(), f32(), 1.0, 6)[2]
    assert va[0] == np.float32(0.5) * np.float32(1e-40) and va[0] != 0
