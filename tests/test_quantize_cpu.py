"""CPU-side checks of the quantiser (sm_create_from_csr_ids_device, sm_quantize_assign,
sm_quantize_update, sm_create_quantized): the library exports the calls and the Python mirror
carries them, the argument checks run before any device work, and the numpy restatement the GPU
tests compare against follows the header -- against a brute-force float64 argmin, on hand-made tie
cases, and against np.bincount."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import quantize_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # SM_ERR_INVALID_ARG
NEW = ("sm_create_from_csr_ids_device", "sm_quantize_assign", "sm_quantize_update", "sm_create_quantized")
P = 64        # stands for a device pointer: the checks below return before any is read


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def _ids_device(lib, nnz=3, rp=P, ci=P, ids=P, table=P, T=2, **opts):
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    st = lib.sm_create_from_csr_ids_device(2, 3, nnz, rp, ci, ids, table, T, 0, None, C.byref(o), C.byref(h))
    return st, h


def _quantized(lib, T=5, iters=1, **opts):
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    return lib.sm_create_quantized(None, T, iters, None, C.byref(o), None, C.byref(h)), h


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    import sparsematrix_amd as smd
    sig = lambda f: list(inspect.signature(f).parameters)
    S = smd.SparseMatrix
    assert sig(S.from_csr_ids_device) == ["row_ptr", "col_idx", "ids", "table", "n_cols", "device", "opts", "stream"]
    assert sig(S.quantize_assign)[1:] == ["table", "stream"]
    assert sig(S.quantize_update)[1:] == ["ids", "table", "stream"]
    assert sig(S.quantized)[1:] == ["table_size", "iters", "init", "opts", "stream"]
    d = inspect.signature(S.quantized).parameters
    assert d["table_size"].default == 255 and d["iters"].default == 8 and d["init"].default is None


def test_device_constructor_checks_come_before_the_device(lib):
    for T in (0, 256, -1):     # nnz > 0 needs T in [1, 255]
        st, h = _ids_device(lib, T=T)
        assert st == INVALID and not h.value and b"table_size" in lib.sm_last_error()
    for null in ("rp", "ci", "ids"):
        st, h = _ids_device(lib, **{null: None})
        assert st == INVALID and not h.value and b"null CSR array" in lib.sm_last_error()
    st, h = _ids_device(lib, table=None)
    assert st == INVALID and not h.value and b"null table" in lib.sm_last_error()
    st, h = _ids_device(lib, table_updatable=2)
    assert st == INVALID and b"table_updatable" in lib.sm_last_error()
    st, h = _ids_device(lib, table_updatable=1, layout="band2")   # check_opts(opts, true), as on the host
    assert st == INVALID and b"table_updatable" in lib.sm_last_error()
    assert lib.sm_create_from_csr_ids_device(2, 3, 3, P, P, P, P, 2, 0, None, None, None) == INVALID


def test_quantizer_checks_come_before_the_device(lib):
    for T in (0, 256):
        assert lib.sm_quantize_assign(None, P, T, P, None) == INVALID and b"table_size" in lib.sm_last_error()
        assert lib.sm_quantize_update(None, P, T, P, None, None, None) == INVALID
        assert b"table_size" in lib.sm_last_error()
        st, h = _quantized(lib, T=T)
        assert st == INVALID and not h.value and b"table_size" in lib.sm_last_error()
    st, h = _quantized(lib, iters=-1)
    assert st == INVALID and not h.value and b"iters" in lib.sm_last_error()
    for st in (lib.sm_quantize_assign(None, P, 5, P, None), lib.sm_quantize_update(None, P, 5, P, None, None, None),
               _quantized(lib)[0]):
        assert st == INVALID and b"null matrix" in lib.sm_last_error()
    assert lib.sm_create_quantized(None, 5, 1, None, None, None, None) == INVALID


def test_updatable_is_refused_by_the_new_constructors(lib):
    st, h = _ids_device(lib, updatable=1)
    assert st == INVALID and not h.value and b"updatable" in lib.sm_last_error()
    st, h = _quantized(lib, updatable=1)
    assert st == INVALID and not h.value and b"updatable" in lib.sm_last_error()
    st, h = _quantized(lib, updatable=1, table_updatable=1)
    assert st == INVALID and not h.value


# ------------------------------------------------------------------ the restatement itself
def _check_against_brute(v, table):
    got = qr.assign(v, table)
    tb = np.asarray(table, np.float64)
    d = np.abs(v.astype(np.float64)[:, None] - tb[None, :])
    d[:, np.isnan(tb)] = np.inf
    best = d.argmin(axis=1)                                   # lowest t on exact ties
    d1 = d[np.arange(v.size), best]
    other = tb[None, :] != tb[best][:, None]                  # entries of another value
    d2 = np.where(other, d, np.inf).min(axis=1)
    clear = d1 < d2 * (1 - 2.0 ** -23)                        # more than 2^-23 relative apart (d2 = inf: T = 1)
    assert clear.mean() > 0.99
    assert np.array_equal(got[clear], best[clear].astype(np.uint8))
    # and otherwise one of the two nearest values, which are then that close to each other
    dg = d[np.arange(v.size), got]
    assert np.all(dg <= d1 * (1 + 2.0 ** -22))


def test_assignment_is_the_nearest_entry():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, 20000).astype(np.float32)
    _check_against_brute(v, rng.uniform(-1, 1, 255).astype(np.float32))
    t7 = rng.uniform(-1, 1, 7).astype(np.float32)
    t7[5] = t7[2]                                             # unsorted, with a duplicate
    _check_against_brute(v, t7)
    _check_against_brute(v, np.array([0.3], np.float32))
    tn = rng.uniform(-1, 1, 16).astype(np.float32)
    tn[3] = np.nan
    _check_against_brute(v, tn)
    assert not np.any(qr.assign(v, tn) == 3)


TIE_TABLE = np.array([0.5, -0.0, 0.5, np.nan, 0.0, -1.0, 0.25], np.float32)
TIE_CASES = [(0.5, 0), (0.7, 0), (-3.0, 5), (0.0, 1), (-0.0, 1), (0.375, 0), (0.125, 1), (-0.5, 1),
             (np.nan, 0), (np.inf, 0), (-np.inf, 5), (0.3, 6)]


def test_tie_rule_on_hand_made_cases():
    """Duplicates (0.5 at t = 0 and 2), -0.0 / +0.0 (t = 1 and 4), a NaN entry (t = 3), v below and
    above every entry, and v exactly midway: 0.375 between 0.25 (t = 6) and 0.5 (t = 0) takes the
    upper one because t_hi < t_lo, 0.125 between 0.0 (t = 1) and 0.25 (t = 6) the lower one."""
    cand, cid = qr.candidates(TIE_TABLE)
    assert cand.tolist() == [-1.0, 0.0, 0.25, 0.5] and cid.tolist() == [5, 1, 6, 0]
    v = np.array([c[0] for c in TIE_CASES], np.float32)
    assert qr.assign(v, TIE_TABLE).tolist() == [c[1] for c in TIE_CASES]
    assert qr.assign(v, np.full(4, np.nan, np.float32)).tolist() == [0] * v.size   # no candidate at all


def test_means_agree_with_bincount():
    rng = np.random.default_rng(6)
    n, T = 5000, 7                                            # three chunks, the last of 904
    v = rng.uniform(-1, 1, n).astype(np.float32)
    ids = rng.integers(0, T - 1, n).astype(np.uint8)          # id 6 has no term
    old = rng.uniform(-1, 1, T).astype(np.float32)
    new, counts, sse = qr.update(v, ids, old)
    assert new.dtype == np.float32 and counts.dtype == np.int32
    want_n = np.bincount(ids, minlength=T)
    want = np.bincount(ids, v.astype(np.float64), T)[:6] / want_n[:6]
    assert np.array_equal(counts, want_n)
    assert np.all(np.abs(new[:6].astype(np.float64) - want) <= 1e-12 * np.abs(want) + 2.0 ** -24 * np.abs(want))
    mean64 = qr._seq_sum(v[ids == 2]) / want_n[2]
    assert abs(mean64 - want[2]) <= 1e-12 * abs(want[2])      # the double sums themselves
    assert new[2] == np.float32(mean64)
    assert new[6].view(np.uint32) == old[6].view(np.uint32)   # the empty cluster keeps its entry
    want_sse = float(np.sum((v.astype(np.float64) - old[ids].astype(np.float64)) ** 2))
    assert abs(float(sse) - want_sse) <= 1e-12 * want_sse
    # a single chunk and one id: a plain left-to-right double sum from +0.0
    one, c1, _ = qr.update(v[:100], np.zeros(100, np.uint8), np.zeros(1, np.float32))
    acc = 0.0
    for x in v[:100]:
        acc += float(x)
    assert one[0] == np.float32(acc / 100) and c1[0] == 100
    # no term at all: the table as it was, counts 0, sse 0.0
    e_new, e_n, e_sse = qr.update(np.zeros(0, np.float32), np.zeros(0, np.uint8), old)
    assert np.array_equal(e_new.view(np.uint32), old.view(np.uint32)) and not e_n.any() and e_sse == 0.0


def test_linear_start_and_loop():
    v = np.array([-0.0, 0.5, 2.0, 1.0], np.float32)
    assert qr.linear_table(v, 5).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert not np.signbit(qr.linear_table(v, 5)[0])           # a zero minimum counts as +0.0
    assert qr.linear_table(v, 1).tolist() == [1.0]
    assert qr.linear_table(np.zeros(0, np.float32), 3).tolist() == [0.0, 0.0, 0.0]
    rng = np.random.default_rng(8)
    w = rng.normal(0, 0.3, 6000).astype(np.float32)
    sse = []
    for it in (0, 1, 4):
        ids, tab = qr.lloyd(w, 16, it)
        assert np.array_equal(ids, qr.assign(w, tab))         # the ids are those of the final table
        sse.append(float(np.sum((w.astype(np.float64) - tab[ids]) ** 2)))
    assert sse[0] > sse[1] > sse[2]                           # Lloyd steps do not increase the error
