"""CPU-side checks of the table matrices (sm_create_from_csr_ids, sm_build_opts.table_updatable,
sm_sddmm_table, sm_set_table, sm_axpy_table): the option's default and its validation run before
any device work, the Python mirror carries the new calls, and the numpy restatement of the
reduction order agrees with a brute-force float64 sum."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import table_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # SM_ERR_INVALID_ARG
INVALID_MATRIX = 6


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


RP = np.array([0, 2, 3], np.int32)
CI = np.array([0, 2, 1], np.int32)
VA = np.array([1.0, 2.0, 3.0], np.float32)
IDS = np.array([0, 1, 1], np.uint8)
TAB = np.array([1.0, 2.0], np.float32)


def _create_ex(lib, **opts):
    """sm_create_from_csr_ex on a 2 x 3 matrix with `opts`: (status, handle)."""
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    st = lib.sm_create_from_csr_ex(2, 3, 3, RP.ctypes.data, CI.ctypes.data, VA.ctypes.data, 0,
                                   C.byref(o), C.byref(h))
    return st, h


def _create_ids(lib, ids=IDS, table=TAB, **opts):
    from sparsematrix_amd import _lib
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    st = lib.sm_create_from_csr_ids(2, 3, 3, RP.ctypes.data, CI.ctypes.data, ids.ctypes.data,
                                    table.ctypes.data, int(table.size), 0, C.byref(o), C.byref(h))
    return st, h


def test_init_leaves_table_updatable_off(lib):
    from sparsematrix_amd import _lib
    o = _lib.SmBuildOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.sm_build_opts_init(C.byref(o))
    assert o.table_updatable == 0 and o.updatable == 0
    assert o.struct_size == C.sizeof(o)
    assert _lib.build_opts(table_updatable=1).table_updatable == 1


@pytest.mark.parametrize("bad", [2, -1])
def test_table_updatable_must_be_0_or_1(lib, bad):
    for st, h in (_create_ex(lib, table_updatable=bad), _create_ids(lib, table_updatable=bad)):
        assert st == INVALID and not h.value
        assert b"table_updatable" in lib.sm_last_error()


def test_only_the_table_constructors_honour_it(lib):
    """table_updatable = 1 through sm_create_from_csr_ex: refused by the option check, before any
    device work (so without a GPU)."""
    st, h = _create_ex(lib, table_updatable=1)
    assert st == INVALID and not h.value
    assert b"table_updatable" in lib.sm_last_error()


@pytest.mark.parametrize("opts", [dict(layout="exact"), dict(layout="blocked"), dict(layout="gather"),
                                  dict(layout="band2"), dict(layout="gcb"), dict(sell_codebook=0),
                                  dict(hot_cols=8), dict(merge_stage=1), dict(updatable=1)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_plain_form_options_are_rejected(lib, opts):
    st, h = _create_ids(lib, table_updatable=1, **opts)
    assert st == INVALID and not h.value
    assert b"table_updatable" in lib.sm_last_error()


def test_argument_checks_come_before_the_device(lib):
    st, h = _create_ids(lib, ids=np.array([0, 2, 1], np.uint8))   # an id >= T
    assert st == INVALID_MATRIX and not h.value
    assert b"ids[1]" in lib.sm_last_error()
    st, h = _create_ids(lib, table=np.zeros(0, np.float32))       # nnz > 0 needs T >= 1
    assert st == INVALID and not h.value
    assert lib.sm_sddmm_table(None, 0, 1.0, None, 1, None, 1, 0.0, None, 0, None) == INVALID
    assert b"n_rhs" in lib.sm_last_error()
    for st in (lib.sm_sddmm_table(None, 1, 1.0, None, 1, None, 1, 0.0, None, 0, None),
               lib.sm_set_table(None, None, None), lib.sm_axpy_table(None, 0.0, None, None),
               lib.sm_copy_table_device(None, None, None), lib.sm_copy_term_ids_device(None, None, None)):
        assert st == INVALID
        assert b"null matrix" in lib.sm_last_error()


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in ("sm_create_from_csr_ids", "sm_copy_table_device", "sm_copy_term_ids_device",
                 "sm_sddmm_table", "sm_set_table", "sm_axpy_table"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "table_updatable" in dict(_lib.SmInfo._fields_)
    assert _lib.SmInfo._fields_[-1][0] == "table_updatable"
    assert _lib.SmBuildOpts._fields_[-1][0] == "table_updatable"
    import sparsematrix_amd as smd
    sig = lambda f: list(inspect.signature(f).parameters)
    S = smd.SparseMatrix
    assert sig(S.from_csr_ids) == ["row_ptr", "col_idx", "ids", "table", "n_cols", "device", "opts"]
    assert sig(S.table_device)[1:] == ["stream"] and sig(S.term_ids_device)[1:] == ["stream"]
    assert sig(S.sddmm_table)[1:] == ["G", "X", "out", "alpha", "beta", "algo", "stream"]
    assert sig(S.set_table)[1:] == ["t", "stream"]
    assert sig(S.axpy_table)[1:] == ["a", "delta", "stream"]
    from sparsematrix_amd import autograd
    assert sig(autograd.apply_table) == ["matrix", "X", "alpha", "table", "values"]
    assert sig(autograd.apply) == ["matrix", "X", "alpha", "values"]


def test_values_and_table_together_raise():
    from sparsematrix_amd import autograd
    with pytest.raises(ValueError, match="values= and table="):
        autograd.apply_table(None, None, 1.0, values=object(), table=object())


def test_restatement_against_brute_force():
    """5000 random terms (three chunks, the last of 904), T = 7 with one id unused: the float32
    restatement is within its own rounding count of the float64 sum, and -0.0 where an id has
    no term."""
    rng = np.random.default_rng(3)
    n, T = 5000, 7
    ids = rng.integers(0, T - 1, n).astype(np.uint8)   # id 6 has no term
    d = rng.uniform(-1, 1, n).astype(np.float32)
    p = table_ref.chunk_partials(d, ids, T)
    assert p.shape == (3, T) and p.dtype == np.float32
    got = table_ref.reduce_by_id(d, ids, T, np.zeros(T, np.float32), 1.0, 1.0)
    want = table_ref.brute_by_id(d, ids, T)
    absum = np.bincount(ids, np.abs(d.astype(np.float64)), T)
    most = max(np.bincount(ids[k:k + 2048], minlength=T).max() for k in range(0, n, 2048))
    bound = (most + 3 + 2) * 2.0 ** -24 * absum
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
    assert np.all(np.signbit(p[:, 6])) and np.all(p[:, 6] == 0)
    # the order is the stated one: a single chunk and one id is a plain left-to-right sum from -0.0
    one = table_ref.reduce_by_id(d[:100], np.zeros(100, np.uint8), 1, np.zeros(1, np.float32), 1.0, 1.0)
    acc = np.float32(-0.0)
    for v in d[:100]:
        acc = np.float32(acc + v)
    assert one[0] == acc
    # alpha, beta: fl(fl(beta * out0) + fl(alpha * S))
    out0 = rng.uniform(-1, 1, T).astype(np.float32)
    ab = table_ref.reduce_by_id(d, ids, T, out0, -0.7, 0.5)
    S = table_ref.reduce_by_id(d, ids, T, np.zeros(T, np.float32), 1.0, 1.0)
    S[6] = np.float32(-0.0)
    assert np.array_equal(ab, (np.float32(0.5) * out0 + np.float32(-0.7) * S).astype(np.float32))
