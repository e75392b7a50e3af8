"""CPU-side checks of the in-place value updates (sm_build_opts.updatable, sm_set_values,
sm_axpy_values): the option's default and its validation run before any device work, and the
Python mirror carries the new calls."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # SM_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def _create(lib, **opts):
    """sm_create_from_csr_ex on a 2 x 3 matrix with `opts`: (status, handle)."""
    from sparsematrix_amd import _lib
    rp = np.array([0, 2, 3], np.int32)
    ci = np.array([0, 2, 1], np.int32)
    va = np.array([1.0, 2.0, 3.0], np.float32)
    o = _lib.build_opts(**opts)
    h = C.c_void_p()
    st = lib.sm_create_from_csr_ex(2, 3, 3, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 0,
                                   C.byref(o), C.byref(h))
    return st, h


def test_init_leaves_updatable_off(lib):
    from sparsematrix_amd import _lib
    o = _lib.SmBuildOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.sm_build_opts_init(C.byref(o))
    assert o.updatable == 0
    assert o.struct_size == C.sizeof(o)
    assert _lib.build_opts(updatable=1).updatable == 1


def test_updatable_must_be_0_or_1(lib):
    for bad in (2, -1):
        st, h = _create(lib, updatable=bad)
        assert st == INVALID and not h.value
        assert b"updatable" in lib.sm_last_error()


@pytest.mark.parametrize("opts", [dict(layout="cband"), dict(layout="sweep"), dict(hot_cols=8),
                                  dict(merge_stage=1)],
                         ids=["cband", "sweep", "hot_cols", "merge_stage"])
def test_codebook_only_options_are_rejected(lib, opts):
    """What exists only in codebook form cannot be updatable: rejected by the option check,
    before any device work (so without a GPU)."""
    st, h = _create(lib, updatable=1, **opts)
    assert st == INVALID and not h.value
    assert b"updatable" in lib.sm_last_error()


def test_null_matrix(lib):
    assert lib.sm_set_values(None, None, 0, None) == INVALID
    assert b"null matrix" in lib.sm_last_error()
    assert lib.sm_axpy_values(None, 1.0, None, 0, None) == INVALID
    assert lib.sm_axpy_values(None, 0.0, None, 1, None) == INVALID


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in ("sm_set_values", "sm_axpy_values"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert (_lib.SM_VALUES_OWN, _lib.SM_VALUES_SOURCE) == (0, 1)
    assert "updatable" in dict(_lib.SmInfo._fields_) and "updatable" in dict(_lib.SmBuildOpts._fields_)
    import sparsematrix_amd as smd
    assert list(inspect.signature(smd.SparseMatrix.set_values).parameters)[1:] == ["val", "stream"]
    assert list(inspect.signature(smd.SparseMatrix.axpy_values).parameters)[1:] == ["a", "delta", "stream"]
