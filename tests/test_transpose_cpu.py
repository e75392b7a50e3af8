"""CPU-side checks of the transposed-matrix surface (no GPU compute): the library exports
sm_create_transpose and rejects null arguments before touching a device, and the Python
mirror carries the transposed calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "sparsematrix_amd", "libsparsematrix_amd.so")


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


def test_library_exports_sm_create_transpose(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True).stdout
    assert "sm_create_transpose" in set(re.findall(r" T (\w+)$", out, flags=re.M))
    assert hasattr(lib, "sm_create_transpose")
    from sparsematrix_amd import _lib
    assert "sm_create_transpose" in _lib.EXPORTS


def test_null_arguments_without_a_device(lib):
    h = C.c_void_p(1)
    assert lib.sm_create_transpose(None, None, None, C.byref(h)) == 1   # SM_ERR_INVALID_ARG
    assert not h.value   # *out is cleared
    assert lib.sm_create_transpose(None, None, None, None) == 1
    # a null `out` is rejected before `src` is looked at (a non-null placeholder is never read)
    assert lib.sm_create_transpose(C.c_void_p(16), None, None, None) == 1


def test_python_surface():
    import sparsematrix_amd as smd
    for name in ("transposed", "T", "spmv_t", "spmm_t"):
        assert hasattr(smd.SparseMatrix, name), name
    assert isinstance(smd.SparseMatrix.T, property)


def test_autograd_imports():
    import sparsematrix_amd
    from sparsematrix_amd import autograd
    assert callable(autograd.apply)
    assert sparsematrix_amd.autograd is autograd
