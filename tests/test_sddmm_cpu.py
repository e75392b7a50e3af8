"""CPU-side checks of the SDDMM surface (no GPU compute): the float32 restatement the GPU tests
compare against sits inside the project's bound on their inputs, the new entry points reject
bad arguments before touching a device, and the Python mirror carries the new calls."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import sddmm_ref
from gpu_util import assert_terms_close, uniform_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", ROOT, "-j", "8"], check=True)
    from sparsematrix_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("N", sddmm_ref.GRID_N)
def test_float32_restatement_is_inside_the_bound(N):
    """The GPU grid's inputs (tests/test_gpu_sddmm.py): sequential float32 against float64."""
    rp, ci, _ = uniform_csr(300, 257, 6, seed=501)
    G, X, out0 = sddmm_ref.grid_inputs(300, 257, ci.size, N)
    for alpha, beta in sddmm_ref.GRID_AB:
        got = sddmm_ref.parity(rp, ci, G, X, out0, alpha, beta)
        want, absum = sddmm_ref.exact(rp, ci, G, X, out0, alpha, beta)
        assert got.shape == (ci.size,)
        assert_terms_close(got, want, absum)


def test_restatement_order_is_sequential():
    """One term by hand: the j loop left to right, alpha last, beta by multiplication."""
    rp, ci = np.array([0, 1], np.int32), np.array([0], np.int32)
    g = np.array([[1.0, 2.0 ** -24, 2.0 ** -24]], np.float32)
    x = np.ones((1, 3), np.float32)
    # (1 + 2^-24) rounds back to 1 (ties to even) twice; a tree would give 1 + 2^-23
    assert sddmm_ref.parity(rp, ci, g, x, np.zeros(1, np.float32), 1.0, 0.0)[0] == np.float32(1.0)
    nan = sddmm_ref.parity(rp, ci, g, x, np.array([np.nan], np.float32), 1.0, 0.0)
    assert np.isnan(nan[0])   # beta = 0 multiplies


def test_invalid_arguments_without_a_device(lib):
    INVALID = 1   # SM_ERR_INVALID_ARG
    assert lib.sm_sddmm(None, 4, 1.0, None, 4, None, 4, 0.0, None, 0, None) == INVALID
    # n_rhs = 0 is rejected before the matrix is looked at (the placeholder is never read)
    assert lib.sm_sddmm(C.c_void_p(16), 0, 1.0, None, 4, None, 4, 0.0, None, 0, None) == INVALID
    assert lib.sm_sddmm(None, 0, 1.0, None, 4, None, 4, 0.0, None, 0, None) == INVALID
    assert lib.sm_sddmm(C.c_void_p(16), -1, 1.0, None, 4, None, 4, 0.0, None, 1, None) == INVALID
    assert lib.sm_copy_csr_device(None, None, None, None, None) == INVALID
    assert b"null matrix" in lib.sm_last_error()


def test_exports_and_python_surface(lib):
    from sparsematrix_amd import _lib
    for name in ("sm_sddmm", "sm_copy_csr_device"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    import sparsematrix_amd as smd
    for name in ("sddmm", "csr_device"):
        assert hasattr(smd.SparseMatrix, name), name
    sig = inspect.signature(smd.SparseMatrix.sddmm)
    assert list(sig.parameters)[1:] == ["G", "X", "out", "alpha", "beta", "algo", "stream"]
    assert sig.parameters["alpha"].default == 1.0 and sig.parameters["beta"].default == 0.0


def test_autograd_apply_accepts_values():
    from sparsematrix_amd import autograd
    sig = inspect.signature(autograd.apply)
    assert list(sig.parameters) == ["matrix", "X", "alpha", "values"]
    assert sig.parameters["values"].default is None and sig.parameters["alpha"].default == 1.0
