"""CPU restatements of sm_sddmm for the tests: the SM_ALGO_PARITY order in numpy float32
(bit-exact target) and the float64 value with the sum of the terms' magnitudes (the bound).

    out[e] = alpha * sum_j G[r_e, j] * X[c_e, j] + beta * out0[e]      for every term e, CSR order
"""
from __future__ import annotations

import numpy as np

# Terms one workgroup of the vector kernel takes (kSddmmChunk, sparsematrix_amd/csrc/sm_internal.h).
CHUNK = 2048

GRID_N = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 257)
GRID_AB = ((1.3, 0.0), (1.3, 1.0), (-0.7, 0.5))


def term_rows(rp) -> np.ndarray:
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def as_2d(a) -> np.ndarray:
    a = np.asarray(a)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def parity(rp, ci, G, X, out0, alpha, beta) -> np.ndarray:
    """The header's PARITY order, every operation rounded to float32 on its own:
    s = G[r,0]*X[c,0]; s = s + G[r,j]*X[c,j] (j = 1..); t = alpha*s; out = out0 + t if beta == 1
    else beta*out0 + t.  Vectorised over the terms, a loop over j."""
    G = as_2d(np.asarray(G, np.float32))
    X = as_2d(np.asarray(X, np.float32))
    r, c = term_rows(rp), np.asarray(ci, np.int64)
    a, b = np.float32(alpha), np.float32(beta)
    with np.errstate(invalid="ignore", over="ignore"):
        s = G[r, 0] * X[c, 0]
        for j in range(1, G.shape[1]):
            s = s + G[r, j] * X[c, j]
        t = a * s
        o = np.asarray(out0, np.float32).reshape(-1)
        o = o if beta == 1.0 else b * o
        res = o + t
    assert res.dtype == np.float32
    return res


def exact(rp, ci, G, X, out0, alpha, beta):
    """(value, absum) in float64: absum = |alpha| * sum_j |G*X| + |beta * out0|."""
    G = as_2d(np.asarray(G, np.float64))
    X = as_2d(np.asarray(X, np.float64))
    r, c = term_rows(rp), np.asarray(ci, np.int64)
    a, b = float(np.float32(alpha)), float(np.float32(beta))
    o = np.asarray(out0, np.float64).reshape(-1)
    prod = G[r] * X[c]
    with np.errstate(invalid="ignore"):
        val = a * prod.sum(1) + b * o
        absum = abs(a) * np.abs(prod).sum(1) + np.abs(b * o)
    return val, absum


def grid_inputs(n_rows: int, n_cols: int, nnz: int, N: int, seed: int = 500):
    """(G, X, out0) for an n_rows x n_cols matrix and N right-hand sides: uniform [-1, 1) float32,
    one fixed stream per N."""
    rng = np.random.default_rng(seed + N)
    G = rng.uniform(-1, 1, (n_rows, N)).astype(np.float32)
    X = rng.uniform(-1, 1, (n_cols, N)).astype(np.float32)
    out0 = rng.uniform(-1, 1, nnz).astype(np.float32)
    return G, X, out0
