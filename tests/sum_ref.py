"""The numpy restatement of sm_create_sum's rule (include/sparsematrix.h): the union pattern and
the source maps on integers, the values with one float32 operation per rounding, so the GPU tests
compare bit for bit (NaN results as NaN).  No torch and no GPU at import.

union(...)   (rp_c, ci_c, terms_a, terms_b): row r of C holds the union of the columns of row r of
             A and of B, ascending, each once; terms_x[e] = the CSR index of that position in X, -1
             where X does not store it.  Positions are compared as row * n_cols + column.
values(...)  the value of every term of C: a contribution is absent where the operand does not
             store the position or its coefficient is 0 (its values are then not read), the
             value's bits where the coefficient is 1, fl(coef * value) otherwise; two
             contributions give fl(pa + pb), one its bits, none +0.0.
sum_csr(...) both: (rp_c, ci_c, va_c, terms_a, terms_b).
"""
from __future__ import annotations

import numpy as np


def _keys(rp, ci, n_cols: int) -> np.ndarray:
    """row * max(n_cols, 1) + column of every term, strictly ascending over the whole matrix."""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64).reshape(-1)
    assert rp[0] == 0 and rp[-1] == ci.size and (np.diff(rp) >= 0).all()
    assert ci.size == 0 or (ci.min() >= 0 and ci.max() < n_cols)
    k = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)) * max(int(n_cols), 1) + ci
    assert (np.diff(k) > 0).all(), "every row's columns must strictly ascend"
    return k


def _terms(k_x: np.ndarray, k_c: np.ndarray) -> np.ndarray:
    """For every position of C its index in X, or -1."""
    if k_x.size == 0:
        return np.full(k_c.size, -1, np.int32)
    i = np.searchsorted(k_x, k_c)
    found = (i < k_x.size) & (k_x[np.minimum(i, k_x.size - 1)] == k_c)
    return np.where(found, i, -1).astype(np.int32)


def union(rp_a, ci_a, rp_b, ci_b, n_cols: int):
    n_rows = np.asarray(rp_a).size - 1
    assert np.asarray(rp_b).size - 1 == n_rows
    k_a, k_b = _keys(rp_a, ci_a, n_cols), _keys(rp_b, ci_b, n_cols)
    k_c = np.union1d(k_a, k_b)                       # sorted, each position once
    w = max(int(n_cols), 1)
    rp_c = np.searchsorted(k_c, np.arange(n_rows + 1, dtype=np.int64) * w).astype(np.int32)
    ci_c = (k_c % w).astype(np.int32)
    return rp_c, ci_c, _terms(k_a, k_c), _terms(k_b, k_c)


def _contribution(v, terms: np.ndarray, coef: float):
    """(present, bits): the operand's contribution to every term of C as uint32 bits."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    coef = np.float32(coef)
    present = (terms >= 0) if coef != 0 else np.zeros(terms.size, bool)
    p = np.zeros(terms.size, np.float32)
    if present.any():                                # coef == 0: v is never indexed
        src = v[terms[present]]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            p[present] = src if coef == 1 else coef * src
    return present, p.view(np.uint32)


def values(va_a, alpha: float, terms_a, va_b, beta: float, terms_b) -> np.ndarray:
    has_a, pa = _contribution(va_a, np.asarray(terms_a), alpha)
    has_b, pb = _contribution(va_b, np.asarray(terms_b), beta)
    out = np.zeros(pa.size, np.uint32)               # none present: +0.0
    out[has_a & ~has_b] = pa[has_a & ~has_b]
    out[has_b & ~has_a] = pb[has_b & ~has_a]
    both = has_a & has_b
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        out[both] = (pa[both].view(np.float32) + pb[both].view(np.float32)).astype(np.float32).view(np.uint32)
    return out.view(np.float32)


def sum_csr(rp_a, ci_a, va_a, alpha, rp_b, ci_b, va_b, beta, n_cols: int):
    rp_c, ci_c, ta, tb = union(rp_a, ci_a, rp_b, ci_b, n_cols)
    return rp_c, ci_c, values(va_a, alpha, ta, va_b, beta, tb), ta, tb
