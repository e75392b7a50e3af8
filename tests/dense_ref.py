"""The numpy restatement of sm_create_from_dense_device (include/sparsematrix.h), on top of
prune_ref: the dense matrix stands for the full CSR in which every element is a stored term (term
index i = r * n_cols + c, columns ascending, zeros included); sm_prune_mask's rule selects, and the
kept terms in stored order are the result.

full_csr(n_rows, n_cols)   (rp, ci) of that full matrix.
select(W, mode, ...)       (rp, ci, va, keep): the compacted arrays and the mask over i.
"""
from __future__ import annotations

import numpy as np

import prune_ref as pr


def full_csr(n_rows: int, n_cols: int):
    rp = np.arange(n_rows + 1, dtype=np.int64) * n_cols
    ci = np.tile(np.arange(n_cols, dtype=np.int32), n_rows)
    return rp, ci


def select(W, mode: int, count: int = 0, threshold: float = 0.0):
    W = np.ascontiguousarray(W, np.float32)
    assert W.ndim == 2
    rp, ci = full_csr(*W.shape)
    keep = pr.mask(rp, W.reshape(-1), mode, count, threshold)
    n_rp, n_ci, n_va, _, _ = pr.compact(rp, ci, W.reshape(-1), keep)
    return n_rp, n_ci, n_va, keep
