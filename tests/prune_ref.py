"""The numpy restatement of the pruning rules of include/sparsematrix.h (sm_prune_mask,
sm_create_masked): integers only, so the GPU tests compare bit for bit.

keys(v)       bits(v) & 0x7FFFFFFF as uint32: -0.0 ties with +0.0, subnormals order as their
              magnitudes, Inf beats every finite value, a NaN beats Inf.
mask(...)     the keep bytes of the three modes, by a stable argsort of the negated keys (key
              descending, CSR index ascending), over the whole matrix or within every row.
compact(...)  the kept terms in stored order with their row pointer and their source indices.
"""
from __future__ import annotations

import numpy as np

GLOBAL_TOPK, ROW_TOPK, THRESHOLD = 0, 1, 2


def keys(v) -> np.ndarray:
    b = np.ascontiguousarray(v, np.float32).reshape(-1).view(np.uint32)
    return b & np.uint32(0x7FFFFFFF)


def _top(k: np.ndarray, count: int) -> np.ndarray:
    """Indices of the first min(count, n) of (key descending, index ascending)."""
    order = np.argsort(-k.astype(np.int64), kind="stable")
    return order[:min(int(count), k.size)]


def mask(rp, v, mode: int, count: int = 0, threshold: float = 0.0) -> np.ndarray:
    """keep[e] in {0, 1} (uint8) for every term in CSR order."""
    k = keys(v)
    keep = np.zeros(k.size, np.uint8)
    if mode == GLOBAL_TOPK:
        assert count >= 0
        keep[_top(k, count)] = 1
    elif mode == ROW_TOPK:
        assert count >= 0
        rp = np.asarray(rp, np.int64)
        for r in range(rp.size - 1):
            a, b = int(rp[r]), int(rp[r + 1])
            keep[a + _top(k[a:b], count)] = 1
    elif mode == THRESHOLD:
        t = np.float32(threshold)
        assert not np.isnan(t) and (t > 0 or t == 0), "a NaN or negative threshold is an argument error"
        keep[k >= keys(t)[0]] = 1
    else:
        raise ValueError(f"unknown mode {mode}")
    return keep


def compact(rp, ci, v, keep, ids=None):
    """(rp', ci', v', ids', source_terms): the terms with keep[e] != 0 in stored order; ids' is
    None without ids; source_terms[j] = the CSR index in the source of kept term j (int32)."""
    rp = np.asarray(rp, np.int64)
    k = np.asarray(keep).reshape(-1) != 0
    pos = np.concatenate([[0], np.cumsum(k)])          # the exclusive scan over nnz + 1 positions
    new_rp = pos[rp].astype(np.int32)
    src = np.flatnonzero(k).astype(np.int32)
    new_ci = np.ascontiguousarray(np.asarray(ci, np.int32)[k])
    new_v = np.ascontiguousarray(np.asarray(v, np.float32)[k])
    new_ids = None if ids is None else np.ascontiguousarray(np.asarray(ids, np.uint8)[k])
    return new_rp, new_ci, new_v, new_ids, src
