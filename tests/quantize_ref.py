"""Numpy restatements of the quantiser's contracts in include/sparsematrix.h (sm_quantize_assign,
sm_quantize_update, sm_create_quantized), step for step: the assignment rule on np.unique /
np.searchsorted, the chunked double sums as sequential np.cumsum (one IEEE add per term, in order),
the linear start and the whole Lloyd loop.  The GPU tests compare against these bit for bit.
"""
from __future__ import annotations

import numpy as np

CHUNK = 2048   # kSddmmChunk


def candidates(table):
    """Step 1: (values ascending, lowest t of each).  NaN entries dropped, the rest compared as
    floats (-0.0 = +0.0), each distinct value represented by its lowest t."""
    tb = np.asarray(table, np.float32).reshape(-1)
    t = np.arange(tb.size)
    keep = ~np.isnan(tb)
    vals = tb[keep] + np.float32(0.0)            # -0.0 -> +0.0: one value
    uniq, first = np.unique(vals, return_index=True)   # first occurrence = lowest t
    return uniq.astype(np.float32), t[keep][first].astype(np.int64)


def assign(val, table) -> np.ndarray:
    """Steps 2-5 for every value: uint8 ids."""
    v = np.asarray(val, np.float32).reshape(-1)
    cand, cid = candidates(table)
    ids = np.zeros(v.size, np.uint8)
    if cand.size == 0 or v.size == 0:
        return ids                                # step 5: no candidate at all
    nan = np.isnan(v)
    c = np.searchsorted(cand, np.where(nan, np.float32(0), v), side="right")   # candidates <= v
    has_lo, has_hi = c > 0, c < cand.size
    lo_i, hi_i = np.maximum(c - 1, 0), np.minimum(c, cand.size - 1)
    lo, hi = cand[lo_i], cand[hi_i]
    with np.errstate(invalid="ignore", over="ignore"):
        dl = (v - lo).astype(np.float32)          # fl32(v - lo)
        dh = (hi - v).astype(np.float32)          # fl32(hi - v)
    assert dl.dtype == np.float32 and dh.dtype == np.float32
    tl, th = cid[lo_i], cid[hi_i]
    take_hi = (dh < dl) | ((dh == dl) & (th < tl))                    # step 4
    pick = np.where(has_lo & has_hi, np.where(take_hi, th, tl), np.where(has_lo, tl, th))   # step 3
    pick[nan] = 0                                                      # step 5
    return pick.astype(np.uint8)


def _seq_sum(x) -> np.float64:
    """x[0], x[1], ... added one at a time in double, from +0.0."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(np.concatenate([[0.0], np.asarray(x, np.float64)]))[-1]


def update(val, ids, table):
    """(new table, counts, sse) by steps 1-5 of sm_quantize_update."""
    v = np.asarray(val, np.float32).reshape(-1).astype(np.float64)
    ids = np.asarray(ids, np.uint8).reshape(-1)
    old = np.asarray(table, np.float32).reshape(-1)
    T = old.size
    assert ids.size == v.size and (ids.size == 0 or int(ids.max()) < T)
    n_chunks = -(-v.size // CHUNK)
    p = np.zeros((n_chunks, T), np.float64)       # +0.0 where an id has no term in the chunk
    c = np.zeros((n_chunks, T), np.int64)
    q = np.zeros(n_chunks, np.float64)
    for k in range(n_chunks):
        vk, ik = v[k * CHUNK:(k + 1) * CHUNK], ids[k * CHUNK:(k + 1) * CHUNK]
        order = np.argsort(ik, kind="stable")     # by id, ascending e within an id
        sv, si = vk[order], ik[order]
        present = np.unique(si)
        start = np.searchsorted(si, present, side="left")
        end = np.searchsorted(si, present, side="right")
        for t, a, b in zip(present, start, end):
            p[k, t] = _seq_sum(sv[a:b])
            c[k, t] = b - a
        with np.errstate(invalid="ignore", over="ignore"):
            d = vk - old[ik].astype(np.float64)
            q[k] = _seq_sum(d * d)                # each square rounded once
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.cumsum(np.concatenate([np.zeros((1, T)), p]), axis=0)[-1]   # ascending k, from +0.0
    n = c.sum(axis=0)
    new = old.copy()                              # n[t] == 0: the entry keeps its bits
    live = n > 0
    with np.errstate(invalid="ignore", over="ignore"):
        new[live] = (S[live] / n[live].astype(np.float64)).astype(np.float32)
    return new, n.astype(np.int32), np.float64(_seq_sum(q))


def linear_table(val, T: int) -> np.ndarray:
    """The linear start of sm_create_quantized (all zeros without a value)."""
    v = np.asarray(val, np.float32).reshape(-1)
    lo = np.float64(v.min()) + 0.0 if v.size else np.float64(0.0)   # a zero bound counts as +0.0
    hi = np.float64(v.max()) + 0.0 if v.size else np.float64(0.0)
    if T == 1:
        return np.array([(lo + hi) / 2], np.float64).astype(np.float32)
    t = np.arange(T, dtype=np.float64)
    return (lo + (hi - lo) * (t / np.float64(T - 1))).astype(np.float32)


def lloyd(val, T: int, iters: int, init=None):
    """(ids, table) of sm_create_quantized: `iters` times assign then update, one last assign."""
    table = linear_table(val, T) if init is None else np.asarray(init, np.float32).copy()
    assert table.size == T
    for _ in range(iters):
        table, _, _ = update(val, assign(val, table), table)
    return assign(val, table), table


def brute_assign(val, table):
    """Float64 argmin over all entries (lowest t on exact ties), with the two best distinct
    distances per value: the check of the rule itself."""
    v = np.asarray(val, np.float64).reshape(-1, 1)
    tb = np.asarray(table, np.float64).reshape(1, -1)
    d = np.abs(v - tb)
    d[:, np.isnan(tb[0])] = np.inf
    best = d.argmin(axis=1)
    ds = np.sort(d, axis=1)
    return best.astype(np.uint8), ds[:, 0], d
