"""CPU restatements for the table-matrix tests (sm_sddmm_table, sm_set_table, sm_axpy_table).

reduce_by_id restates steps 2-4 of the header's summation order from a given float32 array of
per-term dots `d` (what sm_sddmm returns with alpha = 1, beta = 0): plain loops over chunks of
2048 terms, every add done in np.float32.  exact_by_id is the float64 value with the per-id sum of
magnitudes and the header's rounding count R_t.  assert_same_matrix / Operands follow
test_gpu_update_values.py (the scheme "M after the update is what a fresh build gives").
"""
from __future__ import annotations

import numpy as np

from sddmm_ref import CHUNK, as_2d, term_rows

NEG0 = np.float32(-0.0)


def chunk_partials(d, ids, T: int) -> np.ndarray:
    """p[k][t]: the dots of chunk k's terms with id t, in ascending e, one add each, from -0.0."""
    d = np.asarray(d, np.float32).reshape(-1)
    ids = np.asarray(ids, np.uint8).reshape(-1)
    n_chunks = -(-d.size // CHUNK)
    p = np.full((n_chunks, T), NEG0, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(n_chunks):
            row = p[k]
            for e in range(k * CHUNK, min(d.size, (k + 1) * CHUNK)):
                t = ids[e]
                row[t] = np.float32(row[t] + d[e])
    return p


def finish_partials(p, out0, alpha, beta) -> np.ndarray:
    """Steps 3-4 from the per-chunk partials: the chunks in ascending k from -0.0, then
    out = fl(o + fl(alpha * S)), o = out0 if beta == 1 else fl(beta * out0)."""
    T = p.shape[1]
    S = np.full(T, NEG0, np.float32)
    a, b = np.float32(alpha), np.float32(beta)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(p.shape[0]):
            S = (S + p[k]).astype(np.float32)
        t = (a * S).astype(np.float32)
        o = np.asarray(out0, np.float32).reshape(-1)
        o = o if beta == 1.0 else (b * o).astype(np.float32)
        res = (o + t).astype(np.float32)
    assert res.dtype == np.float32 and S.dtype == np.float32
    return res


def reduce_by_id(d, ids, T: int, out0, alpha, beta) -> np.ndarray:
    """Steps 2-4 of the header's order from the per-term dots `d`."""
    return finish_partials(chunk_partials(d, ids, T), out0, alpha, beta)


def r_dot(n_rhs: int, panel: bool) -> int:
    """sm_sddmm's rounding count of the dot itself (before alpha): n_rhs for the PARITY order
    (n_rhs products, n_rhs - 1 adds on one path: each term passes one product and at most
    n_rhs - 1 adds), 4T + log2 L for the vector kernel."""
    if not panel:
        return n_rhs
    L = 1
    while L < 64 and 4 * L < n_rhs:
        L *= 2
    tiles = -(-n_rhs // (4 * L))
    return 4 * tiles + int(np.log2(L))


def exact_by_id(rp, ci, ids, T: int, G, X, out0, alpha, beta, panel: bool):
    """(value, absum, R) per id in float64: absum = |alpha| * sum over the id's terms of
    sum_j |G*X| + |beta * out0|; R_t = R_dot + max_k |{e in chunk k: id_e = t}| + n_chunks + 2."""
    G = as_2d(np.asarray(G, np.float64))
    X = as_2d(np.asarray(X, np.float64))
    r, c = term_rows(rp), np.asarray(ci, np.int64)
    ids = np.asarray(ids, np.int64)
    a, b = float(np.float32(alpha)), float(np.float32(beta))
    prod = G[r] * X[c]
    dots = prod.sum(1)
    mags = np.abs(prod).sum(1)
    o = np.asarray(out0, np.float64).reshape(-1)
    val = a * np.bincount(ids, dots, T) + b * o
    absum = abs(a) * np.bincount(ids, mags, T) + np.abs(b * o)
    n_chunks = -(-ids.size // CHUNK)
    most = np.zeros(T, np.int64)
    for k in range(n_chunks):
        most = np.maximum(most, np.bincount(ids[k * CHUNK:(k + 1) * CHUNK], minlength=T))
    R = r_dot(G.shape[1], panel) + most + n_chunks + 2
    return val, absum, R


def brute_by_id(d, ids, T: int) -> np.ndarray:
    """Float64 sum of d per id, one Python loop: the check of the restatement itself."""
    s = [0.0] * T
    for e in range(len(d)):
        s[int(ids[e])] += float(d[e])
    return np.array(s, np.float64)


# ---- "the updated matrix is what a fresh build gives" (after test_gpu_update_values.py) ----
SPMV_ALGOS = ("auto", "parity", "stream", "vector", "xband", "sell", "merge", "exact")
ALPHA_BETA = ((1.0, 1.0), (1.3, 0.7), (0.5, 0.0))
SPECIAL_BITS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000,
                         0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)


def same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Operands:
    """One set of dense operands per shape, shared by every comparison of a case."""

    def __init__(self, n_rows, n_cols, seed=11):
        from gpu_util import to_dev
        rng = np.random.default_rng(seed)
        u = lambda *s: to_dev(rng.uniform(-1, 1, s).astype(np.float32))
        self.x, self.y0 = u(n_cols), u(n_rows)
        self.X = {n: u(n_cols, n) for n in (4, 32)}
        self.Y0 = {n: u(n_rows, n) for n in (4, 32)}
        self.G4 = u(n_rows, 4)


def assert_same_products(M, F, ops, tag=""):
    """CSR (values by bits), ==, digests and every product of M and F bit for bit."""
    from gpu_util import bits
    m_csr, f_csr = M.csr(), F.csr()
    assert np.array_equal(m_csr[0], f_csr[0]) and np.array_equal(m_csr[1], f_csr[1]), tag + " pattern"
    assert np.array_equal(bits(m_csr[2]), bits(f_csr[2])), tag + " CSR values (bits)"
    assert M == F, tag + " =="
    assert M.layout_digest() == F.layout_digest(), tag + " layout digest"
    for algo in SPMV_ALGOS:
        for alpha, beta in ALPHA_BETA:
            ym, yf = ops.y0.clone(), ops.y0.clone()
            M.spmv(ops.x, ym, alpha, beta, algo=algo)
            F.spmv(ops.x, yf, alpha, beta, algo=algo)
            assert same_bits(ym, yf), f"{tag} spmv {algo} alpha={alpha} beta={beta}"
    for n, algo in ((4, "auto"), (32, "auto"), (32, "mfma")):
        Ym, Yf = ops.Y0[n].clone(), ops.Y0[n].clone()
        M.spmm(ops.X[n], Ym, 1.3, 0.7, algo=algo)
        F.spmm(ops.X[n], Yf, 1.3, 0.7, algo=algo)
        assert same_bits(Ym, Yf), f"{tag} spmm N={n} {algo}"
    assert same_bits(M.sddmm(ops.G4, ops.X[4]), F.sddmm(ops.G4, ops.X[4])), tag + " sddmm"


def assert_same_matrix(M, F, ops, tag=""):
    """M is what F is (both table matrices): assert_same_products, the table, the ids and the
    table gradient."""
    from gpu_util import bits, to_host
    assert_same_products(M, F, ops, tag)
    assert np.array_equal(bits(to_host(M.table_device())), bits(to_host(F.table_device()))), tag + " table"
    assert np.array_equal(to_host(M.term_ids_device()), to_host(F.term_ids_device())), tag + " ids"
    assert same_bits(M.sddmm_table(ops.G4, ops.X[4]), F.sddmm_table(ops.G4, ops.X[4])), tag + " sddmm_table"


def axpy_reference(val, a, delta):
    """fl(val + fl(a * delta)) in float32 numpy: two separately rounded operations."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (val + (np.float32(a) * delta)).astype(np.float32)
