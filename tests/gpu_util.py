"""Shared helpers for the -m gpu parity tests (device buffers via torch)."""
from __future__ import annotations

import numpy as np

TOL = 1e-6   # north_star: "within 1e-6 relative" -- defined against sum |terms|


def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a visible GPU"
    return torch


def to_dev(a: np.ndarray):
    torch = torch_dev()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def to_host(t) -> np.ndarray:
    torch = torch_dev()
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def assert_terms_close(got: np.ndarray, want: np.ndarray, absum: np.ndarray, tol: float = TOL):
    """|got - want| <= tol * sum|terms| elementwise (and NaN where want is NaN)."""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    absum = np.asarray(absum, np.float64).reshape(-1)
    nan_w = np.isnan(want)
    assert np.array_equal(nan_w, np.isnan(got)), "NaN pattern differs"
    ok = ~nan_w
    err = np.abs(got[ok] - want[ok])
    bound = tol * absum[ok] + 1e-37
    bad = err > bound
    assert not bad.any(), (f"{int(bad.sum())} elements out of bound; worst ratio "
                           f"{float((err / bound).max()):.3g}")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


GUARD_BITS = 0x7FC0DEAD   # a quiet NaN no kernel computes: guard words and padding columns


def _guarded_parent(n_elems: int):
    torch = torch_dev()
    parent = torch.empty(n_elems, dtype=torch.float32, device="cuda")
    parent.view(torch.int32).fill_(GUARD_BITS)
    assert parent.data_ptr() % 256 == 0, "allocation base not 256-byte aligned"
    return parent


def placed(vec, off: int, guard: int = 8):
    """(view, parent): `vec` on the device at `off` floats past 16-byte alignment, between
    `guard` words of GUARD_BITS on each side (off in 0..3, guard a multiple of 4)."""
    torch = torch_dev()
    v = np.ascontiguousarray(vec, np.float32).reshape(-1)
    parent = _guarded_parent(guard + off + v.size + guard)
    view = parent[guard + off: guard + off + v.size]
    view.copy_(torch.from_numpy(v))
    assert view.data_ptr() % 16 == 4 * off
    return view, parent


def _guard_words(parent) -> np.ndarray:
    torch = torch_dev()
    torch.cuda.synchronize()
    return parent.view(torch.int32).cpu().numpy().view(np.uint32)


def assert_guards(parent, off: int, n: int, guard: int = 8):
    """Every guard word before and after placed()'s view still holds GUARD_BITS."""
    w = _guard_words(parent)
    lo, hi = guard + off, guard + off + n
    assert w.size == hi + guard
    bad = np.flatnonzero(np.concatenate([w[:lo], w[hi:]]) != GUARD_BITS)
    assert bad.size == 0, f"guard words overwritten (index in front+back guards: {bad[:8].tolist()})"


def placed_2d(mat, ld: int, off: int, guard: int = 8):
    """(view, parent): the rows x n matrix `mat` as a row-major view of leading dimension
    `ld` >= n starting `off` floats past 16-byte alignment; the padding columns [n, ld) and
    `guard` words on each side hold GUARD_BITS."""
    torch = torch_dev()
    a = np.ascontiguousarray(mat, np.float32)
    rows, n = a.shape
    assert ld >= n
    parent = _guarded_parent(guard + off + rows * ld + guard)
    full = parent[guard + off: guard + off + rows * ld].view(rows, ld)
    view = full[:, :n]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * off and view.stride(0) == ld
    return view, parent


def assert_guards_2d(parent, off: int, rows: int, n: int, ld: int, guard: int = 8):
    """The guards and the padding columns [n, ld) of placed_2d()'s parent are bit-unchanged."""
    w = _guard_words(parent)
    lo, hi = guard + off, guard + off + rows * ld
    assert w.size == hi + guard
    assert (w[:lo] == GUARD_BITS).all() and (w[hi:] == GUARD_BITS).all(), "guard words overwritten"
    pad = w[lo:hi].reshape(rows, ld)[:, n:]
    bad = np.argwhere(pad != GUARD_BITS)
    assert bad.size == 0, f"padding columns written, first (row, pad column): {bad[:4].tolist()}"


def uniform_csr(n_rows: int, n_cols: int, per_row: int, seed: int, table=None):
    """`per_row` distinct sorted columns per row, values from a 255-entry table."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.integers(0, n_cols, (n_rows, per_row), dtype=np.int64), axis=1)
    # make columns distinct within a row: bump duplicates forward, then re-sort
    for _ in range(8):
        dup = np.zeros_like(cols, bool)
        dup[:, 1:] = cols[:, 1:] == cols[:, :-1]
        if not dup.any():
            break
        cols[dup] = rng.integers(0, n_cols, int(dup.sum()))
        cols.sort(axis=1)
    if table is None:
        table = rng.uniform(-1, 1, 255).astype(np.float32)
    val = table[rng.integers(0, len(table), n_rows * per_row)].astype(np.float32)
    rp = np.arange(0, n_rows * per_row + 1, per_row, dtype=np.int32)
    return rp, cols.reshape(-1).astype(np.int32), val


MESSY_ROWS, MESSY_COLS = 4099, 40000
MESSY_VARIANTS = ("reversed", "shuffled", "repeated", "shuffled_repeated")
MESSY_LONG = {1234: 300, 3003: 2100}   # past SM_SERIAL_ROW_MAX; past the sell cap and the 2048-term tile


def messy_csr(variant: str, seed: int, codebook: bool = True, long_rows: bool = True):
    """(row_ptr, col_idx, val) of a 4099 x 40000 CSR whose rows are not strictly ascending.

    Base pattern: 8 terms per row from uniform_csr, every 50th row empty, row 1234 of 300 and row
    3003 of 2100 distinct columns (long_rows=False leaves them at 8: the fixed band kinds take no
    row with 31 / 63 terms in one band).  4099 rows are two row blocks of 4096 with a partial
    second one; 40000 columns are three 16384-column bands and five of 8192.  Values from a
    200-entry table (codebook=False: more than 255 distinct values).  Variants:
      reversed           every row descending;
      shuffled           a seeded permutation of every row;
      repeated           ascending, every 5th row (1, 6, 11, ...) with one column stored twice and
                         another three times, the repeats adjacent;
      shuffled_repeated  the previous, every row permuted.
    The repeats get values of their own, so B[r, c] is their sum."""
    assert variant in MESSY_VARIANTS, variant
    rng = np.random.default_rng(seed)
    table = rng.uniform(-1, 1, 200).astype(np.float32)
    rp, ci, _ = uniform_csr(MESSY_ROWS, MESSY_COLS, 8, seed=seed + 1, table=table)
    rows = [ci[rp[r]:rp[r + 1]].astype(np.int64) for r in range(MESSY_ROWS)]
    for r in range(0, MESSY_ROWS, 50):
        rows[r] = rows[r][:0]
    if long_rows:
        for r, k in MESSY_LONG.items():
            assert r % 50 != 0 and r % 5 != 1
            rows[r] = np.sort(rng.choice(MESSY_COLS, k, replace=False))
    for r in range(MESSY_ROWS):
        c = rows[r]
        if "repeated" in variant and r % 5 == 1 and c.size >= 8:
            c = np.concatenate([c[:2], c[1:2], c[2:6], c[5:6], c[5:]])   # c[1] twice, c[5] three times
        if variant == "reversed":
            c = c[::-1]
        elif variant.startswith("shuffled"):
            c = rng.permutation(c)
        rows[r] = c
    lens = np.array([c.size for c in rows], np.int64)
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci2 = np.concatenate(rows).astype(np.int32)
    if codebook:
        va2 = table[rng.integers(0, table.size, ci2.size)]
    else:
        va2 = rng.uniform(-1, 1, ci2.size).astype(np.float32)
    return rp2, ci2, np.ascontiguousarray(va2, np.float32)


def skewed_csr(n_rows: int, n_cols: int, lengths: np.ndarray, seed: int):
    """CSR with the given row lengths: every row's columns drawn with replacement and sorted
    ascending, so a row may hold a chance repeat but never a descending step."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    rp = np.zeros(n_rows + 1, np.int64)
    rp[1:] = np.cumsum(lengths)
    nnz = int(rp[-1])
    col = np.empty(nnz, np.int32)
    for r in range(n_rows):
        col[rp[r]:rp[r + 1]] = np.sort(rng.integers(0, n_cols, int(lengths[r])))
    val = rng.uniform(-1, 1, nnz).astype(np.float32)
    return rp.astype(np.int32), col, val


def with_env(key: str, value: str, fn):
    """Run fn() with os.environ[key] = value (restored afterwards)."""
    import os
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


def slab_order_spmv(rp, ci, va, x, y0, alpha, beta, slab_cols: int, slab0_cols: int | None = None,
                    beta_last: bool = False, term_slab=None, n_slabs: int | None = None):
    """The multi-slab band layouts' sum, restated on the oracle: each column slab summed in
    the reference's order (oracle.csr_spmv) -- slab 0 from beta*y, later slabs from -0.0 --
    then the slab sums added in slab order in fp32.  beta_last (sm_info.xband_beta_last, the
    band2 / cband hand-off): every slab from -0.0, y = (((beta*y + P_0) + P_1) + ...), beta*y
    as kernel.cc:10-29 forms it (y *= beta unless beta == 1).  Slab 0 covers [0, slab0_cols),
    slab s >= 1 [slab0_cols + (s-1) slab_cols, slab0_cols + s slab_cols)
    (sm_info.xband_slab0_cols / xband_slab_cols; even slabs when slab0_cols is None), unless
    term_slab gives every term's slab.  Bit-exact target for has_xband 2/3/4/5/6 with several slabs."""
    import oracle
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci)
    va = np.asarray(va, np.float32)
    y0 = np.asarray(y0, np.float32)
    n = rp.size - 1
    n_cols = x.size
    if term_slab is None:
        s0 = slab_cols if slab0_cols is None else slab0_cols
        n_slabs = 1 + max(0, -(-(n_cols - s0) // slab_cols))
        term_slab = np.where(ci < s0, 0, 1 + (ci.astype(np.int64) - s0) // slab_cols)
    bl = beta_last and n_slabs > 1
    out = (y0 * np.float32(beta) if beta != 1.0 else y0.copy()) if bl else None
    for s in range(n_slabs):
        mask = term_slab == s
        cm = np.concatenate([[0], np.cumsum(mask)])
        rps = np.zeros(n + 1, np.int64)
        rps[1:] = cm[rp[1:]] - cm[rp[:-1]]
        rps = np.cumsum(rps)
        if s == 0 and not bl:
            p = oracle.csr_spmv(rps, ci[mask], va[mask], x, y0, alpha, beta)
        else:
            p = oracle.csr_spmv(rps, ci[mask], va[mask], x, np.full(n, -0.0, np.float32), alpha, 1.0)
        out = p if out is None else (out + p).astype(np.float32)
    return out


def slab_order_for(info, rp, ci, va, x, y0, alpha, beta):
    """slab_order_spmv with the slab geometry and hand-off form the matrix reports."""
    return slab_order_spmv(rp, ci, va, x, y0, alpha, beta, info["xband_slab_cols"], info["xband_slab0_cols"],
                           beta_last=bool(info["xband_beta_last"]))
