"""Helpers for the tests of operands and term arrays of 4 GiB and more (test_gpu_4gib.py, checked
on the CPU by test_big_operands_cpu.py).

Leading dimensions.  The kernels that form 32-bit byte offsets run while an operand of `rows`
rows spans fewer than LIMIT = 0xFFFFFFF0 bytes (rows * ld * 4 < LIMIT): ld_below(rows) is the
largest multiple of 4 on that side of the switch, ld_at(rows) the smallest past it.  At ld_at
the last row still starts below 2^32 bytes; ld_past(rows) is the smallest multiple of 4 that puts
the last row's start at 2^32 bytes or more, where a 32-bit byte offset wraps.

spread_2d.  A rows x n matrix as a view of leading dimension ld into one parent of
rows * ld + 64 floats that is never initialised as a whole: only the live columns and GUARD
words of gpu_util.GUARD_BITS before and after every row's live part are written, and
assert_spread_guards downloads only those windows.  A correct kernel reads nothing else.
write_decoy puts a known row where a wrapped 32-bit offset of the last row's start would read
(wrap_target), so that a kernel that wraps gives wrong bits whatever the allocation held.

The term generator of the 2^30-term matrix, a closed form of the term index e (int64), so the
device (torch) and the host (numpy) agree without a download:
    col[e] = ((e * COL_MUL) & 0xFFFFFFFF) >> 20          n_cols = 4096
    val[e] = table[((e * VAL_MUL) & 0xFFFFFFFF) >> 24]    table: 256 seeded floats in [-1, 1)
with 1280 terms in each of 2^20 rows: nnz = 1.25 * 2^30.  Both multipliers are odd, so terms e
and e - 2^30 differ by a fixed non-zero step: columns by (2^30 * COL_MUL mod 2^32) >> 20 = 1024
(mod 4096), table ids by (2^30 * VAL_MUL mod 2^32) >> 24 = 192 (mod 256).  A kernel whose
32-bit byte offset 4 * e wraps reads term e - 2^30 and cannot give term e's product by chance.
"""
from __future__ import annotations

import numpy as np

from gpu_util import GUARD_BITS

LIMIT = 0xFFFFFFF0     # the bound of the kernels with 32-bit byte offsets (bytes, exclusive)
GUARD = 64             # guard words on each side of a row's live part


# ---------------------------------------------------------------------------- leading dimensions
def ld_below(rows: int) -> int:
    """The largest multiple of 4 with rows * ld * 4 < LIMIT."""
    return (LIMIT - 1) // (4 * rows) // 4 * 4


def ld_at(rows: int) -> int:
    """The smallest multiple of 4 with rows * ld * 4 >= LIMIT."""
    return ld_below(rows) + 4


def ld_past(rows: int) -> int:
    """The smallest multiple of 4 with (rows - 1) * ld * 4 >= 2^32: the last row starts at or
    past 4 GiB."""
    assert rows >= 2
    return (-(-(1 << 30) // (rows - 1)) + 3) // 4 * 4


# ---------------------------------------------------------------------------- spread operands
def spread_windows(rows: int, n: int, ld: int, off: int = 0):
    """(live, before, after): the start index in the parent of every row's live part and of
    its two guard windows (int64 arrays of `rows` entries), and the parent's size.  Pure index
    arithmetic: row r's live part is [base + r ld, base + r ld + n) with base = GUARD + off."""
    assert 0 <= off < 4 and n >= 1 and rows >= 1
    assert ld >= n + 2 * GUARD, "the guard windows of neighbouring rows would overlap"
    base = GUARD + off
    live = base + np.arange(rows, dtype=np.int64) * ld
    return live, live - GUARD, live + n, rows * ld + GUARD + off


def spread_2d(mat, ld: int, off: int = 0):
    """(view, parent): `mat` (rows x n, float32) on the device as a view with stride(0) == ld
    into one torch.empty(rows * ld + 64 (+ off)) parent; the base is 256-byte aligned (`off`
    floats past it).  Only the live columns and the guard windows are written."""
    import torch
    a = np.ascontiguousarray(mat, np.float32)
    rows, n = a.shape
    live, before, after, size = spread_windows(rows, n, ld, off)
    parent = torch.empty(size, dtype=torch.float32, device="cuda")
    assert parent.data_ptr() % 256 == 0, "allocation base not 256-byte aligned"
    view = torch.as_strided(parent, (rows, n), (ld, 1), int(live[0]))
    view.copy_(torch.from_numpy(a).to("cuda"))
    words = parent.view(torch.int32)
    for start in (before, after):
        torch.as_strided(words, (rows, GUARD), (ld, 1), int(start[0])).fill_(GUARD_BITS)
    assert view.stride(0) == ld and view.data_ptr() == parent.data_ptr() + 4 * int(live[0])
    assert view.data_ptr() % 256 == (4 * off) % 256
    return view, parent


def assert_spread_guards(parent, rows: int, n: int, ld: int, off: int = 0):
    """Every guard word of spread_2d's parent still holds GUARD_BITS (2 * rows windows of 64
    words are downloaded, nothing else)."""
    import torch
    _, before, after, size = spread_windows(rows, n, ld, off)
    assert parent.numel() == size
    torch.cuda.synchronize()
    words = parent.view(torch.int32)
    for name, start in (("before", before), ("after", after)):
        w = torch.as_strided(words, (rows, GUARD), (ld, 1), int(start[0])).cpu().numpy().view(np.uint32)
        bad = np.argwhere(w != GUARD_BITS)
        assert bad.size == 0, f"guard words {name} the live part written, first (row, word): {bad[:4].tolist()}"


def flat(view, rows: int, n: int, ld: int):
    """The (rows - 1) * ld + n floats behind a spread view as one 1-D tensor (the C ABI takes a
    pointer and a leading dimension)."""
    f = view.as_strided(((rows - 1) * ld + n,), (1,))
    assert f.data_ptr() == view.data_ptr()
    return f


def wrap_target(rows: int, ld: int) -> int:
    """Where the 32-bit byte offset of the last row's start lands: the float index, counted from
    the operand's first element, of ((rows - 1) * ld * 4) mod 2^32."""
    return ((rows - 1) * ld * 4 % (1 << 32)) // 4


def write_decoy(parent, rows: int, n: int, ld: int, row, off: int = 0):
    """Write `row` (n floats) where a wrapped 32-bit offset of the last row would read
    (wrap_target), inside spread_2d's parent: defined data in place of uninitialised memory.
    Returns the view of it.  The window must lie clear of every live part and guard window."""
    import torch
    t = wrap_target(rows, ld)
    assert decoy_is_clear(rows, n, ld), (rows, n, ld, t)
    view = parent[GUARD + off + t: GUARD + off + t + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(row, np.float32)).to("cuda"))
    return view


def decoy_is_clear(rows: int, n: int, ld: int) -> bool:
    """The last row starts at 2^32 bytes or more and the n floats at wrap_target lie inside
    row 0's stretch of the parent, past its live part and after-guard and before row 1's
    before-guard."""
    t = wrap_target(rows, ld)
    return (rows - 1) * ld * 4 >= 1 << 32 and n + GUARD <= t and t + n <= ld - GUARD


# ---------------------------------------------------------------------------- part A's operands
ROWS_A, COLS_A = 70, 64
LENS_A = (0, 1, 3, 4, 15, 16, 17, 33, 64)
LD_X = {"below": ld_below(COLS_A), "at": ld_at(COLS_A), "past": ld_past(COLS_A)}
LD_Y = {"below": ld_below(ROWS_A), "at": ld_at(ROWS_A), "past": ld_past(ROWS_A)}
SDDMM_PLACES = {               # (ldg, ldx); None: the compact operand, ld = n_rhs
    "g_at": (LD_Y["at"], None), "x_at": (None, LD_X["at"]),
    "g_past": (LD_Y["past"], None), "x_past": (None, LD_X["past"]),
    "both_below": (LD_Y["below"], LD_X["below"]),
}


def small_csr():
    """70 x 64 CSR (a partial 16-row MFMA tile): row lengths cycle through LENS_A, distinct
    ascending columns, columns 0 and 63 in every row of two terms or more, values from a seeded
    200-entry table; ids < 7 and a 7-entry table for the table matrix of the same pattern."""
    rng = np.random.default_rng(7064)
    table = rng.uniform(-1, 1, 200).astype(np.float32)
    rows = []
    for r in range(ROWS_A):
        k = LENS_A[r % len(LENS_A)]
        if k == 0:
            c = np.zeros(0, np.int64)
        elif k == 1:
            c = np.array([0 if (r // len(LENS_A)) % 2 == 0 else COLS_A - 1], np.int64)
        else:
            c = np.sort(np.concatenate([[0, COLS_A - 1], rng.choice(np.arange(1, COLS_A - 1), k - 2, replace=False)]))
        assert np.unique(c).size == k
        rows.append(c)
    lens = np.array([c.size for c in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    va = np.ascontiguousarray(table[rng.integers(0, table.size, ci.size)], np.float32)
    ids = rng.integers(0, 7, ci.size).astype(np.uint8)
    table7 = rng.uniform(-1, 1, 7).astype(np.float32)
    assert (ci == 0).sum() > 40 and (ci == COLS_A - 1).sum() > 40
    return rp, ci, va, ids, table7


def spmm_panel(n_rhs: int):
    """(X 64 x n_rhs, Y0 70 x n_rhs, decoy n_rhs): seeded operands with zero and -0.0 rows in X
    -- never row 0 or row 63, the row that starts past 2^32 bytes at ld_past -- and -0.0 rows in
    Y0; decoy is what write_decoy puts at the wrap target of row 63: non-zero and different
    from X[63] in every column."""
    rng = np.random.default_rng(640 + n_rhs)
    X = rng.uniform(-1, 1, (COLS_A, n_rhs)).astype(np.float32)
    X[1::3] = 0.0
    X[2::9] = -0.0
    Y0 = rng.uniform(-1, 1, (ROWS_A, n_rhs)).astype(np.float32)
    Y0[::4] = -0.0
    decoy = (np.where(X[COLS_A - 1] > 0, -1.0, 1.0) * rng.uniform(0.25, 1, n_rhs)).astype(np.float32)
    assert (X[COLS_A - 1] != 0).all() and (X[0] != 0).all() and (decoy != 0).all()
    assert (decoy != X[COLS_A - 1]).all()
    return X, Y0, decoy


# ---------------------------------------------------------------------------- the term generator
COL_MUL = 0x9E3779B1
VAL_MUL = 0x85EBCA6B
BIG_COLS = 4096
BIG_ROW_TERMS = 1280
BIG_ROWS = 1 << 20
BIG_NNZ = BIG_ROWS * BIG_ROW_TERMS      # 1.25 * 2^30
WRAP = 1 << 30                          # terms in 4 GiB of int32 / float32
GEN_CHUNK = 1 << 26                     # terms generated at a time on the device
assert BIG_NNZ == 5 * (1 << 28) and BIG_NNZ < (1 << 31) and (BIG_NNZ - 1) * COL_MUL < (1 << 63)


def big_table() -> np.ndarray:
    return np.random.default_rng(4096).uniform(-1, 1, 256).astype(np.float32)


def terms_numpy(e0: int, e1: int, table: np.ndarray):
    """(col int32, val float32) of the terms [e0, e1), on the host."""
    e = np.arange(e0, e1, dtype=np.int64)
    col = ((e * COL_MUL) & 0xFFFFFFFF) >> 20
    tid = ((e * VAL_MUL) & 0xFFFFFFFF) >> 24
    return col.astype(np.int32), np.ascontiguousarray(table[tid], np.float32)


def terms_torch(e0: int, e1: int, table, col_out, val_out, device):
    """The terms [e0, e1) written into col_out / val_out (int32 / float32 tensors of e1 - e0
    elements on `device`); `table` a float32 tensor there.  In-place steps on one int64
    temporary at a time: (e1 - e0) * 8 bytes, twice at the peak with the gathered values."""
    import torch
    t = torch.arange(e0, e1, dtype=torch.int64, device=device)
    t.mul_(COL_MUL).bitwise_and_(0xFFFFFFFF).bitwise_right_shift_(20)
    col_out.copy_(t)
    del t
    t = torch.arange(e0, e1, dtype=torch.int64, device=device)
    t.mul_(VAL_MUL).bitwise_and_(0xFFFFFFFF).bitwise_right_shift_(24)
    torch.index_select(table, 0, t, out=val_out)


def big_csr_device(table: np.ndarray):
    """(row_ptr, col, val) of the whole matrix as device tensors, generated in chunks of
    GEN_CHUNK terms."""
    import torch
    dev = torch.device("cuda")
    tab = torch.from_numpy(table).to(dev)
    col = torch.empty(BIG_NNZ, dtype=torch.int32, device=dev)
    val = torch.empty(BIG_NNZ, dtype=torch.float32, device=dev)
    for e0 in range(0, BIG_NNZ, GEN_CHUNK):
        e1 = min(BIG_NNZ, e0 + GEN_CHUNK)
        terms_torch(e0, e1, tab, col[e0:e1], val[e0:e1], dev)
    rp = torch.arange(0, BIG_NNZ + 1, BIG_ROW_TERMS, dtype=torch.int64, device=dev).to(torch.int32)
    return rp, col, val


def big_sample_rows() -> np.ndarray:
    """The sampled rows, ascending: the first 8, [r* - 4, r* + 4) around the row r* that
    straddles term 2^30, 256 seeded rows above r* + 4, and the last 8."""
    r_star = WRAP // BIG_ROW_TERMS
    assert r_star * BIG_ROW_TERMS < WRAP < (r_star + 1) * BIG_ROW_TERMS, "r* straddles term 2^30"
    rng = np.random.default_rng(1280)
    mid = r_star + 4 + rng.choice(BIG_ROWS - 8 - (r_star + 4), 256, replace=False)
    rows = np.concatenate([np.arange(8), np.arange(r_star - 4, r_star + 4), mid,
                           np.arange(BIG_ROWS - 8, BIG_ROWS)]).astype(np.int64)
    rows = np.unique(rows)
    assert rows.size == 8 + 8 + 256 + 8
    return rows


def big_sub_csr(rows: np.ndarray, table: np.ndarray):
    """(row_ptr int64, col, val) of the sub-matrix of `rows`, regenerated from the formula."""
    cols, vals = [], []
    for r in rows:
        c, v = terms_numpy(int(r) * BIG_ROW_TERMS, (int(r) + 1) * BIG_ROW_TERMS, table)
        cols.append(c)
        vals.append(v)
    rp = np.arange(0, (rows.size + 1) * BIG_ROW_TERMS, BIG_ROW_TERMS, dtype=np.int64)
    return rp, np.concatenate(cols), np.concatenate(vals)


def big_sampling_conditions(rows: np.ndarray, table: np.ndarray):
    """The two conditions that keep a wrapped term offset visible: at least 264 sampled rows lie
    wholly at or above term 2^30, and on those rows (col, val) at term t differs from (col, val)
    at t - 2^30 in every position.  Returns the rows above."""
    above = rows[rows * BIG_ROW_TERMS >= WRAP]
    assert above.size >= 264, above.size
    for r in above:
        e0 = int(r) * BIG_ROW_TERMS
        c1, v1 = terms_numpy(e0, e0 + BIG_ROW_TERMS, table)
        c0, v0 = terms_numpy(e0 - WRAP, e0 - WRAP + BIG_ROW_TERMS, table)
        same = (c1 == c0) & (v1.view(np.uint32) == v0.view(np.uint32))
        assert not same.any(), f"row {int(r)}: a term equals the term 2^30 before it"
        assert (c1 != c0).all() and (v1.view(np.uint32) != v0.view(np.uint32)).all(), int(r)
    return above
