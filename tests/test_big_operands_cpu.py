"""tests/big_operands.py checked on the CPU: the leading-dimension formulas, the term generator
(torch against numpy), the sampling conditions of the 2^30-term test, and the index arithmetic
of the spread operands' guard windows, and what a kernel whose 32-bit offset wraps would compute
on the operands of the GPU tests (it differs from the right product).  Nothing big is allocated."""
import numpy as np
import pytest

import big_operands as bo


@pytest.mark.parametrize("rows", [3, 5, 64, 70, 300])
def test_leading_dimensions_sit_on_each_side_of_the_limit(rows):
    lo, hi = bo.ld_below(rows), bo.ld_at(rows)
    assert lo % 4 == 0 and hi == lo + 4
    assert rows * lo * 4 < bo.LIMIT <= rows * hi * 4


@pytest.mark.parametrize("rows", [5, 13, 64, 70, 256, 300])
def test_ld_past_puts_the_last_row_past_4gib(rows):
    ld = bo.ld_past(rows)
    assert ld % 4 == 0 and (rows - 1) * ld * 4 >= 1 << 32 > (rows - 1) * (ld - 4) * 4
    assert ld >= bo.ld_at(rows) and rows * ld * 4 < 6 << 30


def test_leading_dimension_examples():
    assert (bo.ld_below(64), bo.ld_at(64)) == ((1 << 24) - 4, 1 << 24)
    assert (bo.ld_below(70), bo.ld_at(70)) == (15339168, 15339172)


@pytest.mark.parametrize("e0,e1", [(0, 4096), (bo.WRAP - 4096, bo.WRAP + 4096),
                                   (bo.BIG_NNZ - 4096, bo.BIG_NNZ)])
def test_generator_torch_equals_numpy(e0, e1):
    import torch
    table = bo.big_table()
    col = torch.empty(e1 - e0, dtype=torch.int32)
    val = torch.empty(e1 - e0, dtype=torch.float32)
    bo.terms_torch(e0, e1, torch.from_numpy(table), col, val, torch.device("cpu"))
    c, v = bo.terms_numpy(e0, e1, table)
    assert np.array_equal(col.numpy(), c) and np.array_equal(val.numpy().view(np.uint32), v.view(np.uint32))
    assert c.min() >= 0 and c.max() < bo.BIG_COLS
    # the closed form itself, one term at a time in Python integers
    for e in (e0, e0 + 1, (e0 + e1) // 2, e1 - 1):
        assert c[e - e0] == ((e * bo.COL_MUL) & 0xFFFFFFFF) >> 20
        assert v[e - e0] == table[((e * bo.VAL_MUL) & 0xFFFFFFFF) >> 24]


def test_sampling_conditions():
    table = bo.big_table()
    assert np.unique(table.view(np.uint32)).size == 256   # equal entries would hide a wrapped value
    rows = bo.big_sample_rows()
    above = bo.big_sampling_conditions(rows, table)
    r_star = bo.WRAP // bo.BIG_ROW_TERMS
    assert above.size == 3 + 256 + 8 and above.min() == r_star + 1
    assert set(range(r_star - 4, r_star + 4)) <= set(rows.tolist())
    assert set(range(8)) <= set(rows.tolist()) and set(range(bo.BIG_ROWS - 8, bo.BIG_ROWS)) <= set(rows.tolist())
    # the fixed steps between term t and term t - 2^30
    assert ((bo.WRAP * bo.COL_MUL) & 0xFFFFFFFF) >> 20 == 1024
    assert ((bo.WRAP * bo.VAL_MUL) & 0xFFFFFFFF) >> 24 == 192
    rp, ci, va = bo.big_sub_csr(rows[:3], table)
    assert rp.tolist() == [0, 1280, 2560, 3840] and ci.size == va.size == 3840
    # rows hold unsorted columns (the multiplier spreads them: no repeat inside these rows)
    assert (np.diff(ci[:1280]) < 0).any() and ci.min() >= 0 and ci.max() < bo.BIG_COLS


# (rows, n, ld, off) of every spread operand test_gpu_4gib.py makes, from the tables it uses
def _spread_shapes():
    X, Y, N = bo.COLS_A, bo.ROWS_A, (4, 5, 32, 64, 128)
    shapes = {(X, n, ld, 0) for n in N for ld in bo.LD_X.values()}              # spmm X
    shapes |= {(Y, n, ld, 0) for n in N for ld in bo.LD_Y.values()}             # spmm Y
    shapes |= {(X, 32, bo.LD_X["at"], 1)}                                       # X one float off alignment
    for ldg, ldx in bo.SDDMM_PLACES.values():                                   # sddmm, sddmm_table
        shapes |= {(Y, n, ldg, 0) for n in (4, 5, 32) if ldg}
        shapes |= {(X, n, ldx, 0) for n in (4, 5, 32) if ldx}
    lda, ldc = (1 << 29) + 3, (1 << 29) + 1
    shapes |= {(m, 300, lda, 0) for m in (2, 3)} | {(m, 257, ldc, 0) for m in (2, 3)}   # AddMatMat A, C
    shapes |= {(3, 5, (1 << 29) + 1, 0), (5, 3, (1 << 28) + 3, 0)}              # beta, transpose
    shapes |= {(r, n, bo.ld_past(r), 0) for r, n in ((13, 300), (13, 256), (300, 13), (256, 13))}   # panel kernels
    return sorted(shapes)


SPREAD_SHAPES = _spread_shapes()


@pytest.mark.parametrize("rows,n,ld,off", SPREAD_SHAPES)
def test_spread_windows_do_not_touch_live_data(rows, n, ld, off):
    live, before, after, size = bo.spread_windows(rows, n, ld, off)
    assert live[0] == bo.GUARD + off and (np.diff(live) == ld).all()
    # ascending, disjoint intervals: before_r, live_r, after_r, before_{r+1}, ...
    starts = np.stack([before, live, after], 1).reshape(-1)
    ends = np.stack([before + bo.GUARD, live + n, after + bo.GUARD], 1).reshape(-1)
    assert (starts[1:] >= ends[:-1]).all() and starts[0] >= 0 and ends[-1] <= size
    assert (before + bo.GUARD == live).all() and (live + n == after).all()   # no gap next to the live part
    assert size == rows * ld + bo.GUARD + off


def test_spread_windows_refuse_overlapping_guards():
    with pytest.raises(AssertionError):
        bo.spread_windows(4, 32, 32 + 2 * bo.GUARD - 1)


def test_a_wrapped_term_offset_changes_every_sampled_row_above():
    """What a kernel with a wrapping 32-bit byte offset would compute on the rows above term
    2^30 -- the same rows fed the terms 2^30 earlier -- differs from the right product in every
    such row: the sampled rows cannot pass by chance."""
    import oracle
    oracle.build()
    table = bo.big_table()
    above = bo.big_sampling_conditions(bo.big_sample_rows(), table)
    rp, ci, va = bo.big_sub_csr(above, table)
    shifted = [bo.terms_numpy(int(r) * bo.BIG_ROW_TERMS - bo.WRAP, (int(r) + 1) * bo.BIG_ROW_TERMS - bo.WRAP, table)
               for r in above]
    ci_w = np.concatenate([c for c, _ in shifted])
    va_w = np.concatenate([v for _, v in shifted])
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, bo.BIG_COLS).astype(np.float32)
    y0 = rng.uniform(-1, 1, above.size).astype(np.float32)
    right = oracle.csr_spmv(rp, ci, va, x, y0, 1.3, 0.7)
    wrapped = oracle.csr_spmv(rp, ci_w, va_w, x, y0, 1.3, 0.7)
    assert (right.view(np.uint32) != wrapped.view(np.uint32)).all()


@pytest.mark.parametrize("n_rhs", [4, 32, 64])
def test_a_wrapped_x_offset_changes_the_spmm(n_rhs):
    """The "past" placement of the row-panel SpMM test: X's row 63 starts at 2^32 bytes or more,
    a 32-bit byte offset of it wraps to float 188 of X's storage, the decoy written there lies
    clear of every live part and guard, row 63 and the decoy are non-zero and differ in every
    column, and the product a wrapping kernel would form -- row 63 read as the decoy -- differs
    from the right one in every matrix row that holds column 63."""
    import oracle
    oracle.build()
    ld = bo.LD_X["past"]
    assert (bo.COLS_A - 1) * ld * 4 >= 1 << 32
    t = bo.wrap_target(bo.COLS_A, ld)
    assert t == (bo.COLS_A - 1) * ld - (1 << 30) == 188 and bo.decoy_is_clear(bo.COLS_A, n_rhs, ld)
    live, before, after, _ = bo.spread_windows(bo.COLS_A, n_rhs, ld)
    lo, hi = bo.GUARD + t, bo.GUARD + t + n_rhs                  # the decoy inside the parent
    assert after[0] + bo.GUARD <= lo and hi <= before[1]
    X, Y0, decoy = bo.spmm_panel(n_rhs)
    last = X[bo.COLS_A - 1]
    assert (last != 0).all() and (decoy != 0).all() and (last != decoy).all()
    assert not bo.decoy_is_clear(bo.COLS_A, 128, ld)             # N = 128: no decoy, and no pipelined kernel
    rp, ci, va, _, _ = bo.small_csr()
    holds = np.array([(ci[rp[r]:rp[r + 1]] == bo.COLS_A - 1).any() for r in range(bo.ROWS_A)])
    assert holds.sum() > 40
    Xw = X.copy()
    Xw[bo.COLS_A - 1] = decoy
    for alpha, beta in ((1.3, 0.7), (-2.0, 0.0)):
        right = oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)
        wrapped = oracle.csr_spmm(rp.astype(np.int64), ci, va, Xw, Y0, alpha, beta)
        differs = (right.view(np.uint32) != wrapped.view(np.uint32)).any(axis=1)
        assert (differs == holds).all()
