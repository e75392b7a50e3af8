"""Operands at the edges of the float range: the regimes, the comparisons and the bound of
tests/test_range_edges_cpu.py and tests/test_gpu_range_edges.py (numpy only).

Every regime replaces the values, x and y0 of an unchanged pattern with sign * m * 2**e
(m uniform in [1, 2), e an integer uniform in the regime's range), so that the documented
rounding sequence -- fl(v * alpha) first, then fl(x * that), added one at a time
(include/sparsematrix.h, "Semantics kept from the reference") -- runs where it differs most
from any other sequence: subnormal terms and sums, a fold that underflows or overflows, sums
that overflow midway, and alpha = inf.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SEED = 2026
TINY = np.float32(2.0 ** -126)       # the smallest normal float32
ULP_MIN = 2.0 ** -149                # the smallest subnormal float32
X86_NAN_BITS = 0xFFC00000            # what inf - inf and 0 * inf give on the oracle's host


def pow2(rng, n, lo, hi, signed=True):
    """n float32 values sign * m * 2**e: m uniform in [1, 2), e an integer uniform in [lo, hi],
    the sign uniform +-1 (or +1).  Drawn in the order sign, m, e."""
    s = np.where(rng.random(n) < 0.5, -1.0, 1.0) if signed else 1.0
    m = rng.uniform(1.0, 2.0, n)
    e = rng.integers(lo, hi + 1, n)
    return (s * np.ldexp(m, e)).astype(np.float32)


@dataclass(frozen=True)
class Regime:
    values: tuple            # (lo, hi, signed)
    x: tuple
    y0: tuple
    scalars: tuple           # ((alpha, beta), ...)

    def table(self, rng, n):
        return pow2(rng, n, *self.values)

    def draw_x(self, rng, shape):
        return pow2(rng, int(np.prod(shape)), *self.x).reshape(shape)

    def draw_y0(self, rng, shape):
        return pow2(rng, int(np.prod(shape)), *self.y0).reshape(shape)


A_UNDER = 1.3 * 2.0 ** -40
A_OVER = 1.3 * 2.0 ** 28

REGIMES = {
    "subnormal": Regime((-75, -62, True), (-75, -62, True), (-140, -127, True),
                        ((1.3, 0.7), (1.0, 1.0), (0.5, 0.0))),
    "fold_under": Regime((-110, -100, True), (100, 120, True), (-30, -10, True),
                         ((A_UNDER, 0.7), (A_UNDER, 1.0))),
    "fold_over": Regime((84, 99, True), (-120, -100, True), (-30, -20, True), ((A_OVER, 0.7),)),
    "midsum_over": Regime((60, 64, True), (60, 62, True), (120, 126, True), ((1.3, 0.7), (1.0, 1.0))),
    "alpha_inf": Regime((-3, 3, False), (-3, 3, False), (-3, 3, True), ((float("inf"), 1.0),)),
}
BOUND_REGIMES = ("subnormal", "fold_under")      # where assert_sum_close applies


def values_like(rng, regime, va_old):
    """New values on the pattern of va_old.  A codebook matrix (at most 255 distinct bit
    patterns) keeps its ids and takes a 200-entry table (255 where it used more than 200);
    any other matrix takes one draw per term."""
    old = np.ascontiguousarray(va_old, np.float32).view(np.uint32)
    uniq, ids = np.unique(old, return_inverse=True)
    if uniq.size <= 255:
        return regime.table(rng, 200 if uniq.size <= 200 else 255)[ids]
    va = regime.table(rng, old.size)
    assert np.unique(va.view(np.uint32)).size >= 256
    return va


def draw(name, va_old, n_cols, n_rows):
    """(va, x, y0) of regime `name` for a pattern whose values were va_old.  One generator per
    regime, drawn in the order y0, values, x: with a 200-entry table the share of rows that
    overflow depends on the few largest entries, and tests/test_range_edges_cpu.py holds this
    stream to what each regime is named for."""
    reg = REGIMES[name]
    rng = np.random.default_rng(SEED)
    y0 = reg.draw_y0(rng, n_rows)
    va = values_like(rng, reg, va_old)
    return va, reg.draw_x(rng, n_cols), y0


# ---------------------------------------------------------------------------- comparisons
def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def assert_same_nanclass(got, want, mask=None, what=""):
    """NaN exactly where `want` is NaN (any sign and payload: they are the hardware's); every
    other output bit-identical, signed zeros and infinities included."""
    g, w = _bits(got), _bits(want)
    assert g.size == w.size, (what, g.size, w.size)
    if mask is not None:
        m = np.asarray(mask).reshape(-1)
        g, w = g[m], w[m]
    gn, wn = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    bad = np.flatnonzero((gn != wn) | (~wn & (g != w)))
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} outputs differ, first at {bad[:5].tolist()}: "
                           f"got {[hex(v) for v in g[bad[:5]]]} want {[hex(v) for v in w[bad[:5]]]}")


def rounded_terms(rp, ci, va, x, y0, alpha, beta):
    """(sum64, absum64, n_r): the terms t_e = fl(x * fl(v * alpha)) and fl(beta * y) (y itself
    when beta == 1) formed in float32 as documented, then summed per row in float64, with the
    sum of their magnitudes and the number of terms of each row."""
    rp = np.asarray(rp, np.int64)
    n = rp.size - 1
    n_r = np.diff(rp)
    rows = np.repeat(np.arange(n), n_r)
    with np.errstate(all="ignore"):
        t = np.asarray(x, np.float32)[np.asarray(ci, np.int64)] * (np.asarray(va, np.float32) * np.float32(alpha))
        y0 = np.asarray(y0, np.float32)
        by = y0 if beta == 1.0 else y0 * np.float32(beta)
        assert t.dtype == np.float32 and by.dtype == np.float32
        t64 = t.astype(np.float64)
        sum64 = by.astype(np.float64) + np.bincount(rows, t64, n)
        absum64 = np.abs(by.astype(np.float64)) + np.bincount(rows, np.abs(t64), n)
    return sum64, absum64, n_r


def sum_bound(absum64, n_r):
    return 1e-6 * np.asarray(absum64, np.float64) + (np.asarray(n_r, np.float64) + 1) * ULP_MIN


def assert_sum_close(got, sum64, absum64, n_r, what=""):
    """|got - sum64| <= 1e-6 * absum64 + (n_r + 1) * 2**-149 on the outputs whose absum64 is
    finite.  The second term is one rounding of at most 2**-150 per product where a kernel
    fuses the multiply-add, plus one for beta*y (additions below 2**-125 are exact); there is
    no other absolute slack."""
    got = np.asarray(got, np.float64)
    sum64 = np.broadcast_to(np.asarray(sum64, np.float64), got.shape)
    bound = np.broadcast_to(sum_bound(absum64, n_r), got.shape)
    ok = np.isfinite(np.broadcast_to(np.asarray(absum64, np.float64), got.shape))
    assert ok.any(), what
    with np.errstate(invalid="ignore"):
        err = np.abs(got - sum64)[ok]
    assert not np.isnan(err).any(), f"{what}: NaN among outputs with finite terms"
    ratio = err / bound[ok]
    bad = ratio > 1.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {ratio.size} outputs out of bound, worst ratio "
                           f"{float(ratio.max()):.3g}, first at {np.flatnonzero(ok.reshape(-1))[bad][:5].tolist()}")
    return float(ratio.max())


# ---------------------------------------------------------------------------- restatement
def flush(a):
    """Subnormals to zero (sign kept)."""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < TINY, np.copysign(np.float32(0), a), a).astype(np.float32)


def restate_spmv(rp, ci, va, x, y0, alpha, beta, ftz=False, alpha_last=False):
    """The reference's order in numpy float32, one operation and one rounding at a time:
    acc = y (times beta unless beta == 1), then acc = acc + x * (v * alpha) over the row's terms
    in stored order.  Variants that must NOT match: ftz flushes every subnormal product and sum
    to zero; alpha_last forms (x * v) * alpha."""
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    a = np.float32(alpha)
    f = flush if ftz else (lambda v: v)
    with np.errstate(all="ignore"):
        xv = np.asarray(x, np.float32)[np.asarray(ci, np.int64)]
        va = np.asarray(va, np.float32)
        t = f(f(xv * va) * a) if alpha_last else f(xv * f(va * a))
        y0 = np.asarray(y0, np.float32)
        acc = y0.copy() if beta == 1.0 else f(y0 * np.float32(beta))
        if alpha != 0.0:
            order = np.argsort(-lens, kind="stable")          # rows by length: row k terms deep
            n_active = order.size
            for k in range(int(lens.max()) if lens.size else 0):
                while n_active and lens[order[n_active - 1]] <= k:
                    n_active -= 1
                r = order[:n_active]
                acc[r] = f(acc[r] + t[rp[r] + k])
    assert acc.dtype == np.float32 and t.dtype == np.float32
    return acc


def fold(va, alpha):
    """fl(v * alpha) and whether it is exact."""
    with np.errstate(all="ignore"):
        va = np.asarray(va, np.float32)
        fv = va * np.float32(alpha)
        exact = fv.astype(np.float64) == va.astype(np.float64) * float(np.float32(alpha))
    return fv, exact


def is_subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < TINY)


def nan_patterns(a):
    """The distinct bit patterns of the NaNs in `a`, as hex strings."""
    b = _bits(a)
    return sorted(hex(v) for v in np.unique(b[np.isnan(b.view(np.float32))]))
