"""The range-edge regimes (tests/range_edges.py) checked on the CPU oracle alone: the numpy
restatement of the reference's order equals the oracle, every regime still produces what it is
named for, a flushed or re-associated restatement differs where it should, and the bound of
assert_sum_close holds for the oracle itself.  No GPU."""
import functools

import numpy as np
import pytest

import oracle
import range_edges as re_
from layout_specs import _base, _long_csr
from range_edges import REGIMES

PATTERNS = {"base": _base, "long_csr": _long_csr}
CASES = [(p, r, ab) for p in PATTERNS for r in REGIMES for ab in REGIMES[r].scalars]
IDS = [f"{p}-{r}-{i}" for p in PATTERNS for r in REGIMES for i in range(len(REGIMES[r].scalars))]


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


@functools.lru_cache(maxsize=None)
def _data(pattern, regime):
    c = PATTERNS[pattern]()
    return c.with_data(*re_.draw(regime, c.va, c.n_cols, c.n_rows))


@functools.lru_cache(maxsize=None)
def _oracle_spmv(pattern, regime, alpha, beta):
    c = _data(pattern, regime)
    return oracle.csr_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta)


def _restate(c, alpha, beta, **kw):
    return re_.restate_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, **kw)


def _differs(a, b):
    """Outputs that would fail assert_same_nanclass."""
    an, bn = np.isnan(a), np.isnan(b)
    return (an != bn) | (~bn & (a.view(np.uint32) != b.view(np.uint32)))


def test_generator():
    rng = np.random.default_rng(1)
    v = re_.pow2(rng, 4096, -3, 3)
    a = np.abs(v.astype(np.float64))
    assert v.dtype == np.float32 and a.min() >= 2.0 ** -3 and a.max() < 2.0 ** 4
    assert 0.4 < (v < 0).mean() < 0.6
    assert (re_.pow2(rng, 4096, -3, 3, signed=False) > 0).all()
    assert set(np.floor(np.log2(a)).astype(int)) == set(range(-3, 4))
    c = _data("base", "subnormal")
    assert np.unique(c.va.view(np.uint32)).size <= 200           # the codebook layouts still apply
    assert np.unique(_data("long_csr", "subnormal").va.view(np.uint32)).size >= 256


@pytest.mark.parametrize("pattern,regime,ab", CASES, ids=IDS)
def test_restatement_equals_oracle(pattern, regime, ab):
    c = _data(pattern, regime)
    re_.assert_same_nanclass(_restate(c, *ab), _oracle_spmv(pattern, regime, *ab), None,
                             f"{pattern} {regime} {ab}")


@pytest.mark.parametrize("pattern,regime,ab", CASES, ids=IDS)
def test_inputs_exercise_their_regime(pattern, regime, ab):
    """Conditions on the reference alone."""
    c = _data(pattern, regime)
    alpha, beta = ab
    want = _oracle_spmv(pattern, regime, alpha, beta)
    ne = c.lens > 0
    if beta == 0.0:                       # the seeded NaNs of y_in are not the regime's
        ne = ne & ~np.isnan(c.y_in(beta))
    w = want[ne]
    n = w.size
    fv, exact = re_.fold(c.va, alpha)
    with np.errstate(all="ignore"):
        terms = c.x[c.ci] * fv
    frac = dict(inf=np.isinf(w).sum() / n, nan=np.isnan(w).sum() / n, finite=np.isfinite(w).sum() / n)
    print(f"{pattern} {regime} {ab}: rows {n} finite {np.isfinite(w).sum()} inf {np.isinf(w).sum()} "
          f"nan {np.isnan(w).sum()} subnormal rows {re_.is_subnormal(w).sum()} "
          f"subnormal terms {re_.is_subnormal(terms).mean():.3f} fold overflow {np.isinf(fv).mean():.3f}")
    if regime == "subnormal":
        assert re_.is_subnormal(terms).mean() >= 0.90
        assert re_.is_subnormal(w).mean() >= 0.60
        assert np.isfinite(w).all() and (w != 0).all()
    elif regime == "fold_under":
        assert re_.is_subnormal(fv).all() and not exact.any()
    elif regime == "fold_over":
        assert frac["inf"] >= 0.10 and frac["nan"] >= 0.005 and frac["finite"] >= 0.70
        assert np.isinf(fv).any()
    elif regime == "midsum_over":
        assert frac["inf"] >= 0.10 and frac["finite"] >= 0.60
        assert np.isfinite(fv).all()
        if ab == (1.3, 0.7):
            assert np.isnan(w).sum() >= 50
    elif regime == "alpha_inf":
        assert (w.view(np.uint32) == 0x7F800000).all()
        empty = c.lens == 0
        assert empty.any() and np.array_equal(want[empty].view(np.uint32), c.y0[empty].view(np.uint32))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_flush_to_zero_is_noticed(pattern):
    """The restatement with every subnormal product and sum flushed differs from the oracle in
    every non-empty row of `subnormal`."""
    c = _data(pattern, "subnormal")
    for alpha, beta in REGIMES["subnormal"].scalars:
        d = _differs(_restate(c, alpha, beta, ftz=True), _oracle_spmv(pattern, "subnormal", alpha, beta))
        ne = (c.lens > 0) & ~np.isnan(c.y_in(beta))
        assert d[ne].all(), (alpha, beta, int(d[ne].sum()), int(ne.sum()))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_alpha_folded_late_is_noticed(pattern):
    """(x * v) * alpha instead of x * (v * alpha): >= 90 % of the rows of `fold_under` differ,
    and in `fold_over` every row that holds an overflowed fl(v * alpha) (the oracle ends it inf
    or NaN, the late fold finite).  The other rows of `fold_over` hold normal numbers only, where
    the two forms differ by a last-bit rounding that the row's largest term often absorbs: about
    half of all rows differ there (measured 49 % and 53 %), so "every row" cannot be asked."""
    for regime in ("fold_under", "fold_over"):
        c = _data(pattern, regime)
        for alpha, beta in REGIMES[regime].scalars:
            d = _differs(_restate(c, alpha, beta, alpha_last=True), _oracle_spmv(pattern, regime, alpha, beta))
            ne = c.lens > 0
            print(f"{pattern} {regime} ({alpha}, {beta}): {int(d[ne].sum())} of {int(ne.sum())} rows differ")
            if regime == "fold_under":
                assert d[ne].mean() >= 0.90, (alpha, beta, float(d[ne].mean()))
            else:
                over = np.isinf(re_.fold(c.va, alpha)[0])
                hit = np.add.reduceat(np.append(over, False), c.rp[:-1].astype(np.int64))[: c.n_rows] > 0
                hit &= ne
                assert hit.mean() >= 0.10 and d[hit].all(), (int(hit.sum()), int(d[hit].sum()))


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("regime", re_.BOUND_REGIMES)
def test_oracle_meets_the_bound(pattern, regime):
    c = _data(pattern, regime)
    for alpha, beta in REGIMES[regime].scalars:
        y0 = c.y_in(beta)
        s, ab, n_r = re_.rounded_terms(c.rp, c.ci, c.va, c.x, y0, alpha, beta)
        ok = ~np.isnan(y0)
        worst = re_.assert_sum_close(_oracle_spmv(pattern, regime, alpha, beta)[ok], s[ok], ab[ok], n_r[ok],
                                     f"{pattern} {regime} ({alpha}, {beta})")
        print(f"{pattern} {regime} ({alpha}, {beta}): worst ratio {worst:.3g}")


def test_bound_has_no_hidden_slack():
    """One ulp of a subnormal sum beyond the bound fails: nothing like 1e-37 is added."""
    s, ab, n_r = np.array([2.0 ** -130]), np.array([2.0 ** -130]), np.array([1])
    re_.assert_sum_close(np.array([2.0 ** -130 + 2 * 2.0 ** -149], np.float32), s, ab, n_r)
    with pytest.raises(AssertionError):
        re_.assert_sum_close(np.array([2.0 ** -130 + 3 * 2.0 ** -149], np.float32), s, ab, n_r)
    with pytest.raises(AssertionError):
        re_.assert_sum_close(np.array([0.0], np.float32), s, ab, n_r)


def test_same_nanclass():
    nan2 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    want = np.array([1.0, np.nan, -0.0, np.inf], np.float32)
    re_.assert_same_nanclass(np.array([1.0, nan2, -0.0, np.inf], np.float32), want)
    for got in ([1.0, np.nan, 0.0, np.inf], [1.0, 1.0, -0.0, np.inf], [np.nan, np.nan, -0.0, np.inf],
                [1.0, np.nan, -0.0, -np.inf]):
        with pytest.raises(AssertionError):
            re_.assert_same_nanclass(np.array(got, np.float32), want)
    re_.assert_same_nanclass(np.array([2.0, np.nan, -0.0, np.inf], np.float32), want,
                             np.array([False, True, True, True]))


def test_oracle_generated_nan_bits():
    """inf - inf and 0 * inf on the oracle's host (x86): the sign bit set, payload zero."""
    rp = np.array([0, 2, 3], np.int64)
    ci = np.array([0, 1, 2], np.int32)
    va = np.array([1.0, -1.0, 0.0], np.float32)
    x = np.array([np.inf, np.inf, np.inf], np.float32)
    got = oracle.csr_spmv(rp, ci, va, x, np.zeros(2, np.float32), 1.0, 1.0)
    assert [hex(v) for v in got.view(np.uint32)] == [hex(re_.X86_NAN_BITS)] * 2
    for pattern in PATTERNS:
        assert re_.nan_patterns(_oracle_spmv(pattern, "fold_over", *REGIMES["fold_over"].scalars[0])) \
            == [hex(re_.X86_NAN_BITS)]
