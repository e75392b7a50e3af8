"""The layout registry of the -m gpu operand tests: one CSR case per pattern (Case), and for
every layout the build options, the sm_info fields that prove the layout was built, its
algorithms and the rows of each algorithm that are bit-identical to oracle.csr_spmv (Spec,
SPECS).  Matrix shape: 20011 rows (3 mod 4, two row blocks of <= 16384), 8 terms per row,
every 50th row empty with y = -0.0 there.  No GPU and no torch at import.
"""
import copy
import functools
import os
from dataclasses import dataclass
from typing import Callable

import numpy as np

import oracle
from gpu_util import bits, slab_order_for, uniform_csr

N_ROWS, N_COLS, WIDE_COLS = 20011, 120001, 400000
MERGE_IPT = int(os.environ.get("SM_MERGE_IPT", "8"))             # as tests/test_gpu_merge.py


# ---------------------------------------------------------------------------- matrices
class Case:
    """One CSR with its operands and its (cached) expected values."""

    def __init__(self, rp, ci, va, n_cols, seed):
        self.rp = np.ascontiguousarray(rp, np.int32)
        self.ci = np.ascontiguousarray(ci, np.int32)
        self.va = np.ascontiguousarray(va, np.float32)
        self.n_cols = n_cols
        self.n_rows = self.rp.size - 1
        self.lens = np.diff(self.rp.astype(np.int64))
        rng = np.random.default_rng(seed)
        self.x = rng.uniform(-1, 1, n_cols).astype(np.float32)
        self.y0 = rng.uniform(-1, 1, self.n_rows).astype(np.float32)
        self.y0[self.lens == 0] = -0.0
        self._ref, self._slab = {}, {}

    def with_data(self, va, x, y0):
        """The same pattern (and so the same masks) with other values, x and y0, and fresh
        caches."""
        c = copy.copy(self)
        c.va = np.ascontiguousarray(va, np.float32)
        c.x = np.ascontiguousarray(x, np.float32)
        c.y0 = np.ascontiguousarray(y0, np.float32)
        assert c.va.shape == self.va.shape and c.x.shape == (self.n_cols,) and c.y0.shape == (self.n_rows,)
        c._ref, c._slab = {}, {}
        return c

    def y_in(self, beta):
        y0 = self.y0.copy()
        if beta == 0.0:          # the reference multiplies: the NaN must survive
            y0[::97] = np.nan
        return y0

    def ref(self, alpha, beta):
        """(oracle.csr_spmv, sum|terms|) for x, y_in(beta)."""
        if (alpha, beta) not in self._ref:
            y0 = self.y_in(beta)
            want = oracle.csr_spmv(self.rp, self.ci, self.va, self.x, y0, alpha, beta)
            _, absum = oracle.csr_spmv_f64(self.rp, self.ci, self.va, self.x, y0, alpha, beta)
            self._ref[alpha, beta] = (want, absum)
        return self._ref[alpha, beta]

    def slab_ref(self, info, alpha, beta):
        key = (info["xband_slab_cols"], info["xband_slab0_cols"], info["xband_beta_last"], alpha, beta)
        if key not in self._slab:
            self._slab[key] = slab_order_for(info, self.rp, self.ci, self.va, self.x, self.y_in(beta),
                                             alpha, beta)
        return self._slab[key]

    def all_rows(self):
        return np.ones(self.n_rows, bool)

    def one_thread_rows(self):
        """Rows whose merge items lie in one thread's share (tests/test_gpu_merge.py)."""
        r = np.arange(self.n_rows, dtype=np.int64)
        start = self.rp[:-1].astype(np.int64) + r
        end = self.rp[1:].astype(np.int64) + r
        return (start // MERGE_IPT) == (end // MERGE_IPT)


def _table(seed=0, n=200):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def _csr(n_cols, seed, long_rows=None, codebook=True, short_every=0):
    """8 terms per row from uniform_csr on a 200-entry table, every 50th row empty, the rows
    of `long_rows` ({row: terms}) replaced by that many distinct sorted columns, and every
    `short_every`-th row cut to 3 terms."""
    table = _table(seed)
    rp, ci, va = uniform_csr(N_ROWS, n_cols, 8, seed=seed, table=table)
    rng = np.random.default_rng(seed + 1)
    rows = [ci[rp[r]:rp[r + 1]] for r in range(N_ROWS)]
    for r in range(1, N_ROWS, short_every or N_ROWS):
        rows[r] = rows[r][:3] if short_every else rows[r]
    for r in range(0, N_ROWS, 50):
        rows[r] = rows[r][:0]
    for r, k in (long_rows or {}).items():
        assert r % 50 != 0
        rows[r] = np.sort(rng.choice(n_cols, k, replace=False)).astype(np.int32)
    lens = np.array([c.size for c in rows], np.int64)
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci2 = np.concatenate(rows).astype(np.int32)
    if codebook:
        va2 = table[rng.integers(0, table.size, ci2.size)]
    else:
        va2 = rng.uniform(-1, 1, ci2.size).astype(np.float32)
    return rp2, ci2, va2


@functools.lru_cache(maxsize=None)
def _base(n_cols=N_COLS):
    return Case(*_csr(n_cols, seed=n_cols), n_cols, seed=5)


@functools.lru_cache(maxsize=None)
def _plain():
    c = Case(*_csr(N_COLS, seed=7, codebook=False), N_COLS, seed=6)
    assert np.unique(c.va.view(np.uint32)).size >= 256
    return c


@functools.lru_cache(maxsize=None)
def _long_sell():
    """One 3000-term row: past the stream kernel's 2048-term tile and the sliced ELL's cap."""
    return Case(*_csr(N_COLS, seed=9, long_rows={777: 3000}), N_COLS, seed=8)


@functools.lru_cache(maxsize=None)
def _long_csr():
    """One 5000-term row (split over workgroups), rows of 65 .. 300 terms (past
    SM_SERIAL_ROW_MAX: the wave reduction) and every 7th row of 3 terms (with their row end
    four merge items: a share of them falls inside one thread's 8, the merge path's
    bit-exact rows)."""
    long_rows = {777: 5000, 3: 65, 4099: 300, 16385: 129, 20009: 200, 20010: 66}
    return Case(*_csr(N_COLS, seed=11, long_rows=long_rows, codebook=False, short_every=7), N_COLS, seed=10)


@functools.lru_cache(maxsize=None)
def _hot(n_rows=N_ROWS, n_cols=1 << 17):
    """The power-law-column matrix of test_hot_bands_forced_skewed (tests/test_gpu_sell.py)."""
    rng = np.random.default_rng(8192)
    label = rng.permutation(n_cols).astype(np.int32)
    raw = np.minimum(rng.zipf(1.2, (n_rows, 12)) - 1, n_cols - 1)
    cols = np.sort(label[raw], axis=1)
    keep = np.ones_like(cols, bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    keep[::50] = False
    lens = keep.sum(axis=1)
    ci = cols[keep].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    table = rng.uniform(-1, 1, 255).astype(np.float32)
    va = table[rng.integers(0, 255, ci.size)]
    return Case(rp, ci, va, n_cols, seed=12)


@dataclass
class Spec:
    case: Case
    opts: dict
    expect: Callable[[dict], None]      # asserts the info() fields of the layout wanted
    algos: tuple
    masks: dict                         # algo -> rows bit-identical to oracle.csr_spmv (aligned x)
    band: bool = False                  # a band layout: served only for a 16-byte aligned x


def _want(info, **fields):
    for k, v in fields.items():
        got = info[k]
        assert (v(got) if callable(v) else got == v), (k, got, info)


def _pos(v):
    return v > 0


def _several(v):
    return v > 1


def _three_up(v):       # three or more slabs: their sum depends on the order
    return v >= 3


BAND_CODE = {"exact": 1, "blocked": 2, "gather": 3, "band2": 4, "cband": 5, "gcb": 6}


def _band_spec(kind, n_cols=N_COLS, **opts):
    c = _base(n_cols)
    slabs = opts.get("band_slabs")
    want_slabs = slabs if slabs else (1 if kind == "exact" else _three_up)
    return Spec(c, dict(layout=kind, **opts),
                lambda i: _want(i, has_xband=BAND_CODE[kind], xband_slabs=want_slabs),
                ("xband", "exact") if kind == "exact" else ("xband",) if kind in ("blocked", "gather", "gcb")
                else ("xband", "auto"),
                {a: c.all_rows() for a in ("xband", "auto", "exact")}, band=True)


def _sell_spec(case, masks_max, expect, **opts):
    m = case.lens <= masks_max
    return Spec(case, dict(layout="no_bands", **opts), lambda i: _want(i, has_xband=0, sweep_blocks=0, **expect),
                ("sell", "auto"), {"sell": m, "auto": m})


def _csr_spec(relabel):
    c = _long_csr()
    none = np.zeros(c.n_rows, bool)
    return Spec(c, dict(layout="no_bands", sell=0, relabel=relabel),
                lambda i: _want(i, has_xband=0, sell_slices=0, ccsell_chunks=0, n_long_rows=_pos,
                                max_row_nnz=5000, col_relabel=relabel),
                ("stream", "vector", "parity", "merge", "exact"),
                {"stream": c.lens <= 64, "vector": none, "parity": c.all_rows(), "exact": c.all_rows(),
                 "merge": c.one_thread_rows()})


# Widths: every case is built at 120001 columns (the forced 3-slab layouts get their three
# slabs there) except blocked / gather, whose builders choose the slab count themselves: 2 slabs
# of 65536 columns at 120001, where a reversed sum of the slab sums would equal the right one, so
# they are built at WIDE_COLS (400000 columns: 7 slabs).
SPECS = {
    "exact": lambda: _band_spec("exact"),
    "blocked": lambda: _band_spec("blocked", WIDE_COLS),
    "gather": lambda: _band_spec("gather", WIDE_COLS),
    **{f"{kind}-tall{tall}-slabs{slabs}":
       (lambda kind=kind, tall=tall, slabs=slabs:
        _band_spec(kind, N_COLS, band_tall=tall, band_slabs=slabs))
       for kind in ("band2", "cband") for tall in (0, 6) for slabs in (1, 3)},
    **{f"gcb-slabs{slabs}":
       (lambda slabs=slabs: _band_spec("gcb", N_COLS, band_slabs=slabs))
       for slabs in (1, 3)},
    "sweep": lambda: Spec(_base(N_COLS), dict(layout="sweep"),
                          lambda i: _want(i, sweep_blocks=_pos, has_xband=0), ("auto",),
                          {"auto": _base(N_COLS).all_rows()}),
    "sell-codebook": lambda: _sell_spec(_base(N_COLS), 2048, dict(sell_slices=_pos, sell_codebook=1)),
    "sell-plain": lambda: _sell_spec(_plain(), 2048, dict(sell_slices=_pos, sell_codebook=0)),
    "sell-relabel": lambda: _sell_spec(_base(N_COLS), 2048, dict(sell_slices=_pos, col_relabel=1), relabel=1),
    "sell-long-rows": lambda: _sell_spec(_long_sell(), 64, dict(sell_slices=_pos, n_long_rows=_pos,
                                                                max_row_nnz=3000), sell_max_len=64),
    "sell-ccsell": lambda: _sell_spec(_base(N_COLS), 1 << 30, dict(ccsell_chunks=_several, sell_slices=0),
                                      ccsell=1, ccsell_chunk_log2=14),
    "hot-bands": lambda: Spec(_hot(), dict(layout="no_bands", relabel=1, hot_cols=8192),
                              lambda i: _want(i, hot_cols=8192, sell_slices=_pos, col_relabel=1), ("sell",),
                              {"sell": np.zeros(_hot().n_rows, bool)}),
    "csr": lambda: _csr_spec(0),
    "csr-relabel": lambda: _csr_spec(1),
}


def _build(sm, spec):
    c = spec.case
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=spec.opts)
    info = M.info()
    spec.expect(info)
    return M, info


def _same(got, want, mask=None, what=""):
    g, w = bits(got), bits(want)
    if mask is not None:
        g, w = g[mask], w[mask]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} outputs differ, first at {bad[:5].tolist()}"


@functools.lru_cache(maxsize=None)
def _ragged(n_rows):
    """The matrix of test_spmm_ragged_all_panel_widths (3000 x 5000, lengths 0 .. 40, signed
    zeros); 3003 rows leave the last 16-row MFMA tile partial."""
    from gpu_util import skewed_csr
    n_cols = 5000
    rng = np.random.default_rng(21)
    lengths = rng.integers(0, 41, n_rows)
    lengths[::7] = 0
    lengths[1::11] = 16
    lengths[2::13] = 17
    rp, ci, va = skewed_csr(n_rows, n_cols, lengths, seed=22)
    va[::5] = -0.0
    return rp, ci, va, n_cols
