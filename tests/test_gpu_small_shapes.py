"""Every layout and every device builder on the grid of small cases (tests/small_shapes.py: 13
shapes from 1 x 1 to 300 x 768 at the edges of the wavefront, the 256-column slab pieces, the
serial-row limit and the 16-row MFMA tile, 6 patterns each).  One test per layout name, so a
layout that is wrong at a small shape fails alone.

Expected values come from outside the kernels: oracle.csr_spmv bit for bit where the header
promises the reference's order (one slab, exact, parity, sweep, sell rows up to their cap, stream
rows up to 64 terms, merge rows inside one thread), gpu_util.slab_order_for bit for bit for
several slabs, and gpu_util.TOL * sum|terms| everywhere.  x and y sit between guard words; every
product runs twice on one matrix and must give the same bits (the band hand-off words are back
at zero).  After each build the info() fields prove the layout asked for is the one that ran --
or, for a case listed in DECLINES, that nothing of it stays and AUTO's fall-back is right.
"""
import numpy as np
import pytest

import oracle
import small_shapes as ss
from gpu_util import (assert_guards, assert_guards_2d, assert_terms_close, bits, placed, placed_2d, to_host,
                      torch_dev)
from layout_specs import _same, _want

gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------- declines
# What a builder legitimately declines on the grid, from the printout of the stand-alone builder
# programs (tests/native/*_asan.cpp, "grid <layout> <shape> <pattern> declined";
# tests/test_xband_builder.py holds the two against each other) and, for hot-bands, from
# upload_sell_layouts.  A case listed here must decline, a case not listed must build.
_COLS_63_UP = ((63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (300, 513), (300, 767), (300, 768))
DECLINES = {
    # xband_build: a row's segment inside one band (here the whole row: fewer than 8192 columns
    # are one band) is longer than the rank field holds -- 62 terms for exact (6 rank bits), 30
    # for blocked and gather (5 bits).  Rows of 63 terms and more: row0_full and dense from 63
    # columns on.
    **{(kind, s, p): "row segment longer than the rank field"
       for kind in ("exact", "blocked", "gather") for s in _COLS_63_UP for p in ("row0_full", "dense")},
    # upload_sell_layouts: the hot prefix must leave a cold part (hot_cols < n_cols), and a
    # one-column matrix has none: the sliced ELL takes every term.
    **{("hot-bands", s, p): "hot_cols < n_cols leaves no hot prefix of one column"
       for s in ((1, 1), (5, 1)) for p in ss.PATTERNS},
}
# The layouts whose builders are host programs of their own (the stand-alone printout covers them).
HOST_BUILDER_LAYOUTS = tuple(n for n in ss.LAYOUTS if n not in ("sweep", "sell-relabel", "hot-bands", "csr",
                                                                 "csr-relabel"))


def _assert_nothing_stays(name, info):
    """A declined build leaves no part of the layout behind."""
    if name == "hot-bands":
        _want(info, hot_cols=0, has_xband=0, sell_slices=lambda v: v > 0, col_relabel=1)
    else:
        _want(info, has_xband=0, xband_slabs=0, xband_bands=0, xband_blocks=0)


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _spmv(M, c, xv, alpha, beta, algo):
    """One product, y between guards (one float past 16-byte alignment for odd row counts)."""
    y_off = c.n_rows % 2
    yv, yp = placed(c.y_in(beta), y_off)
    M.spmv(xv, yv, alpha, beta, algo=algo)
    got = to_host(yv).copy()
    assert_guards(yp, y_off, c.n_rows)
    return got


def _fallback_mask(c, info):
    """Rows AUTO sums in the reference's order without the declined layout: the sliced ELL's rows
    up to its 2048-term cap, else the stream kernel's up to SM_SERIAL_ROW_MAX."""
    return c.lens <= (2048 if info["sell_slices"] > 0 else ss.SERIAL_ROW_MAX)


# ---------------------------------------------------------------------------- a + b
@gpu
@pytest.mark.parametrize("name", list(ss.LAYOUTS))
def test_small_spmv(sm, name):
    """The whole grid through one layout: built or declined as DECLINES says, then every algorithm
    the layout serves at (1.3, 0.7) and (0.5, 0.0) (NaN in y), twice."""
    built = 0
    for shape, pattern in ss.GRID:
        spec = ss.LAYOUTS[name](shape, pattern)
        c = spec.case
        tag0 = f"{name} {shape[0]}x{shape[1]} {pattern}"
        M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=spec.opts)
        info = M.info()
        declined = (name, shape, pattern) in DECLINES
        try:
            if declined:
                _assert_nothing_stays(name, info)
            else:
                spec.expect(info)
                built += 1
        except AssertionError as e:
            raise AssertionError(f"{tag0}: {'listed in DECLINES but' if declined else 'not in DECLINES but'} {e}") from e
        multi = not declined and spec.band and info["xband_slabs"] > 1
        algos = ("auto",) if declined and name != "hot-bands" else spec.algos
        xv, xp = placed(c.x, 0)
        for alpha, beta in ss.SCALARS:
            want, absum = c.ref(alpha, beta)
            for algo in algos:
                tag = f"{tag0} {algo} alpha {alpha} beta {beta}"
                got = _spmv(M, c, xv, alpha, beta, algo)
                try:
                    assert_terms_close(got, want, absum)
                except AssertionError as e:
                    raise AssertionError(f"{tag}: {e}") from e
                if declined:
                    _same(got, want, _fallback_mask(c, info), tag + " vs oracle (fall-back)")
                elif algo == "exact":
                    _same(got, want, None, tag + " vs oracle")
                elif multi:
                    _same(got, c.slab_ref(info, alpha, beta), None, tag + " vs slab order")
                else:
                    _same(got, want, spec.masks[algo], tag + " vs oracle")
                again = _spmv(M, c, xv, alpha, beta, algo)
                _same(again, got, None, tag + " second run vs first")
        assert_guards(xp, 0, c.n_cols)
        assert np.array_equal(bits(to_host(xv)), bits(c.x)), tag0 + ": x was written"
    assert built == len(ss.GRID) - sum(1 for k in DECLINES if k[0] == name)


# ---------------------------------------------------------------------------- c
DEV_KEYS = ("has_xband", "xband_slabs", "xband_slab_cols", "xband_slab0_cols", "xband_blocks", "xband_bands",
            "xband_block_rows", "device_bytes", "sell_slices", "sell_codebook", "col_relabel", "n_long_rows",
            "max_row_nnz", "ccsell_chunks", "merge_stage")
RELABEL, SELL, GCB, MERGE_STAGE, BANDS = 1, 2, 4, 8, 16     # sm_built_on_device
# request -> (opts, the sm_built_on_device bits the device path must report, info fields, algo)
DEV_REQUESTS = {
    **{f"{kind}-slabs{slabs}": (dict(layout=kind, band_slabs=slabs), BANDS, dict(has_xband=code), "auto")
       for kind, code in (("band2", 4), ("cband", 5)) for slabs in (1, 3)},
    **{f"gcb-slabs{slabs}": (dict(layout="gcb", band_slabs=slabs), GCB, dict(has_xband=6), "xband")
       for slabs in (1, 3)},
    "no_bands": (dict(layout="no_bands"), SELL, dict(has_xband=0, col_relabel=0), "auto"),
    "no_bands-relabel": (dict(layout="no_bands", relabel=1), RELABEL | SELL, dict(has_xband=0, col_relabel=1), "auto"),
    "merge-stage": (dict(layout="no_bands", merge_stage=1), SELL | MERGE_STAGE, dict(merge_stage=1), "merge"),
}


@gpu
@pytest.mark.parametrize("request_name", list(DEV_REQUESTS))
def test_small_device_build_equals_host_build(sm, request_name):
    """Every grid case from device tensors with host_build = 0 and 1: the same info(), the same
    layout bytes (sm_layout_digest), the device builders reported where they apply (nothing on
    the grid is declined by them: no DEV_REQUESTS layout is in DECLINES), and one SpMV bit for
    bit between the two and within the bound of the oracle."""
    torch = torch_dev()
    opts, mask, fields, algo = DEV_REQUESTS[request_name]
    for shape, pattern in ss.GRID:
        c = ss.case(*shape, pattern, True)
        tag = f"{request_name} {shape[0]}x{shape[1]} {pattern}"
        dev = [torch.from_numpy(a).cuda() for a in (c.rp, c.ci, c.va)]
        D, H = (sm.SparseMatrix.from_csr(*dev, c.n_cols, opts=dict(opts, host_build=hb)) for hb in (0, 1))
        di, hi = D.info(), H.info()
        assert {k: di[k] for k in DEV_KEYS} == {k: hi[k] for k in DEV_KEYS}, (tag, di, hi)
        _want(di, sell_slices=(lambda v: v > 0) if opts["layout"] == "no_bands" else 0, **fields)
        if "band_slabs" in opts:
            _want(di, xband_slabs=ss.b2_slabs(c.n_cols, opts["band_slabs"])[1])
        dd, hd = D.layout_digest(), H.layout_digest()
        assert dd == hd, (tag, dd, hd)
        assert any(dd), (tag, dd)
        assert H.built_on_device() == 0, (tag, H.built_on_device())
        assert D.built_on_device() == mask, (tag, D.built_on_device(), mask)
        xv, xp = placed(c.x, 0)
        want, absum = c.ref(1.3, 0.7)
        got = [_spmv(M, c, xv, 1.3, 0.7, algo) for M in (D, H)]
        _same(got[0], got[1], None, tag + " device build vs host build")
        assert_terms_close(got[0], want, absum)
        assert_guards(xp, 0, c.n_cols)


# ---------------------------------------------------------------------------- d
@gpu
@pytest.mark.parametrize("n_rows", ss.SPMM_ROWS)
def test_small_spmm_rows_around_the_panels(sm, n_rows):
    """1, 15, 16 and 17 rows x 65 columns, n_rhs 1, 3, 4, 5 and 32, Y with ldy = n_rhs + 4 between
    guards: auto, vector and parity bit-exact against oracle.csr_spmm (n_rhs 4 and 32 take the
    row-panel kernels, the others the generic one); mfma within the bound at n_rhs = 32 and
    SM_ERR_NOT_SUPPORTED with Y unchanged at the others."""
    torch = torch_dev()
    for pattern in ss.SPMM_PATTERNS:
        rp, ci, va = ss.spmm_case(n_rows, pattern)
        M = sm.SparseMatrix.from_csr(rp, ci, va, ss.SPMM_COLS)
        for n_rhs in ss.SPMM_RHS:
            X, Y0 = ss.spmm_panels(n_rows, n_rhs)
            ldy = n_rhs + 4
            Xv, Xp = placed_2d(X, n_rhs, 0)
            for alpha, beta in ((1.3, 0.7), (-2.0, 0.0)):
                want = oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)
                for algo in ("auto", "vector", "parity", "mfma"):
                    tag = f"{pattern} {n_rows} rows N {n_rhs} {algo} alpha {alpha} beta {beta}"
                    Yv, Yp = placed_2d(Y0, ldy, 0)
                    if algo == "mfma" and n_rhs != 32:
                        before = Yp.view(torch.int32).cpu().numpy().copy()
                        with pytest.raises(sm.SparseMatrixError) as ei:
                            M.spmm(Xv, Yv, alpha, beta, algo=algo)
                        assert ei.value.status == 4, tag
                        torch.cuda.synchronize()
                        assert np.array_equal(Yp.view(torch.int32).cpu().numpy(), before), tag + ": Y changed"
                        continue
                    M.spmm(Xv, Yv, alpha, beta, algo=algo)
                    got = to_host(Yv)
                    if algo == "mfma":
                        absum = np.stack([oracle.csr_spmv_f64(rp.astype(np.int64), ci, va, np.ascontiguousarray(X[:, j]),
                                                              np.ascontiguousarray(Y0[:, j]), alpha, beta)[1]
                                          for j in range(n_rhs)], axis=1)
                        assert_terms_close(got, want, absum)
                    else:
                        _same(got, want, None, tag)
                    assert_guards_2d(Yp, 0, n_rows, n_rhs, ldy)
            assert_guards_2d(Xp, 0, ss.SPMM_COLS, n_rhs, n_rhs)
            assert np.array_equal(bits(to_host(Xv)), bits(X)), "X was written"
