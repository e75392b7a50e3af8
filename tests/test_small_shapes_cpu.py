"""The grid of small cases (tests/small_shapes.py) checked on its own, no GPU: every case is a
valid CSR with the property it is named for, the slab geometry restated from b2_slabs gives the
one-column, 255-column and 256-column last slabs the grid is there for, the layout registry
builds a Spec for every layout at every grid point, and the three references the GPU tests
compare against -- oracle.csr_spmv, oracle.csr_spmv_f64 and gpu_util.slab_order_for -- agree
with one another on the grid within the bound the GPU tests use (gpu_util.TOL * sum|terms|),
bit for bit where there is one slab."""
import numpy as np
import pytest

import oracle
import small_shapes as ss
from gpu_util import assert_terms_close, bits, slab_order_spmv


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.build()


def test_grid_is_the_stated_one():
    assert len(ss.SHAPES) == 13 and len(set(ss.SHAPES)) == 13
    assert len(ss.GRID) == 13 * 6
    for need in ((1, 1), (1, 5), (5, 1), (2, 3), (63, 65), (64, 64), (65, 63), (255, 257), (256, 256),
                 (257, 255), (300, 513), (300, 767), (300, 768)):
        assert need in ss.SHAPES
    assert ss.SCALARS == ((1.3, 0.7), (0.5, 0.0))


@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_are_valid_and_as_named(shape):
    n_rows, n_cols = shape
    for pattern in ss.PATTERNS:
        for codebook in (True, False):
            c = ss.case(n_rows, n_cols, pattern, codebook)
            assert (c.n_rows, c.n_cols) == shape and c.rp[0] == 0 and c.rp[-1] == c.ci.size == c.va.size
            assert c.ci.size > 0 and (c.lens >= 0).all()
            assert c.ci.min() >= 0 and c.ci.max() < n_cols
            rows = [c.ci[c.rp[r]:c.rp[r + 1]] for r in range(n_rows)]
            assert all((np.diff(r) > 0).all() for r in rows), "rows strictly ascending"
            assert np.array_equal(bits(c.y0[c.lens == 0]), bits(np.full(int((c.lens == 0).sum()), -0.0)))
            n_vals = ss.distinct_values(c)
            if codebook:
                assert n_vals <= 200 and (n_vals == min(200, c.ci.size) or c.ci.size > 200)
            else:
                assert n_vals > 255 or c.ci.size < 256
            if pattern == "one":
                assert c.ci.tolist() == [n_cols - 1] and c.lens[-1] == 1
            elif pattern == "diag":
                k = min(n_rows, n_cols)
                assert c.ci.tolist() == list(range(k)) and (c.lens[:k] == 1).all() and (c.lens[k:] == 0).all()
            elif pattern == "last_col":
                assert (c.lens == 1).all() and (c.ci == n_cols - 1).all()
            elif pattern == "row0_full":
                assert c.lens[0] == n_cols and (c.lens[1:] == 0).all()
            elif pattern == "dense":
                assert (c.lens == n_cols).all()
            else:
                assert (c.lens[4::5] == 0).all() and (c.lens <= 3).all()
                full = np.delete(c.lens, np.arange(4, n_rows, 5))
                assert (full >= 1).all() and (n_cols < 30 or full.mean() > 2.5)
            assert np.isnan(c.y_in(0.0)[0]) and not np.isnan(c.y_in(0.7)).any()


def test_slab_widths_are_the_stated_ones():
    """b2_slabs restated (small_shapes.b2_slabs): the grid's reason for 513 / 767 / 768 and 257."""
    assert ss.slab_widths(513, 3) == [256, 256, 1]
    assert ss.slab_widths(767, 3) == [256, 256, 255]
    assert ss.slab_widths(768, 3) == [256, 256, 256]
    assert ss.slab_widths(257, 2) == [256, 1]
    assert ss.slab_widths(257, 3) == [256, 1]
    assert ss.slab_widths(256, 3) == [256] and ss.slab_widths(255, 2) == [255]
    for n_rows, n_cols in ss.SHAPES:
        for slabs in (1, 2, 3):
            w = ss.slab_widths(n_cols, slabs)
            sc, ns = ss.b2_slabs(n_cols, slabs)
            assert sum(w) == n_cols and len(w) == ns <= slabs and sc % 256 == 0 and min(w) >= 1
            assert all(x == sc for x in w[:-1])
    assert {len(ss.slab_widths(c, 3)) for _, c in ss.SHAPES} == {1, 2, 3}


def test_every_layout_has_a_spec_everywhere():
    import layout_specs
    assert set(layout_specs.SPECS) <= set(ss.LAYOUTS)
    for name, make in ss.LAYOUTS.items():
        for shape, pattern in ss.GRID:
            spec = make(shape, pattern)
            assert spec.case.n_rows == shape[0] and spec.case.n_cols == shape[1]
            assert set(spec.algos) <= set(spec.masks), name
            assert all(m.shape == (shape[0],) for m in spec.masks.values())


@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_references_agree(shape):
    """csr_spmv (fp32, the reference's order) against csr_spmv_f64, and the slab-order sum of 1, 2
    and 3 slabs, both hand-off forms, against both: within TOL * sum|terms|, NaN where y_in holds
    one; a single slab is csr_spmv bit for bit."""
    for pattern in ss.PATTERNS:
        for codebook in (True, False):
            c = ss.case(*shape, pattern, codebook)
            for alpha, beta in ss.SCALARS:
                want, absum = c.ref(alpha, beta)
                y0 = c.y_in(beta)
                f64, absum2 = oracle.csr_spmv_f64(c.rp, c.ci, c.va, c.x, y0, alpha, beta)
                assert np.array_equal(absum, absum2, equal_nan=True)
                assert_terms_close(want, f64, absum)
                if beta == 0.0:
                    assert np.isnan(want[0])
                for slabs in (1, 2, 3):
                    sc, ns = ss.b2_slabs(c.n_cols, slabs)
                    for beta_last in (False, True):
                        got = slab_order_spmv(c.rp, c.ci, c.va, c.x, y0, alpha, beta, sc, sc, beta_last=beta_last)
                        assert_terms_close(got, f64, absum)
                        assert_terms_close(got, want, absum)
                        if ns == 1:
                            assert np.array_equal(bits(got), bits(want))


def test_declines_table_conditions():
    """DECLINES (tests/test_gpu_small_shapes.py) names grid cases of known layouts only, and no
    layout is declined on every pattern of more than half of the shapes -- a layout declined that
    widely would not be tested on the grid.  (That the table is the host builders' own printout is
    checked where the builders run: tests/test_xband_builder.py.)"""
    from test_gpu_small_shapes import DECLINES, DEV_REQUESTS
    for layout, shape, pattern in DECLINES:
        assert layout in ss.LAYOUTS and shape in ss.SHAPES and pattern in ss.PATTERNS
    for layout in ss.LAYOUTS:
        wide = ss.declined_widely(DECLINES, layout)
        assert 2 * len(wide) <= len(ss.SHAPES), (layout, wide)
    # the device-buildable requests decline nothing on the grid
    assert not {k[0].split("-")[0] for k in DECLINES} & {r.split("-")[0] for r in DEV_REQUESTS}
