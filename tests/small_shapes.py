"""The grid of small cases shared by tests/test_small_shapes_cpu.py, tests/test_gpu_small_shapes.py
and (restated in C++, tests/native/small_grid.h) the stand-alone builder programs: 13 shapes at
the edges of the code's own constants x 6 patterns, each with codebook values (a 200-entry
table) and with plain fp32 values, and for every layout of layout_specs.SPECS the Spec it takes
at a grid case.  No GPU and no torch at import.

Shapes, by the constant they sit on: 1 x 1, 1 x 5, 5 x 1, 2 x 3 (a row block, a slice, a sort
of one key); 63 / 64 / 65 (the wavefront, the sliced ELL's 64-lane slice, cband's 63 terms
per chunk, SM_SERIAL_ROW_MAX = 64 terms of a row); 255 / 256 / 257 (b2_slabs' 256-column
pieces, the sweep's 256-row blocks, kSellGroup = 4 slices of 64 rows, ccsell chunks of 2^8
columns); 300 x 513 / 767 / 768 (three slabs whose last is 1, 255 and 256 columns wide).  The
2048-term constants (kSellMaxLen, kCcMaxUnit, the stream kernel's tile) and the 4096 / 8192 /
16384 ones (row blocks, x windows) lie above every shape here: their edges are the long-row
cases of layout_specs.py and the ragged cases of test_gpu_devbuild*.py; the stream kernel's
tile (every size, at T - 1 / T / T + 1 terms) is the subject of stream_ref.py.

Patterns (rows strictly ascending, no RNG in the structure so that small_grid.h restates it
exactly):
  one        a single term at (last row, last column);
  diag       (r, r) for r < min(rows, cols);
  last_col   every row's only term is in the last column;
  row0_full  row 0 holds every column, the other rows are empty;
  dense      every position stored;
  sparse     rows with r % 5 == 4 empty; row r holds the distinct columns among
             (7 r + 1) % cols, (13 r + 5) % cols, (29 r + 11) % cols.
Empty rows get y0 = -0.0 (layout_specs.Case).
"""
import functools

import numpy as np

from layout_specs import BAND_CODE, Case, Spec, _pos, _table, _want

SHAPES = ((1, 1), (1, 5), (5, 1), (2, 3),
          (63, 65), (64, 64), (65, 63),
          (255, 257), (256, 256), (257, 255),
          (300, 513), (300, 767), (300, 768))
PATTERNS = ("one", "diag", "last_col", "row0_full", "dense", "sparse")
SCALARS = ((1.3, 0.7), (0.5, 0.0))      # the second: y_in puts NaN into y, beta = 0 multiplies it
SERIAL_ROW_MAX = 64                      # SM_SERIAL_ROW_MAX (include/sparsematrix.h)
SELL_LONG = 64                           # sell_max_len of the "sell-long-rows" spec
CC_CHUNK_LOG2 = 8                        # the smallest ccsell_chunk_log2: 256-column chunks
GRID = tuple((s, p) for s in SHAPES for p in PATTERNS)


def pattern_rows(n_rows, n_cols, pattern):
    """The column list of every row."""
    none = np.zeros(0, np.int64)
    rows = [none] * n_rows
    if pattern == "one":
        rows[n_rows - 1] = np.array([n_cols - 1])
    elif pattern == "diag":
        for r in range(min(n_rows, n_cols)):
            rows[r] = np.array([r])
    elif pattern == "last_col":
        rows = [np.array([n_cols - 1])] * n_rows
    elif pattern == "row0_full":
        rows[0] = np.arange(n_cols)
    elif pattern == "dense":
        rows = [np.arange(n_cols)] * n_rows
    elif pattern == "sparse":
        for r in range(n_rows):
            if r % 5 != 4:
                rows[r] = np.unique([(7 * r + 1) % n_cols, (13 * r + 5) % n_cols, (29 * r + 11) % n_cols])
    else:
        raise ValueError(pattern)
    return rows


@functools.lru_cache(maxsize=None)
def csr(n_rows, n_cols, pattern):
    rows = pattern_rows(n_rows, n_cols, pattern)
    lens = np.array([c.size for c in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return rp, ci


@functools.lru_cache(maxsize=None)
def case(n_rows, n_cols, pattern, codebook=True):
    """The Case of a grid point: values from a 200-entry table (term e takes entry
    (37 e + 11) % 200), or plain fp32 with more than 255 bit patterns where there are that
    many terms."""
    rp, ci = csr(n_rows, n_cols, pattern)
    seed = 1000 * SHAPES.index((n_rows, n_cols)) + 10 * PATTERNS.index(pattern)
    if codebook:
        table = _table(seed)
        va = table[(37 * np.arange(ci.size) + 11) % table.size]
    else:
        va = np.random.default_rng(seed + 1).uniform(-1, 1, ci.size).astype(np.float32)
        assert ci.size < 256 or np.unique(va.view(np.uint32)).size > 255
    return Case(rp, ci, va, n_cols, seed=seed + 2)


SPMM_ROWS = (1, 15, 16, 17)              # around the 16-row MFMA tile and the row panels
SPMM_COLS = 65
SPMM_PATTERNS = ("sparse", "row0_full")
SPMM_RHS = (1, 3, 4, 5, 32)


@functools.lru_cache(maxsize=None)
def spmm_case(n_rows, pattern):
    """(row_ptr, col_idx, val) of `pattern` at n_rows x 65 with plain values, some of them -0.0."""
    rows = pattern_rows(n_rows, SPMM_COLS, pattern)
    rp = np.concatenate([[0], np.cumsum([c.size for c in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    va = np.random.default_rng(500 + n_rows).uniform(-1, 1, ci.size).astype(np.float32)
    va[::5] = -0.0
    return rp, ci, va


@functools.lru_cache(maxsize=None)
def spmm_panels(n_rows, n_rhs):
    """(X, Y0) with zeros of both signs, as test_gpu_operands._panel."""
    rng = np.random.default_rng(600 + 40 * n_rows + n_rhs)
    X = rng.uniform(-1, 1, (SPMM_COLS, n_rhs)).astype(np.float32)
    X[::3] = 0.0
    X[1::9] = -0.0
    Y0 = rng.uniform(-1, 1, (n_rows, n_rhs)).astype(np.float32)
    Y0[::4] = -0.0
    return X, Y0


def distinct_values(c):
    return int(np.unique(c.va.view(np.uint32)).size)


# ---------------------------------------------------------------------------- slab geometry
def b2_slabs(n_cols, n_slabs):
    """band2_place.h b2_slabs with even slabs (slab0_permille = 1000), restated: (columns per
    slab, slabs) -- whole 256-column pieces."""
    sc = (-(-n_cols // n_slabs) + 255) & ~255
    return sc, -(-n_cols // sc)


def slab_widths(n_cols, n_slabs):
    """The width of every slab band2_build (and gcb_build: the same rounding) cuts."""
    sc, ns = b2_slabs(n_cols, n_slabs)
    return [min(n_cols, (s + 1) * sc) - s * sc for s in range(ns)]


# ---------------------------------------------------------------------------- specs
def _band(kind, c, **opts):
    """layout_specs._band_spec at a grid case.  The slab count is the builder's own: b2_slabs of
    the asked count for band2 / cband / gcb; one for exact, and for blocked and gather too
    (fewer than 8192 columns are one band, and a slab is whole bands)."""
    ns = b2_slabs(c.n_cols, opts["band_slabs"])[1] if "band_slabs" in opts else 1
    algos = (("xband", "exact") if kind == "exact" else ("xband",) if kind in ("blocked", "gather", "gcb")
             else ("xband", "auto"))
    return Spec(c, dict(layout=kind, **opts),
                lambda i: _want(i, has_xband=BAND_CODE[kind], xband_slabs=ns),
                algos, {a: c.all_rows() for a in ("xband", "auto", "exact")}, band=True)


def _sell(c, masks_max, expect, **opts):
    m = c.lens <= masks_max
    return Spec(c, dict(layout="no_bands", **opts),
                lambda i: _want(i, has_xband=0, sweep_blocks=0, n_long_rows=0, max_row_nnz=int(c.lens.max()),
                                **expect),
                ("sell", "auto"), {"sell": m, "auto": m})


def _csr(c, relabel):
    none = np.zeros(c.n_rows, bool)
    return Spec(c, dict(layout="no_bands", sell=0, relabel=relabel),
                lambda i: _want(i, has_xband=0, sell_slices=0, ccsell_chunks=0, n_long_rows=0,
                                max_row_nnz=int(c.lens.max()), col_relabel=relabel),
                ("stream", "vector", "parity", "merge", "exact"),
                {"stream": c.lens <= SERIAL_ROW_MAX, "vector": none, "parity": c.all_rows(),
                 "exact": c.all_rows(), "merge": c.one_thread_rows()})


def hot_cols_for(n_cols):
    """The hot prefix of the "hot-bands" spec: a quarter of the columns, at least one (8192 of
    2^17 columns in layout_specs: a sixteenth).  One column leaves no cold part: declined."""
    return max(1, n_cols // 4)


def _cb(s, p):
    return case(*s, p, True)


def _pl(s, p):
    return case(*s, p, False)


# The names of layout_specs.SPECS plus two slabs for band2 / cband (255 x 257: a second slab of
# one column); every entry maps a grid point to its Spec.
LAYOUTS = {
    "exact": lambda s, p: _band("exact", _cb(s, p)),
    "blocked": lambda s, p: _band("blocked", _cb(s, p)),
    "gather": lambda s, p: _band("gather", _cb(s, p)),
    **{f"{kind}-tall{tall}-slabs{slabs}":
       (lambda s, p, kind=kind, tall=tall, slabs=slabs: _band(kind, _cb(s, p), band_tall=tall, band_slabs=slabs))
       for kind in ("band2", "cband") for tall in (0, 6) for slabs in (1, 2, 3)},
    **{f"gcb-slabs{slabs}": (lambda s, p, slabs=slabs: _band("gcb", _cb(s, p), band_slabs=slabs))
       for slabs in (1, 3)},
    "sweep": lambda s, p: Spec(_cb(s, p), dict(layout="sweep"),
                               lambda i: _want(i, sweep_blocks=-(-s[0] // 256), has_xband=0), ("auto",),
                               {"auto": _cb(s, p).all_rows()}),
    "sell-codebook": lambda s, p: _sell(_cb(s, p), 2048, dict(sell_slices=_pos, sell_codebook=1)),
    # plain values of at most 255 bit patterns are a codebook: the builder takes the codebook form
    "sell-plain": lambda s, p: _sell(_pl(s, p), 2048,
                                     dict(sell_slices=_pos, sell_codebook=int(distinct_values(_pl(s, p)) <= 255))),
    "sell-relabel": lambda s, p: _sell(_cb(s, p), 2048, dict(sell_slices=_pos, col_relabel=1), relabel=1),
    "sell-long-rows": lambda s, p: _sell(_cb(s, p), SELL_LONG, dict(sell_slices=_pos), sell_max_len=SELL_LONG),
    "sell-ccsell": lambda s, p: _sell(_cb(s, p), 1 << 30,
                                      dict(ccsell_chunks=-(-s[1] >> CC_CHUNK_LOG2), sell_slices=0),
                                      ccsell=1, ccsell_chunk_log2=CC_CHUNK_LOG2),
    "hot-bands": lambda s, p: Spec(_cb(s, p), dict(layout="no_bands", relabel=1, hot_cols=hot_cols_for(s[1])),
                                   lambda i: _want(i, hot_cols=hot_cols_for(s[1]), sell_slices=_pos, col_relabel=1),
                                   ("sell",), {"sell": np.zeros(s[0], bool)}),
    "csr": lambda s, p: _csr(_pl(s, p), 0),
    "csr-relabel": lambda s, p: _csr(_pl(s, p), 1),
}


def declined_widely(declines, layout):
    """The shapes at which `layout` is declined on every pattern (the cap: at most half)."""
    return [s for s in SHAPES if all((layout, s, p) in declines for p in PATTERNS)]
