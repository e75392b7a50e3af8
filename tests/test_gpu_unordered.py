"""CSR rows whose columns are out of order or repeated (include/sparsematrix.h, "Rows"): the
input a COO-converted or concatenated graph gives.

Matrices: gpu_util.messy_csr -- 4099 x 40000, about 35k terms, rows reversed / shuffled / with
adjacent repeats / shuffled with repeats.  The contract under test: B is the sum of its stored
terms and "the reference's order" is the stored order (oracle.csr_spmv / csr_spmm, fp32, for
the bit-exact claims; oracle.csr_spmv_f64 with gpu_util.assert_terms_close, 1e-6 * sum|terms|,
for the bound); the layouts that need ascending columns are not built, forced or not, and
what remains serves the matrix; the transposition is the stable sort by column; sddmm gives
every stored term its own output; in-place updates reach every slot; sm_to_dense keeps the
last stored repeat; the reference stream sorts unsorted rows and refuses repeats.
"""
import functools

import numpy as np
import pytest

import oracle
import sddmm_ref
import table_ref
from gpu_util import (MESSY_COLS, MESSY_ROWS, MESSY_VARIANTS, assert_guards, assert_guards_2d, assert_terms_close,
                      bits, messy_csr, placed, placed_2d, to_dev, to_host, torch_dev, uniform_csr)
from layout_specs import BAND_CODE, Case, _same

pytestmark = pytest.mark.gpu

NOT_SUPPORTED = 4
SERIAL_MAX = 64          # SM_SERIAL_ROW_MAX: the stream kernel sums longer rows by a wave reduction
SELL_MAX_LEN = 2048      # the sliced ELL's default segment cap
SCALARS = [(1.0, 1.0), (1.3, 0.7), (0.5, 0.0)]
SPMV_ALGOS = ("auto", "xband", "exact", "sell", "stream", "vector", "parity", "merge")
REPEATED = ("repeated", "shuffled_repeated")


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


@functools.lru_cache(maxsize=None)
def _case(variant, codebook=True, long_rows=True):
    """The variant's CSR with x, y0 and the cached oracle results (layout_specs.Case)."""
    rp, ci, va = messy_csr(variant, seed=40 + MESSY_VARIANTS.index(variant), codebook=codebook, long_rows=long_rows)
    c = Case(rp, ci, va, MESSY_COLS, seed=60 + MESSY_VARIANTS.index(variant))
    assert c.n_rows == MESSY_ROWS and (c.lens[::50] == 0).all()
    desc = np.flatnonzero((np.diff(ci.astype(np.int64)) < 0) & (np.diff(_term_rows(rp)) == 0)).size
    rep = np.flatnonzero((np.diff(ci.astype(np.int64)) == 0) & (np.diff(_term_rows(rp)) == 0)).size
    if variant == "repeated":      # ascending, 3 adjacent repeats in every 5th row
        assert desc == 0 and rep == 3 * np.count_nonzero(c.lens == 11)
    else:
        assert desc > 1000
    assert (c.lens.max() == 2100) == long_rows and codebook == (np.unique(bits(va)).size <= 255)
    return c


def _term_rows(rp):
    return sddmm_ref.term_rows(rp)


def _has_repeat(c):
    key = _term_rows(c.rp) * c.n_cols + c.ci
    return np.unique(key).size != key.size


# ------------------------------------------------------- 1. every layout request, every algorithm
OPTION_SETS = {
    "exact": dict(layout="exact"), "blocked": dict(layout="blocked"), "gather": dict(layout="gather"),
    "band2": dict(layout="band2"), "cband": dict(layout="cband"), "gcb": dict(layout="gcb"),
    "sweep": dict(layout="sweep"), "bands": dict(layout="bands"), "auto": dict(),
    "no_bands": dict(layout="no_bands"),
    "no_bands-relabel": dict(layout="no_bands", relabel=1),
    "no_bands-sell0": dict(layout="no_bands", sell=0),
    "no_bands-maxlen64": dict(layout="no_bands", sell_max_len=64),
    "no_bands-ccsell": dict(layout="no_bands", ccsell=1, ccsell_chunk_log2=14),
    "no_bands-hot": dict(layout="no_bands", relabel=1, hot_cols=8192),
    "merge_stage": dict(merge_stage=1),
}
# The fixed band kinds take no row with 31 (blocked, gather) or 63 (exact) terms in one band, so
# on the base pattern its two long rows decline them for every variant; the pattern without the
# long rows is where "repeated" builds them and where a descending step alone declines them.
SHORT_SETS = ("exact", "blocked", "gather", "bands")
# Values outside any codebook (more than 255 bit patterns) for the plain forms: the sliced ELL with
# fp32 slots, and band2 -- not cband -- as the kind "bands" tries before the blocked one.
PLAIN_SETS = (("no_bands", True), ("no_bands-relabel", True), ("band2", True), ("bands", False), ("exact", False))
LAYOUT_CASES = ([(o, True, True) for o in OPTION_SETS] + [(o, False, True) for o in SHORT_SETS] +
                [(o, l, False) for o, l in PLAIN_SETS])


def _hot_split_applies(c, hot_cols):
    """The hot split (layouts.cpp) sorts every row's hot terms itself and hands them to the
    cband builder, which needs them strictly ascending: it is built unless some row stores a
    hot column twice.  Hot = the hot_cols columns of highest degree, ties in column order."""
    deg = np.bincount(c.ci, minlength=c.n_cols)
    rank = np.empty(c.n_cols, np.int64)
    rank[np.argsort(-deg, kind="stable")] = np.arange(c.n_cols)
    hot = rank[c.ci] < hot_cols
    key = (_term_rows(c.rp) * c.n_cols + c.ci)[hot]
    return np.unique(key).size == key.size


def _expect_layouts(variant, name, long_rows, codebook, info, c):
    """The contract's layouts for this request (include/sparsematrix.h, "Rows")."""
    opts = OPTION_SETS[name]
    tag = (variant, name, long_rows, codebook, info)
    if not codebook:
        assert info["sell_codebook"] == 0, tag
    elif name == "no_bands":
        assert info["sell_codebook"] == 1, tag
    # nothing here ascends strictly: no band2 / cband / gcb, no sweep, no column-chunked ELL
    assert info["has_xband"] not in (4, 5, 6) and info["sweep_blocks"] == 0 and info["ccsell_chunks"] == 0, tag
    fixed_ok = variant == "repeated" and not long_rows       # ascending with repeats, short segments
    if name in ("exact", "blocked", "gather"):
        assert info["has_xband"] == (BAND_CODE[name] if fixed_ok else 0), tag
    elif name == "bands":      # cband declines; its fall-back, the blocked kind, takes repeats only
        assert info["has_xband"] == (BAND_CODE["blocked"] if fixed_ok else 0), tag
    else:                      # forced strict kinds, AUTO below the band size floor, no_bands
        assert info["has_xband"] == 0, tag
    if info["has_xband"]:
        assert info["xband_slabs"] >= 1 and info["xband_blocks"] >= 1, tag
    # the sliced ELL wherever no band layout was built (and it is not switched off)
    assert (info["sell_slices"] > 0) == (opts.get("sell") != 0 and info["has_xband"] == 0), tag
    if opts.get("layout") == "no_bands":
        assert info["col_relabel"] == opts.get("relabel", 0), tag
        if "sell_max_len" in opts:
            assert info["n_long_rows"] > 0, tag
        want_hot = opts["hot_cols"] if "hot_cols" in opts and _hot_split_applies(c, opts["hot_cols"]) else 0
        assert info["hot_cols"] == want_hot, tag
        if "hot_cols" in opts:
            assert (want_hot == 0) == (variant in REPEATED), tag
    else:
        assert info["hot_cols"] == 0, tag
    assert info["merge_stage"] == opts.get("merge_stage", 0), tag
    assert info["max_row_nnz"] == c.lens.max() and info["nnz"] == c.ci.size, tag


def _route(info, algo, aligned):
    """What serves `algo` (capi.cpp launch_spmv_algo), as the kind of bit-exactness claimed for
    it by tests/layout_specs.py: all rows / a band layout / sell rows up to the segment cap /
    stream rows up to SM_SERIAL_ROW_MAX / merge rows inside one thread / none."""
    if algo in ("parity", "exact"):
        return "all"
    if algo == "vector":
        return "none"
    if algo == "merge":
        return "none" if info["merge_stage"] else "merge"    # the staged stream is column-sorted
    if algo in ("auto", "xband"):
        if info["sweep_blocks"] > 0:
            return "all"
        if info["has_xband"] and aligned:
            return "band"
        algo = "sell"
    if algo == "sell":
        if info["ccsell_chunks"] > 0:
            return "all"
        if info["sell_slices"] > 0:
            return "none" if info["hot_cols"] > 0 else "sell"
    return "stream"


@pytest.mark.parametrize("name,long_rows,codebook", LAYOUT_CASES,
                         ids=[f"{o}{'' if l else '-short'}{'' if cb else '-plain'}" for o, l, cb in LAYOUT_CASES])
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_every_layout_request_every_algorithm(sm, variant, name, long_rows, codebook):
    """Build with the option set, assert from info() which layouts exist, then every SpMV
    algorithm at three (alpha, beta) (NaN in y at beta = 0) with x 16-byte aligned and one float
    past: every result within 1e-6 * sum|terms|; parity and exact bit-identical to the stored
    order on every row; the others on the rows tests/layout_specs.py claims for what serves
    them.  The "bands" rows are the regression test of the fixed band builder: before its
    ascending-columns check a descending step put garbage into the rank and row fields."""
    c = _case(variant, codebook=codebook, long_rows=long_rows)
    opts = OPTION_SETS[name]
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=opts)
    info = M.info()
    _expect_layouts(variant, name, long_rows, codebook, info, c)
    cap = opts.get("sell_max_len", SELL_MAX_LEN)
    masks = {"all": c.all_rows(), "none": np.zeros(c.n_rows, bool), "sell": c.lens <= cap,
             "stream": c.lens <= SERIAL_MAX, "merge": c.one_thread_rows()}
    xs = {off: placed(c.x, off) for off in (0, 1)}
    for alpha, beta in SCALARS:
        want, absum = c.ref(alpha, beta)
        for algo in SPMV_ALGOS:
            for off in (0, 1):
                yv, yp = placed(c.y_in(beta), 0)
                M.spmv(xs[off][0], yv, alpha, beta, algo=algo)
                got = to_host(yv).copy()
                assert_guards(yp, 0, c.n_rows)
                tag = f"{variant} {name} {algo} x+{off} alpha {alpha} beta {beta}"
                assert_terms_close(got, want, absum)
                route = _route(info, algo, off == 0)
                if route == "band" and info["xband_slabs"] > 1:
                    _same(got, c.slab_ref(info, alpha, beta), None, tag + " vs slab order")
                else:
                    _same(got, want, masks["all" if route == "band" else route], tag + f" ({route}) vs oracle")
    for off, (xv, xp) in xs.items():
        assert_guards(xp, off, c.n_cols)
        assert np.array_equal(bits(to_host(xv)), bits(c.x)), "x was written"


# ------------------------------------------------------- 2. host and device ingestion agree
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_host_and_device_ingestion_agree(sm, variant):
    """The same CSR from device tensors with host_build 0 and 1 (the device builders re-implement
    the host builders' row rules): the layouts' digests and info equal the host-built matrix's,
    every SpMV bit for bit."""
    c = _case(variant)
    opts = dict(merge_stage=1)
    H = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols, opts=opts)
    hi = H.info()
    assert hi["merge_stage"] == 1 and H.layout_digest()[3] != 0
    dev = [to_dev(a) for a in (c.rp, c.ci, c.va)]
    x = to_dev(c.x)
    want = {}
    for algo in SPMV_ALGOS:
        y = to_dev(c.y0)
        H.spmv(x, y, 1.3, 0.7, algo=algo)
        want[algo] = to_host(y).copy()
    for hb in (0, 1):
        D = sm.SparseMatrix.from_csr(*dev, c.n_cols, opts=dict(opts, host_build=hb))
        di = D.info()
        assert di == dict(hi, device_bytes=di["device_bytes"]), (hb, di, hi)
        assert D.layout_digest() == H.layout_digest(), hb
        for a, b in zip(D.csr(), (c.rp, c.ci, c.va)):
            assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
        for algo in SPMV_ALGOS:
            y = to_dev(c.y0)
            D.spmv(x, y, 1.3, 0.7, algo=algo)
            _same(to_host(y), want[algo], None, f"{variant} host_build {hb} {algo}")


# ------------------------------------------------------- 3. SpMM
@functools.lru_cache(maxsize=None)
def _panel(n_rows, n_cols, n_rhs):
    rng = np.random.default_rng(700 + n_rhs)
    X = rng.uniform(-1, 1, (n_cols, n_rhs)).astype(np.float32)
    Y0 = rng.uniform(-1, 1, (n_rows, n_rhs)).astype(np.float32)
    Y0[::4] = -0.0
    return X, Y0


def _spmm_absum(c, X, Y0, alpha, beta):
    ab = np.empty(Y0.shape, np.float64)
    for j in range(Y0.shape[1]):
        ab[:, j] = oracle.csr_spmv_f64(c.rp.astype(np.int64), c.ci, c.va, np.ascontiguousarray(X[:, j]),
                                       np.ascontiguousarray(Y0[:, j]), alpha, beta)[1]
    return ab


@pytest.mark.parametrize("n_rhs", [4, 5, 12, 20, 32, 128])
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_spmm_stored_order(sm, variant, n_rhs):
    """Row-panel SpMM (contiguous, 16-byte aligned operands; 12 and 20 leave lanes of the panel
    kernels inactive) and the generic kernel (n_rhs = 5), "auto" and "vector": bit-identical to
    oracle.csr_spmm, the stored order."""
    c = _case(variant)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    X, Y0 = _panel(c.n_rows, c.n_cols, n_rhs)
    Xd = to_dev(X)
    assert Xd.data_ptr() % 16 == 0 and Xd.is_contiguous()
    for alpha, beta in ((1.3, 0.7), (-2.0, 0.0)):
        want = oracle.csr_spmm(c.rp.astype(np.int64), c.ci, c.va, X, Y0, alpha, beta)
        for algo in ("auto", "vector"):
            Yd = to_dev(Y0)
            assert Yd.data_ptr() % 16 == 0
            M.spmm(Xd, Yd, alpha, beta, algo=algo)
            _same(to_host(Yd), want, None, f"{variant} N {n_rhs} {algo} alpha {alpha} beta {beta}")


def _zero_sign_free(a):
    """As tests/test_gpu_spmm_mfma.py: -0.0 read as +0.0 (a tile's other rows add fma(0, x, acc))."""
    b = bits(a).copy()
    b[b == 0x80000000] = 0
    return b


@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_spmm_mfma_stored_order(sm, variant):
    """SM_ALGO_MFMA at n_rhs = 32: the fma chain in stored order (oracle.csr_spmm_fma), and the
    project's bound."""
    c = _case(variant)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    X, Y0 = _panel(c.n_rows, c.n_cols, 32)
    Xd = to_dev(X)
    for alpha, beta in ((1.3, 0.7), (-2.0, 0.0)):
        Yd = to_dev(Y0)
        M.spmm(Xd, Yd, alpha, beta, algo="mfma")
        got = to_host(Yd)
        model = oracle.csr_spmm_fma(c.rp.astype(np.int64), c.ci, c.va, X, Y0, alpha, beta)
        bad = np.flatnonzero(_zero_sign_free(got) != _zero_sign_free(model))
        assert bad.size == 0, f"{variant}: {bad.size} outputs differ from the fma chain, first {bad[:5].tolist()}"
        want = oracle.csr_spmm(c.rp.astype(np.int64), c.ci, c.va, X, Y0, alpha, beta)
        assert_terms_close(got, want, _spmm_absum(c, X, Y0, alpha, beta))


@pytest.mark.parametrize("n_rhs", [12, 20, 36, 68])
def test_spmm_rowpanel_inactive_lanes_store_nothing(sm, n_rhs):
    """Panel widths that are no power of two on a clean matrix, Y between guard words with
    ldy = n_rhs (no padding column to absorb a store): a lane of spmm_rowpanel_kernel /
    spmm_rowpanel2_kernel past the panel must neither load nor store.  Bit-identical to
    oracle.csr_spmm; Y's and X's guards unchanged."""
    n_rows, n_cols = 3003, 5000
    rp, ci, va = uniform_csr(n_rows, n_cols, 9, seed=31)
    M = sm.SparseMatrix.from_csr(rp, ci, va, n_cols)
    X, Y0 = _panel(n_rows, n_cols, n_rhs)
    Xv, Xp = placed_2d(X, n_rhs, 0)
    for alpha, beta in ((1.3, 0.7), (-2.0, 0.0)):
        want = oracle.csr_spmm(rp.astype(np.int64), ci, va, X, Y0, alpha, beta)
        for algo in ("auto", "vector"):
            Yv, Yp = placed_2d(Y0, n_rhs, 0)
            assert Yv.data_ptr() % 16 == 0 and Xv.data_ptr() % 16 == 0
            M.spmm(Xv, Yv, alpha, beta, algo=algo)
            _same(to_host(Yv), want, None, f"N {n_rhs} {algo} alpha {alpha} beta {beta}")
            assert_guards_2d(Yp, 0, n_rows, n_rhs, n_rhs)
    assert_guards_2d(Xp, 0, n_cols, n_rhs, n_rhs)
    assert np.array_equal(bits(to_host(Xv)), bits(X)), "X was written"


# ------------------------------------------------------- 4. transpose
def _cpu_transpose(rp, ci, va, n_cols):
    from test_gpu_transpose import cpu_transpose
    return cpu_transpose(rp, ci, va, n_cols)


@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_transpose_is_the_stable_sort_by_column(sm, variant):
    """M.T: row c of B^T holds column c's terms by ascending source row, equal rows in stored
    order, values bit for bit (the host transposer of tests/test_gpu_transpose.py).  The rows of
    B^T ascend -- with adjacent repeats where B repeats a term, so no layout that needs strictly
    ascending columns is built for it -- and spmv_t / spmm_t follow the oracle on the host
    transpose."""
    c = _case(variant)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    T = M.T
    t_rp, t_ci, t_va = _cpu_transpose(c.rp, c.ci, c.va, c.n_cols)
    g_rp, g_ci, g_va = T.csr()
    assert np.array_equal(g_rp, t_rp) and np.array_equal(g_ci, t_ci), "pattern of B^T"
    assert np.array_equal(bits(g_va), bits(t_va)), "values of B^T (bits)"
    steps = np.diff(t_ci.astype(np.int64))[np.diff(_term_rows(t_rp)) == 0]
    assert (steps >= 0).all() and ((steps == 0).any() == (variant in REPEATED))
    ti = T.info()
    assert (ti["n_rows"], ti["n_cols"], ti["nnz"]) == (c.n_cols, c.n_rows, c.ci.size)
    assert ti["has_xband"] == 0 and ti["sweep_blocks"] == 0 and ti["ccsell_chunks"] == 0, ti
    for layout in ("cband", "gcb", "sweep"):    # forced on B^T: built only where its rows strictly ascend
        F = M.transposed(opts=dict(layout=layout)).info()
        built = F["sweep_blocks"] > 0 if layout == "sweep" else F["has_xband"] == BAND_CODE[layout]
        assert built == (variant not in REPEATED), (layout, F)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, c.n_rows).astype(np.float32)
    y0 = rng.uniform(-1, 1, c.n_cols).astype(np.float32)
    t_lens = np.diff(t_rp.astype(np.int64))
    for alpha, beta in SCALARS:
        want = oracle.csr_spmv(t_rp, t_ci, t_va, x, y0, alpha, beta)
        _, absum = oracle.csr_spmv_f64(t_rp, t_ci, t_va, x, y0, alpha, beta)
        for algo in ("auto", "parity", "exact", "stream"):
            y = to_dev(y0)
            M.spmv_t(to_dev(x), y, alpha, beta, algo=algo)
            got = to_host(y)
            assert_terms_close(got, want, absum)
            mask = None if algo in ("parity", "exact") else t_lens <= SERIAL_MAX
            _same(got, want, mask, f"{variant} spmv_t {algo} alpha {alpha} beta {beta}")
    X, Y0 = _panel(c.n_cols, c.n_rows, 12)
    Yd = to_dev(Y0)
    M.spmm_t(to_dev(X), Yd, 1.3, 0.7)
    _same(to_host(Yd), oracle.csr_spmm(t_rp.astype(np.int64), t_ci, t_va, X, Y0, 1.3, 0.7), None, "spmm_t")


# ------------------------------------------------------- 5. SDDMM and the table gradient
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_sddmm_every_stored_term(sm, variant):
    """out[e] for every stored term in CSR order at N = 1, 4, 32: PARITY is the restated order
    by bits, AUTO within tests/sddmm_ref.py's bound, and the stored repeats of one (row, column)
    get bit-equal dots."""
    c = _case(variant)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    key = _term_rows(c.rp) * c.n_cols + c.ci
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    assert (first.size != key.size) == (variant in REPEATED)
    for N in (1, 4, 32):
        G, X, out0 = sddmm_ref.grid_inputs(c.n_rows, c.n_cols, c.ci.size, N)
        Gd, Xd = to_dev(G), to_dev(X)
        for alpha, beta in ((1.3, 0.0), (-0.7, 0.5)):
            want32 = sddmm_ref.parity(c.rp, c.ci, G, X, out0, alpha, beta)
            want64, absum = sddmm_ref.exact(c.rp, c.ci, G, X, out0, alpha, beta)
            for algo in ("parity", "auto"):
                got = to_host(M.sddmm(Gd, Xd, to_dev(out0), alpha, beta, algo=algo))
                tag = f"{variant} N {N} {algo} alpha {alpha} beta {beta}"
                if algo == "parity":
                    assert np.array_equal(bits(got), bits(want32)), tag + ": not the restated order"
                assert_terms_close(got, want64, absum)
                if beta == 0.0:      # nothing of out0 left: a (row, column)'s terms share one dot
                    assert np.array_equal(bits(got), bits(got[first][inv])), tag + ": repeats differ"


T_IDS = 200


def _ids_for(c):
    return np.random.default_rng(34).integers(0, T_IDS - 1, c.ci.size).astype(np.uint8)


def _make_table(seed):
    return np.random.default_rng(seed).uniform(-1, 1, T_IDS).astype(np.float32)


@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_table_gradient(sm, variant):
    """from_csr_ids on the same patterns: sddmm_table is the stated order (tests/table_ref.py fed
    with the GPU's own dots) bit for bit and within the header's bound of the float64 value."""
    c = _case(variant)
    ids, table = _ids_for(c), _make_table(31)
    M = sm.SparseMatrix.from_csr_ids(c.rp, c.ci, ids, table, c.n_cols)
    assert M.info()["table_size"] == T_IDS
    assert np.array_equal(bits(M.csr()[2]), bits(table[ids]))
    U = 2.0 ** -24
    for N in (1, 4, 32):
        G, X, _ = sddmm_ref.grid_inputs(c.n_rows, c.n_cols, c.ci.size, N)
        out0 = np.random.default_rng(600 + N).uniform(-1, 1, T_IDS).astype(np.float32)
        Gd, Xd = to_dev(G), to_dev(X)
        for algo in ("auto", "parity"):
            d = to_host(M.sddmm(Gd, Xd, alpha=1.0, beta=0.0, algo=algo))
            p = table_ref.chunk_partials(d, ids, T_IDS)
            panel = algo != "parity" and N >= 4 and N % 4 == 0
            for alpha, beta in ((1.3, 0.0), (-0.7, 0.5)):
                want = table_ref.finish_partials(p, out0, alpha, beta)
                got = to_host(M.sddmm_table(Gd, Xd, out=to_dev(out0), alpha=alpha, beta=beta, algo=algo))
                tag = f"{variant} N {N} {algo} alpha {alpha} beta {beta}"
                assert np.array_equal(bits(got), bits(want)), tag + ": not the stated order"
                val, absum, R = table_ref.exact_by_id(c.rp, c.ci, ids, T_IDS, G, X, out0, alpha, beta, panel)
                err = np.abs(got.astype(np.float64) - val)
                assert np.all(err <= R * U * absum + 1e-37), tag


@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_table_updates_reach_every_slot(sm, variant):
    """table_updatable = 1: after set_table / axpy_table the matrix is what a fresh build from
    the new table gives -- CSR, digests and every product bit for bit (table_ref.assert_same_matrix)."""
    c = _case(variant)
    ids = _ids_for(c)
    t1, t2, delta = _make_table(31), _make_table(32), _make_table(33)
    t2[9] = t2[5]
    t2.view(np.uint32)[20:20 + table_ref.SPECIAL_BITS.size] = table_ref.SPECIAL_BITS
    build = lambda t: sm.SparseMatrix.from_csr_ids(c.rp, c.ci, ids, t, c.n_cols, opts=dict(table_updatable=1))
    ops = table_ref.Operands(c.n_rows, c.n_cols)
    M, F = build(t1), build(t2)
    info = M.info()
    assert info["table_updatable"] == 1 and F.info() == info
    assert info["has_xband"] == 0 and info["sweep_blocks"] == 0 and info["ccsell_chunks"] == 0
    M.set_table(to_dev(t2))
    assert np.array_equal(bits(M.csr()[2]), bits(t2[ids]))
    table_ref.assert_same_matrix(M, F, ops, f"{variant} set_table:")
    M2 = build(t1)
    M2.axpy_table(-0.37, to_dev(delta))
    table_ref.assert_same_matrix(M2, build(table_ref.axpy_reference(t1, -0.37, delta)), ops, f"{variant} axpy_table:")


# ------------------------------------------------------- 6. in-place values
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_value_updates_reach_every_slot(sm, variant):
    """updatable = 1: set_values and axpy_values against fresh builds from the new values, every
    algorithm bit for bit (the scheme and helpers of tests/test_gpu_update_values.py); the
    transposed companion follows, and takes values in the source's order through the C ABI."""
    from sparsematrix_amd import _lib
    from test_gpu_update_values import Operands, assert_same_matrix, axpy_reference, check_case, new_values
    torch = torch_dev()
    c = _case(variant)
    check_case(sm, c.rp, c.ci, c.n_cols, {}, expect=dict(has_xband=0, sweep_blocks=0, ccsell_chunks=0),
               companion=True)
    # sm_create_transpose(updatable) of a plain matrix, updated in the source's order
    nnz = c.ci.size
    val1, val2, delta = new_values(nnz, 1, special=False), new_values(nnz, 2), new_values(nnz, 3, special=False)
    src = sm.SparseMatrix.from_csr(c.rp, c.ci, val1, c.n_cols)
    T = src.transposed(opts=dict(updatable=1))
    assert T.info()["updatable"] == 1
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    d2, dd = to_dev(val2), to_dev(delta)
    ops_t = Operands(c.n_cols, c.n_rows)
    fresh_t = lambda v: sm.SparseMatrix.from_csr(c.rp, c.ci, v, c.n_cols, opts=dict(updatable=1)).transposed()
    assert L.sm_set_values(T._h, d2.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    assert_same_matrix(T, fresh_t(val2), ops_t, f"{variant} set, source order:")
    assert L.sm_axpy_values(T._h, -0.37, dd.data_ptr(), _lib.SM_VALUES_SOURCE, stream) == 0
    assert_same_matrix(T, fresh_t(axpy_reference(val2, -0.37, delta)), ops_t, f"{variant} axpy, source order:")
    torch.cuda.synchronize()


# ------------------------------------------------------- 7. reference stream and native
def _dense_twin(c):
    """The dense index equivalent to the CSR (Trans: S = dm^T, so B = dm) with its table, and the
    oracle's restated reference built from it."""
    table = np.unique(c.va)
    assert table.size <= 255 and not _has_repeat(c)
    dm = np.full((c.n_rows, c.n_cols), 255, np.uint8)
    dm[_term_rows(c.rp), c.ci] = np.searchsorted(table, c.va).astype(np.uint8)
    return dm, table, oracle.RefModel(dm, c.n_rows, c.n_cols, c.n_cols, table, table.size, trans=True)


@pytest.mark.parametrize("variant", ["reversed", "shuffled"])
def test_reference_stream_of_unsorted_rows(sm, variant):
    """sm_build_ref_stream sorts: the stream equals the one CopyForm gives for the equivalent
    dense index (and the restated reference's), and AddMatMat straight from it (SM_ALGO_NATIVE)
    at m = 1 and 3 is the reference's, bit for bit."""
    c = _case(variant)
    dm, table, ref = _dense_twin(c)
    twin = sm.SparseMatrix(dm, c.n_rows, c.n_cols, c.n_cols, table, table.size, sm.SblasTrans)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    assert M.info()["has_ref_stream"] == 0
    M.build_ref_stream(table)
    assert M.info()["has_ref_stream"] == 1
    got, want, model = M.ref_stream(), twin.ref_stream(), ref.stream()
    for k in ("rows", "cols", "pos", "val", "panel_row_off", "panel_col_off", "panel_begin", "panel_end"):
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[k], getattr(model, k)), k + " (restated reference)"
    assert M == twin
    k, n = c.n_cols, c.n_rows
    rng = np.random.default_rng(9)
    for m in (1, 3):
        A = rng.uniform(-1, 1, (m, k)).astype(np.float32)
        C = rng.uniform(-1, 1, (m, n)).astype(np.float32)
        for alpha, beta in ((1.3, 0.7), (1.0, 0.0)):
            wantc = ref.add_mat_mat(A.reshape(-1), m, k, C.reshape(-1), n, alpha, beta)
            c_d = to_dev(C.reshape(-1))
            M.AddMatMat(to_dev(A.reshape(-1)), m, k, c_d, n, alpha, beta, algo="native")
            assert np.array_equal(bits(to_host(c_d)), bits(wantc)), (variant, m, alpha, beta)


@pytest.mark.parametrize("variant", REPEATED)
def test_reference_stream_refuses_repeats(sm, variant):
    """A (row, column) stored twice: sm_build_ref_stream is SM_ERR_NOT_SUPPORTED (the reference's
    format comes from a dense index and cannot hold it; the native kernel ranks a batch's entries
    by one bit per position and would drop one) and leaves the matrix as it was."""
    c = _case(variant)
    assert _has_repeat(c)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    x = to_dev(c.x)
    before = to_dev(c.y0)
    M.spmv(x, before, 1.3, 0.7)
    info = M.info()
    for table in (None, np.unique(c.va)):
        with pytest.raises(sm.SparseMatrixError) as e:
            M.build_ref_stream(table)
        assert e.value.status == NOT_SUPPORTED and "more than once" in str(e.value)
    assert M.info() == info and info["has_ref_stream"] == 0
    with pytest.raises(sm.SparseMatrixError) as e:
        M.ref_stream()
    assert e.value.status == NOT_SUPPORTED
    for m in (1, 3):
        a = to_dev(np.zeros(m * c.n_cols, np.float32))
        cc = to_dev(np.zeros(m * c.n_rows, np.float32))
        with pytest.raises(sm.SparseMatrixError) as e:
            M.AddMatMat(a, m, c.n_cols, cc, c.n_rows, 1.0, 1.0, algo="native")
        assert e.value.status == NOT_SUPPORTED
    after = to_dev(c.y0)
    M.spmv(x, after, 1.3, 0.7)
    _same(to_host(after), to_host(before), None, "spmv after the refused call")


# ------------------------------------------------------- 8. CopyTo
COPY_ROWS = 400     # S (n_cols x n_rows) of the whole matrix is 656 MB dense: the first 400 rows of B


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("variant", ["repeated", "shuffled"])
def test_copy_to_keeps_the_last_stored_repeat(sm, variant, trans):
    """sm_to_dense assigns: the last stored of several repeats at a repeated position, the one
    value elsewhere, zero where nothing is stored -- for both `trans`.  For "shuffled" (no
    repeats) that is the dense matrix of the sorted CSR.  On the first 400 rows of the variant
    (80 of them with repeats), all 40000 columns."""
    c = _case(variant)
    nnz = int(c.rp[COPY_ROWS])
    rp, ci, va = c.rp[:COPY_ROWS + 1], c.ci[:nnz], c.va[:nnz]
    M = sm.SparseMatrix.from_csr(rp, ci, va, c.n_cols)
    rows = _term_rows(rp)
    key = rows * c.n_cols + ci
    pos, last = np.unique(key[::-1], return_index=True)      # per position: first in reversed = last stored
    assert (pos.size != nnz) == (variant == "repeated")
    dense = np.zeros((COPY_ROWS, c.n_cols), np.float32)      # B
    dense.reshape(-1)[pos] = va[::-1][last]
    if variant == "shuffled":
        o = np.lexsort((ci, rows))
        srt = np.zeros_like(dense)
        srt[rows[o], ci[o]] = va[o]
        assert np.array_equal(bits(srt), bits(dense))
    # S = B^T is n_cols x n_rows: NoTrans writes S, Trans writes S^T = B
    want = dense if trans else np.ascontiguousarray(dense.T)
    stride = want.shape[1] + 3
    got = M.CopyTo(None, stride, trans)[: want.shape[0] * stride].reshape(want.shape[0], stride)
    assert np.array_equal(bits(got[:, : want.shape[1]]), bits(want))
    assert not got[:, want.shape[1]:].any(), "padding columns are zeroed"


# ------------------------------------------------------- 9. AddMatMat on the device
@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("variant", MESSY_VARIANTS)
def test_addmatmat_device_odd_leading_dimensions(sm, variant, m):
    """C (m x n, ldc n + 1) = alpha A (m x k, lda k + 3) S + beta C on the device, "auto" and
    "parity": row i of C is the SpMV of B with x = row i of A, so the oracle is oracle.csr_spmv
    per row.  Parity on every m, and auto at m > 1 (reference-order routes), are bit-identical;
    auto at m = 1 is the AUTO SpMV: within the bound.  C's padding and guards unchanged."""
    c = _case(variant)
    M = sm.SparseMatrix.from_csr(c.rp, c.ci, c.va, c.n_cols)
    k, n = M.NumRows(), M.NumCols()
    assert (k, n) == (c.n_cols, c.n_rows)
    lda, ldc = k + 3, n + 1
    rng = np.random.default_rng(100 + m)
    A = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    C = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    Av, Ap = placed_2d(A, lda, 0)
    for alpha, beta in ((1.3, 0.7), (1.0, 0.0)):
        want = np.stack([oracle.csr_spmv(c.rp, c.ci, c.va, A[i], C[i], alpha, beta) for i in range(m)])
        absum = np.stack([oracle.csr_spmv_f64(c.rp, c.ci, c.va, A[i], C[i], alpha, beta)[1] for i in range(m)])
        for algo in ("auto", "parity"):
            Cv, Cp = placed_2d(C, ldc, 0)
            M.AddMatMat(Ap[8:], m, lda, Cp[8:], ldc, alpha, beta, algo=algo)
            got = to_host(Cv)
            tag = f"{variant} m {m} {algo} alpha {alpha} beta {beta}"
            assert_terms_close(got, want, absum)
            if algo == "parity" or m > 1:
                _same(got, want, None, tag)
            assert_guards_2d(Cp, 0, m, n, ldc)
    assert_guards_2d(Ap, 0, m, k, lda)
    assert np.array_equal(bits(to_host(Av)), bits(A)), "A was written"
