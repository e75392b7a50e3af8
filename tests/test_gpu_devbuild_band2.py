"""Device builder of the balanced bands (sparsematrix_amd/csrc/builddev_band2.hip): from a
device CSR the band2 / cband layout is built on the GPU.  Every case builds one CSR both ways
(sm_build_opts.host_build = 0 / 1) and checks the reported layout, the layout's bytes
(sm_layout_digest: geometry, tile -> band offsets, band columns, entry words, table), which
builder ran (sm_built_on_device bit 16), one SpMV bit for bit between the two, and that SpMV
against the slab-order restatement of the reference's sum (gpu_util.slab_order_for)."""
import time

import numpy as np
import pytest

import oracle
from gpu_util import bits, slab_order_for, to_host, torch_dev, uniform_csr

pytestmark = pytest.mark.gpu

KEYS = ("has_xband", "xband_slabs", "xband_slab_cols", "xband_slab0_cols", "xband_blocks", "xband_bands",
        "xband_block_rows", "device_bytes", "sell_slices")
BANDS = 16   # sm_built_on_device: the balanced bands


@pytest.fixture(scope="module")
def sm():
    torch_dev()
    oracle.build()
    import sparsematrix_amd
    sparsematrix_amd.load()
    return sparsematrix_amd


def _both(sm, rp, ci, va, n_cols, opts, built=True):
    """Device and host builds of one CSR (device tensors): same info and layout bytes.  `built`:
    a band2 / cband layout is expected, made by the device builder under host_build = 0."""
    torch = torch_dev()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a for a in (rp, ci, va)]
    assert all(a.is_cuda for a in dev)
    out = []
    for hb in (0, 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = sm.SparseMatrix.from_csr(*dev, n_cols, opts=dict(opts, host_build=hb))
        torch.cuda.synchronize()
        out.append((M, time.perf_counter() - t0))
    (D, td), (H, th) = out
    di, hi = D.info(), H.info()
    print(f"band build: device {td:.3f} s, host {th:.3f} s", {k: di[k] for k in KEYS})
    assert {k: di[k] for k in KEYS} == {k: hi[k] for k in KEYS}, (di, hi)
    dd, hd = D.layout_digest(), H.layout_digest()
    assert dd == hd, (dd, hd)
    assert H.built_on_device() & BANDS == 0
    if built:
        assert di["has_xband"] in (4, 5), di
        assert dd[1] != 0 and dd[2] != 0, dd
        assert D.built_on_device() & BANDS == BANDS, D.built_on_device()
    else:
        assert D.built_on_device() & BANDS == 0
    return D, H, di, td, th


def _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, seed, oracle_check=True):
    x = np.random.default_rng(seed).uniform(-1, 1, n_cols).astype(np.float32)
    y0 = np.random.default_rng(seed + 1).uniform(-1, 1, n_rows).astype(np.float32)
    torch = torch_dev()
    yd, yh = torch.from_numpy(y0).cuda(), torch.from_numpy(y0).cuda()
    xd = torch.from_numpy(x).cuda()
    D.spmv(xd, yd, 1.3, 0.5)
    H.spmv(xd, yh, 1.3, 0.5)
    assert torch.equal(yd.view(torch.int32), yh.view(torch.int32))
    if oracle_check:
        rp, ci, va = (a if isinstance(a, np.ndarray) else to_host(a) for a in (rp, ci, va))
        want = (oracle.csr_spmv(rp, ci, va, x, y0, 1.3, 0.5) if info["xband_slabs"] == 1
                else slab_order_for(info, rp, ci, va, x, y0, 1.3, 0.5))
        assert np.array_equal(bits(to_host(yd)), bits(want))


def _csr_from_rows(rows, n_cols, seed, codebook=True):
    """CSR of a list of sorted, distinct column arrays; 255-value codebook or plain values."""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = (np.concatenate(rows) if rp[-1] else np.zeros(0)).astype(np.int32)
    rng = np.random.default_rng(seed)
    if codebook:
        va = rng.uniform(-1, 1, 255).astype(np.float32)[rng.integers(0, 255, ci.size)]
    else:
        va = rng.uniform(-1, 1, ci.size).astype(np.float32)
    return rp, ci, va


_UNIFORM = {}


def _uniform(n_rows, n_cols, per_row):
    """One CSR per shape, shared by the cases; never modified."""
    key = (n_rows, n_cols, per_row)
    if key not in _UNIFORM:
        _UNIFORM[key] = uniform_csr(n_rows, n_cols, per_row, seed=n_rows % 97 + per_row)
    return _UNIFORM[key]


@pytest.mark.parametrize("n_rows,n_cols,per_row", [(5000, 1000, 5), (40000, 20000, 3), (9000, 70001, 40),
                                                   (1, 50000, 30), (16384, 8192, 1)])
@pytest.mark.parametrize("kind", ["band2", "cband"])
@pytest.mark.parametrize("tall", [0, 6])
@pytest.mark.parametrize("slabs", [1, 0, 3])
def test_devbuild_band2_uniform(sm, n_rows, n_cols, per_row, kind, tall, slabs):
    """Forced band2 / cband on uniform shapes (three row blocks with a partial last one, one row,
    one term per row), the dma3 and wide geometries, one, AUTO's and three slabs."""
    rp, ci, va = _uniform(n_rows, n_cols, per_row)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout=kind, band_tall=tall, band_slabs=slabs))
    assert info["has_xband"] == (4 if kind == "band2" else 5), info
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 3)


@pytest.mark.parametrize("width", [40, 90])
@pytest.mark.parametrize("kind", ["band2", "cband"])
def test_devbuild_band2_consecutive_columns(sm, width, kind):
    """Rows of 40 and 90 consecutive columns: band2 cuts a band after 14 terms of a row (the
    rank field), cband after 63 (one chunk)."""
    n_rows, n_cols = 6000, 7000
    rng = np.random.default_rng(width)
    start = rng.integers(0, n_cols - width, n_rows)
    rows = [np.arange(s, s + width) for s in start]
    rp, ci, va = _csr_from_rows(rows, n_cols, 5)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout=kind))
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 4)


@pytest.mark.parametrize("kind", ["band2", "cband"])
def test_devbuild_band2_hub_columns(sm, kind):
    """Every row holds column 4097 and every third row column 9000: a column's terms in one row
    block exceed a band, so it is split by rows over one-column bands."""
    n_rows, n_cols = 40000, 20000
    rng = np.random.default_rng(11)
    extra = rng.integers(0, n_cols, (n_rows, 4))
    rows = []
    for r in range(n_rows):
        c = [4097] + ([9000] if r % 3 == 0 else []) + extra[r].tolist()
        rows.append(np.unique(c))
    rp, ci, va = _csr_from_rows(rows, n_cols, 6)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout=kind))
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 5)


@pytest.mark.parametrize("kind", ["band2", "cband"])
def test_devbuild_band2_ragged(sm, kind):
    """Empty rows, a 3000-term row, column ranges without terms, a partial last row block."""
    n_rows, n_cols = 20000, 600000
    rng = np.random.default_rng(12)
    rows = []
    for r in range(n_rows):
        k = 3000 if r == 777 else 0 if r % 5 == 0 else int(rng.integers(0, 9))
        c = rng.integers(0, n_cols - 300000, k)
        rows.append(np.unique(np.where(c >= 100000, c + 300000, c)))   # nothing in [100000, 400000)
    rp, ci, va = _csr_from_rows(rows, n_cols, 7)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout=kind))
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 6)


def test_devbuild_cband_row_span(sm):
    """cband, 16384 rows with about one term per 300 rows inside one window: the chunks are
    opened by the 1024-row span of a chunk, not by its fill."""
    n_rows, n_cols = 16384, 9000
    rng = np.random.default_rng(13)
    has = rng.integers(0, 300, n_rows) == 0
    rows = [rng.integers(0, 7000, 1) if h else np.zeros(0, np.int64) for h in has]
    rp, ci, va = _csr_from_rows(rows, n_cols, 8)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout="cband", band_slabs=1))
    assert info["has_xband"] == 5 and info["xband_bands"] == 1, info
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 7)


@pytest.mark.parametrize("distinct", [255, 256])
def test_devbuild_cband_codebook_edges(sm, distinct):
    """Exactly 255 distinct values take codebook words, 256 take 8-byte entries under
    layout="cband": the same choice and bytes on both paths."""
    n_rows, n_cols, per_row = 5000, 9000, 6
    rp, ci, _ = _uniform(n_rows, n_cols, per_row)
    rng = np.random.default_rng(distinct)
    table = (np.arange(distinct) * 0.375 - 40.0).astype(np.float32)
    va = table[rng.integers(0, distinct, ci.size)]
    va[:distinct] = table   # every value present
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout="cband"))
    assert info["has_xband"] == (5 if distinct == 255 else 4), info
    assert (D.layout_digest()[3] != 0) == (distinct == 255)
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 8)


@pytest.mark.parametrize("kind", ["band2", "cband"])
def test_devbuild_band2_slab0_permille(sm, kind):
    """A narrower slab 0 (band_slab0_permille = 900) with 4 slabs."""
    n_rows, n_cols, per_row = 40000, 20000, 3
    rp, ci, va = _uniform(n_rows, n_cols, per_row)
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, dict(layout=kind, band_slabs=4, band_slab0_permille=900))
    assert info["xband_slab0_cols"] < info["xband_slab_cols"], info
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 9)


@pytest.mark.parametrize("case", ["swapped", "repeated", "sparse_bands"])
def test_devbuild_band2_declines(sm, case):
    """What band2_build or the 70 % rule declines, the device path declines: a row with two
    swapped columns, a row with a repeated column (forced cband), and a layout="bands" matrix
    whose dma3 and wide bands would be under 70 % full.  Both paths report the same layout, none
    says the device built bands, and the digests are equal."""
    if case == "sparse_bands":
        n_rows, n_cols = 20000, 600000
        rp, ci, va = _uniform(n_rows, n_cols, 4)
        opts = dict(layout="bands")
    else:
        n_rows, n_cols = 5000, 9000
        rp, ci, va = _uniform(n_rows, n_cols, 6)
        ci = ci.copy()
        if case == "swapped":
            ci[[3003, 3004]] = ci[[3004, 3003]]
        else:
            ci[3004] = ci[3003]
        opts = dict(layout="cband")
    D, H, info, _, _ = _both(sm, rp, ci, va, n_cols, opts, built=False)
    assert info["has_xband"] not in (4, 5), info
    _spmv_check(D, H, info, rp, ci, va, n_rows, n_cols, 10, oracle_check=False)


def test_devbuild_band2_transpose(sm):
    """transposed() of a 40000 x 20000 cband matrix goes through the same builder: the same
    layout bytes and SpMV bits for host_build 0 and 1."""
    torch = torch_dev()
    n_rows, n_cols = 40000, 20000
    rp, ci, va = _uniform(n_rows, n_cols, 3)
    M = sm.SparseMatrix.from_csr(*(torch.from_numpy(a).cuda() for a in (rp, ci, va)), n_cols,
                                 opts=dict(layout="cband"))
    T = [M.transposed(opts=dict(layout="cband", host_build=hb)) for hb in (0, 1)]
    assert T[0].info()["has_xband"] == 5, T[0].info()
    assert T[0].layout_digest() == T[1].layout_digest() and T[0].layout_digest()[2] != 0
    assert {k: T[0].info()[k] for k in KEYS} == {k: T[1].info()[k] for k in KEYS}
    assert T[0].built_on_device() & BANDS == BANDS and T[1].built_on_device() & BANDS == 0
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n_rows).astype(np.float32)).cuda()
    y0 = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, n_cols).astype(np.float32)).cuda()
    ys = [y0.clone(), y0.clone()]
    for t, y in zip(T, ys):
        t.spmv(x, y, 1.3, 0.5)
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))


@pytest.mark.parametrize("values", ["codebook", "fp32"])
def test_devbuild_band2_config2_full_size(sm, values):
    """BASELINE config 2 as bench.py builds it (2^20 x 2^20, 16 per row, codebook values: AUTO
    takes cband), and the same pattern with arbitrary fp32 values (band2): the device build is
    byte-identical to the host build; the build times of both paths are printed."""
    import sparsematrix_amd.synth as synth
    torch = torch_dev()
    n = 1 << 20
    rp, ci, va = synth.uniform_rows_device(n, n, 16, seed=5)
    if values == "fp32":
        va = torch.rand(va.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)) * 2 - 1
    D, H, info, td, th = _both(sm, rp, ci, va, n, {})
    assert info["has_xband"] == (5 if values == "codebook" else 4), info
    print(f"config 2 ({values}): device build {td:.3f} s, host build {th:.3f} s")
    _spmv_check(D, H, info, rp, ci, va, n, n, 11, oracle_check=False)
