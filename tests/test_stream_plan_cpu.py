"""The stream kernel's planner and the restated CSR orders, no GPU.

plan_rows (sparsematrix_amd/csrc/plan.cpp) runs as a stand-alone program under AddressSanitizer
and UBSan (tests/native/plan_rows.cpp) and its printout is held against stream_ref.plan -- the
plan the -m gpu tests of tests/test_gpu_stream_tiles.py expect sm_info to report.  The restated
orders themselves (stream_ref.stream_spmv / vector_spmv) are checked against what does not depend
on them: oracle.csr_spmv on the serial rows, 1e-6 * sum|terms| of the float64 value on all rows,
and -- so that a GPU test that passes means something -- that the orders they pin differ in bits
from the serial order, from each other between tile sizes, and between neighbouring lane widths."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import stream_ref as sr
from gpu_util import assert_terms_close, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ((1.3, 0.7), (0.5, 0.0), (1.0, 1.0))


# ---------------------------------------------------------------------------- the planner program
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("plan_rows")
    exe = d / "plan_rows"
    src = [os.path.join(ROOT, "tests", "native", "plan_rows.cpp"),
           os.path.join(ROOT, "sparsematrix_amd", "csrc", "plan.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "sparsematrix_amd", "csrc"), *src, "-o", str(exe)], check=True)
    count = [0]

    def run(rp, tile_nnz, tile_rows=sr.TILE_ROWS, chunk=sr.CHUNK, serial=sr.SERIAL):
        count[0] += 1
        path = d / f"rp{count[0]}.bin"
        np.ascontiguousarray(rp, np.int32).tofile(path)
        r = subprocess.run([str(exe), str(path), str(tile_nnz), str(tile_rows), str(chunk), str(serial)],
                           capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0 and r.stdout.endswith("plan_rows: ok\n"), r.stdout[-2000:] + r.stderr
        tiles, chunks, longs, ptrs, tail = [], [], [], [], {}
        for line in r.stdout.splitlines()[:-1]:
            kind, *v = line.split()
            if kind == "tile":
                tiles.append(tuple(int(a) for a in v))
            elif kind == "chunk":
                chunks.append(tuple(int(a) for a in v))
            elif kind == "long":
                longs.append(int(v[0]))
                ptrs.append((int(v[1]), int(v[2])))
            else:
                tail[kind] = v[0]
        # long_ptr: long row i owns the chunks [first, end) that name it, in order
        for i, (a, e) in enumerate(ptrs):
            assert [c[0] for c in chunks[a:e]] == [i] * (e - a) and e > a
            assert a == (ptrs[i - 1][1] if i else 0)
        assert (ptrs[-1][1] if ptrs else 0) == len(chunks)
        n = len(rp) - 1
        assert float(tail["avg_row_nnz"]) == (int(rp[-1]) / n if n else 0.0)
        return sr.Plan(tiles, chunks, longs, int(tail["max_row_nnz"]))

    return run


def _check_plan(planner, rp, tile_nnz, **kw):
    got, want = planner(rp, tile_nnz, **kw), sr.plan(rp, tile_nnz, **kw)
    assert got == want, (tile_nnz, kw)
    # what any plan must satisfy, whoever computed it
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    cap, rows, serial = tile_nnz, kw.get("tile_rows", sr.TILE_ROWS), kw.get("serial", sr.SERIAL)
    owner = np.zeros(lens.size, np.int64)
    for r0, r1, flags in got.tiles:
        assert 0 < r1 - r0 <= rows and rp[r1] - rp[r0] <= cap
        assert flags == int((lens[r0:r1] > serial).any())
        owner[r0:r1] += 1
    owner[got.long_rows] += 1
    assert (owner == 1).all() and (lens[got.long_rows] > cap).all() and (np.delete(lens, got.long_rows) <= cap).all()
    assert got.max_row_nnz == int(lens.max(initial=0))
    return got


@pytest.mark.parametrize("T", sr.TILES)
def test_planner_on_the_edge_matrices(planner, T):
    """edges(T) under all four tile sizes."""
    seen = set()
    for tile in sr.TILES:
        p = _check_plan(planner, sr.edges(T).rp, tile)
        seen.add((len(p.tiles), len(p.long_rows)))
    assert len(seen) == len(sr.TILES)       # the four plans differ in (tiles, long rows)


def test_planner_on_the_vector_auto_and_exact_matrices(planner):
    cases = [c for c, _ in sr.vector_cases().values()] + [c for c, _ in sr.auto_cases().values()]
    cases += list(sr.exact_cases())
    for c in cases:
        for tile in sr.TILES:
            _check_plan(planner, c.rp, tile)


def test_planner_degenerate_and_random(planner):
    """n = 0, all rows empty, one row, one long row only, 1025 empty rows; a dozen seeded mixes
    of lengths, also with small caps so that every branch turns up often."""
    z = lambda *lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    for rp in (z(), z(0, 0, 0), z(5), z(0), z(1025), z(1024), z(*([0] * 1025)), z(*([0] * 1024)),
               z(0, 1025, 0), z(4097), z(8193)):
        for tile in sr.TILES:
            _check_plan(planner, rp, tile)
    assert sr.plan(z(1025), 1024) == sr.Plan([], [(0, 0, 1025)], [0], 1025)
    assert sr.plan(z(*([0] * 1025)), 1024) == sr.Plan([(0, 1024, 0), (1024, 1025, 0)], [], [], 0)
    assert sr.plan(z(), 1024) == sr.Plan([], [], [], 0)
    for seed in range(12):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(1, 3000))
        lens = rng.choice([0, 0, 1, 2, 7, 63, 64, 65, 200, 1023, 1024, 1025, 2049, 4096, 4097, 9000], n,
                          p=[.2, .2, .2, .1, .1, .04, .04, .04, .03, .01, .01, .01, .005, .005, .005, .005])
        for tile in sr.TILES:
            _check_plan(planner, z(*lens), tile)
        _check_plan(planner, z(*lens), 64, tile_rows=3, chunk=100, serial=2)


# ---------------------------------------------------------------------------- the restated orders
def _serial_differs(got, want, rows, what):
    d = bits(got)[rows] != bits(want)[rows]
    assert d.any(), f"{what}: no row of {np.flatnonzero(rows).tolist()} differs from the serial order"


@pytest.mark.parametrize("T", sr.TILES)
def test_stream_order_on_the_edge_matrices(T):
    """stream_spmv at T on edges(T): the serial rows are the oracle's bits, every row is within the
    bound, an in-tile row above 64 terms and a long row differ from the serial order, and every
    other tile size gives another plan or other bits."""
    c = sr.edges(T)
    p = sr.plan(c.rp, T)
    long_rows = np.zeros(c.n_rows, bool)
    long_rows[p.long_rows] = True
    wave = (c.lens > sr.SERIAL) & ~long_rows
    assert wave.sum() >= 6 and long_rows.sum() == 3
    for alpha, beta in SCALARS:
        want, absum = c.ref(alpha, beta)
        f64, _ = oracle.csr_spmv_f64(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta)
        got = sr.stream_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, T)
        assert_terms_close(got, f64, absum)
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[(c.lens <= sr.SERIAL) & ok], bits(want)[(c.lens <= sr.SERIAL) & ok])
        _serial_differs(got, want, wave & ok, f"T {T} in-tile rows")
        _serial_differs(got, want, long_rows & ok, f"T {T} long rows")
        for other in sr.TILES:
            if other == T:
                continue
            q = sr.plan(c.rp, other)
            alt = sr.stream_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, other)
            assert_terms_close(alt, f64, absum)
            assert (len(q.tiles), len(q.long_rows)) != (len(p.tiles), len(p.long_rows)) or \
                (bits(alt)[ok] != bits(got)[ok]).any(), (T, other)
            # a row that is long under one size and in a tile under the other changes its bits
            moved = (c.lens > min(T, other)) & (c.lens <= max(T, other)) & ok
            assert moved.any() and (bits(alt)[moved] != bits(got)[moved]).any(), (T, other)


def test_stream_order_on_the_auto_and_exact_matrices():
    """The tile_nnz = 0 matrices: auto_tile takes 4096 at longest == 64 x mean and 2048 one term
    past it, and the 2048 and 4096 plans and bits of each differ.  The EXACT matrices: with no
    row above 64 terms the restated stream order is the oracle's on every row at every tile."""
    auto = sr.auto_cases()
    assert [t for _, t in auto.values()] == [4096, 2048, 2048]
    for name, (c, tile) in auto.items():
        p, q = sr.plan(c.rp, 2048), sr.plan(c.rp, 4096)
        assert (len(p.tiles), len(p.long_rows)) != (len(q.tiles), len(q.long_rows)), name
        for alpha, beta in SCALARS:
            f64, absum = oracle.csr_spmv_f64(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta)
            a, b = (sr.stream_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, t) for t in (2048, 4096))
            assert_terms_close(a, f64, absum)
            assert_terms_close(b, f64, absum)
            ok = ~np.isnan(f64)
            assert (bits(a)[ok] != bits(b)[ok]).any(), name
    at64, at65 = sr.exact_cases()
    assert at64.lens.max() == 64 and at65.lens.max() == 65 and at64.n_rows == at65.n_rows == 300
    for alpha, beta in SCALARS:
        want, _ = at64.ref(alpha, beta)
        ok = ~np.isnan(want)
        for T in sr.TILES:
            got = sr.stream_spmv(at64.rp, at64.ci, at64.va, at64.x, at64.y_in(beta), alpha, beta, T)
            assert np.array_equal(bits(got)[ok], bits(want)[ok])


@pytest.mark.parametrize("name", [n for n, _, _ in sr._vector_shapes()])
def test_vector_order(name):
    """vector_spmv at the case's L: within the bound, the rows of 0 and 1 terms as the arithmetic
    says, and L/2 and 2L give other bits than L on at least one row."""
    c, L = sr.vector_cases()[name]
    assert L == sr.vector_lanes(c.n_rows, int(c.rp[-1]))
    differs = {L // 2: 0, 2 * L: 0}     # outputs, over the three scalar pairs, that tell the width apart
    for alpha, beta in SCALARS:
        f64, absum = oracle.csr_spmv_f64(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta)
        want, _ = c.ref(alpha, beta)
        ok = ~np.isnan(want)
        got = sr.vector_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, L)
        assert_terms_close(got, f64, absum)
        # one term: fl(beta y) + (0 + t) is the serial order's bits; no term: -0.0 + +0.0 = +0.0
        one = (c.lens == 1) & ok
        assert one.any() and np.array_equal(bits(got)[one], bits(want)[one])
        none = (c.lens == 0) & ok
        assert none.any() and (bits(got)[none] == 0).all() and (bits(want)[none] == 0x80000000).all()
        for other in (L // 2, 2 * L):
            alt = sr.vector_spmv(c.rp, c.ci, c.va, c.x, c.y_in(beta), alpha, beta, other)
            assert_terms_close(alt, f64, absum)
            differs[other] += int((bits(alt)[ok] != bits(got)[ok]).sum())
    # only rows of more than 2 min(L, other) terms can differ (up to there the two orders coincide)
    assert all(differs.values()), (name, L, differs)


def test_vector_lanes_thresholds():
    assert [sr.vector_lanes(64, 64 * m) for m in (0, 1, 2, 4, 8, 16, 32, 40, 64, 1000)] == \
        [2, 2, 2, 4, 8, 16, 32, 64, 64, 64]
    assert [sr.vector_lanes(64, 64 * m + 1) for m in (2, 4, 8, 16, 32)] == [4, 8, 16, 32, 64]
    assert sr.vector_lanes(0, 0) == 2
