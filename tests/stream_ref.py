"""The CSR kernels' plan and summation orders, restated in numpy: what SM_ALGO_STREAM and
SM_ALGO_VECTOR (sparsematrix_amd/csrc/kernels.hip) compute bit for bit, the row-tile planner
they run on (csrc/plan.cpp, upload_plan in csrc/layouts.cpp), and the matrices that sit on the
edges of both.  fp32 throughout, every multiplication and addition rounded on its own (the
kernels use __fmul_rn / __fadd_rn and the library is built with -ffp-contract=off).  No GPU and
no torch at import.

The orders (kernels.hip, by kernel):
  term            fl(x[c] * fl(v * alpha));  beta*y: y * beta unless beta == 1.
  spmv_stream     a row of <= 64 terms (SM_SERIAL_ROW_MAX): beta*y, then its terms in stored order.
                  A longer row inside a tile: lane l of a wavefront adds terms l, l + 64, ... from
                  +0.0, the 64 lane sums go through the xor butterfly at distances 32 .. 1, and
                  y = fl(beta*y) + that.  A row of more than tile_nnz terms (a long row) is cut
                  into chunks of 4096 terms; in a chunk [begin, end), thread t of 256 adds the
                  indices (begin & ~3) + 4 t + q + 1024 j (q = 0 .. 3) that lie inside the chunk,
                  ascending, from +0.0; a butterfly per wavefront; waves 0 .. 3 added in order;
                  spmv_long_finalize adds the chunk sums onto beta*y in chunk order.
  spmv_vector     L lanes per row (L = 2 .. 64, the first power of two that is not below the mean
                  row length): lane l adds terms l, l + L, ... from +0.0, a butterfly at distances
                  L/2 .. 1, y = fl(beta*y) + that -- every row, so an empty row's -0.0 becomes +0.0.
"""
import functools
from collections import namedtuple

import numpy as np

from layout_specs import Case

TILES = (1024, 2048, 4096, 8192)        # the spmv_stream_kernel instantiations (launch_spmv_stream)
TILE_ROWS, CHUNK, SERIAL = 1024, 4096, 64   # kTileRows, kLongChunk, SM_SERIAL_ROW_MAX
THREADS, WAVE = 256, 64                 # kStreamThreads, the wavefront
EDGE_COLS = 20011
F32 = np.float32

Plan = namedtuple("Plan", "tiles chunks long_rows max_row_nnz")


# ---------------------------------------------------------------------------- the planner
def plan(rp, tile_nnz, tile_rows=TILE_ROWS, chunk=CHUNK, serial=SERIAL):
    """plan_rows (csrc/plan.cpp): tiles (r0, r1, flags), chunks (long_row, begin, end) and the
    long rows, greedily in row order.  A row of more than tile_nnz terms is a long row (no tile;
    chunks of `chunk` terms); a tile takes rows while it stays within tile_nnz terms and
    tile_rows rows and the next row is not long; flags bit 0: it holds a row above `serial`."""
    rp = [int(v) for v in np.asarray(rp).reshape(-1)]
    n = len(rp) - 1
    tiles, chunks, long_rows = [], [], []
    r = 0
    while r < n:
        if rp[r + 1] - rp[r] > tile_nnz:
            for b in range(rp[r], rp[r + 1], chunk):
                chunks.append((len(long_rows), b, min(rp[r + 1], b + chunk)))
            long_rows.append(r)
            r += 1
            continue
        r0, terms, flags = r, 0, 0
        while r < n and r - r0 < tile_rows:
            ln = rp[r + 1] - rp[r]
            if ln > tile_nnz or terms + ln > tile_nnz:
                break
            terms += ln
            flags |= int(ln > serial)
            r += 1
        tiles.append((r0, r, flags))
    longest = max((rp[i + 1] - rp[i] for i in range(n)), default=0)
    return Plan(tiles, chunks, long_rows, longest)


def auto_tile(rp):
    """upload_plan's choice for tile_nnz = 0 (csrc/layouts.cpp): 4096, or 2048 when the longest
    row is strictly greater than 64 x the mean row length."""
    rp = np.asarray(rp, np.int64).reshape(-1)
    n = rp.size - 1
    if n <= 0:
        return 4096
    return 2048 if float(np.diff(rp).max()) > 64.0 * float(rp[-1]) / float(n) else 4096


# ---------------------------------------------------------------------------- the sums
def _terms(ci, va, x, alpha):
    return np.asarray(x, F32)[np.asarray(ci, np.int64)] * (np.asarray(va, F32) * F32(alpha))


def _beta_y(y0, beta):
    y0 = np.asarray(y0, F32)
    return y0 * F32(beta) if F32(beta) != F32(1.0) else y0.copy()


def _lane_sums(t, lanes):
    """Lane l's sum of t[l], t[l + lanes], ... in that order from +0.0."""
    k = -(-t.size // lanes)
    pad = np.zeros(k * lanes, F32)
    pad[:t.size] = t
    live = (np.arange(k * lanes) < t.size).reshape(k, lanes)
    pad = pad.reshape(k, lanes)
    s = np.zeros(lanes, F32)
    for j in range(k):
        s = np.where(live[j], s + pad[j], s)
    return s


def _butterfly(s):
    """The xor butterfly at distances len/2 .. 1; every lane ends with the same bits."""
    lane = np.arange(s.size)
    off = s.size // 2
    while off:
        s = s + s[lane ^ off]
        off >>= 1
    return s[0]


def _chunk_sum(t, begin, end):
    """One chunk of a long row (spmv_stream_kernel, b < n_chunks)."""
    base = begin & ~3
    tid = np.arange(THREADS)
    s = np.zeros(THREADS, F32)
    j = 0
    while base + 4 * THREADS * j < end:
        for q in range(4):
            idx = base + 4 * THREADS * j + 4 * tid + q
            live = (idx >= begin) & (idx < end)
            s = np.where(live, s + t[np.where(live, idx, begin)], s)
        j += 1
    waves = [_butterfly(s[w * WAVE:(w + 1) * WAVE]) for w in range(THREADS // WAVE)]
    p = waves[0]
    for w in waves[1:]:
        p = p + w
    return p


def stream_spmv(rp, ci, va, x, y0, alpha, beta, tile_nnz):
    """SM_ALGO_STREAM on the plan of `tile_nnz`, bit for bit."""
    rp = np.asarray(rp, np.int64).reshape(-1)
    lens = np.diff(rp)
    t = _terms(ci, va, x, alpha)
    acc = _beta_y(y0, beta)
    out = acc.copy()
    p = plan(rp, tile_nnz)
    in_tile = np.zeros(lens.size, bool)
    for r0, r1, flags in p.tiles:
        in_tile[r0:r1] = True
        for r in range(r0, r1):
            if lens[r] > SERIAL and flags & 1:      # the wave pass runs only on flagged tiles
                out[r] = acc[r] + _butterfly(_lane_sums(t[rp[r]:rp[r + 1]], WAVE))
    serial = in_tile & (lens <= SERIAL)
    for k in range(int(lens[serial].max(initial=0))):
        m = serial & (lens > k)
        out[m] = out[m] + t[rp[:-1][m] + k]
    for i, r in enumerate(p.long_rows):
        a = acc[r]
        for lr, b, e in p.chunks:
            if lr == i:
                a = a + _chunk_sum(t, b, e)
        out[r] = a
    return out


def vector_lanes(n_rows, nnz):
    """launch_spmv_vector's L: 2, doubled while it is below 64 and below the mean row length."""
    avg = nnz / n_rows if n_rows else 0.0
    lanes = 2
    while lanes < 64 and lanes < avg:
        lanes <<= 1
    return lanes


def vector_spmv(rp, ci, va, x, y0, alpha, beta, L):
    """SM_ALGO_VECTOR with L lanes per row (any power of two, 1 included), bit for bit."""
    rp = np.asarray(rp, np.int64).reshape(-1)
    t = _terms(ci, va, x, alpha)
    acc = _beta_y(y0, beta)
    out = acc.copy()
    for r in range(rp.size - 1):
        out[r] = acc[r] + _butterfly(_lane_sums(t[rp[r]:rp[r + 1]], L))
    return out


# ---------------------------------------------------------------------------- the matrices
def _case(lens, n_cols, seed):
    """A Case with the given row lengths: sorted distinct columns, plain fp32 values in (-1, 1)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate([np.sort(rng.choice(n_cols, int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)])
    va = rng.uniform(-1, 1, ci.size).astype(F32)
    return Case(rp, ci, va, n_cols, seed=seed + 1)


def edge_lens(T):
    """The row lengths of edges(T), and the row index of each named situation."""
    lens, at = [], {}

    def add(name, *ls):
        at[name] = len(lens)
        lens.extend(ls)

    add("head", 3)
    add("full_one_row", T)                  # a one-row tile of exactly T terms from index 3
    add("long_unaligned", T + 1)            # a long row whose only chunk starts at 3 + T
    add("row_cap", *([1, 0] * 520))         # 1040 rows of 520 terms: past the 1024-row cap
    add("long_second", T + 1)               # the tile after it starts fresh
    add("full_many_rows", *([64] * (T // 64)))   # a tile filled to exactly T
    add("opens_tile", 1)                    # ... so this term opens the next one
    add("strided", *([1] * 256))
    add("wave_strided", 65)                 # row 257 of its tile: met by the strided loop, wave-summed
    add("serial_edge", 63, 64, 65, 127, 128, 129)
    add("almost_full", T - 1)
    add("two", 2)
    add("empty", 0)
    add("long_last", 2 * T + 1)             # ends the term arrays, off a multiple of 4
    return np.array(lens, np.int64), at


@functools.lru_cache(maxsize=None)
def edges(T):
    """The edge matrix of tile size T (about 1350 rows, 7 T + 1425 terms, 20011 columns), with
    the asserts that every situation it is named for is in its own plan."""
    assert T in TILES
    lens, at = edge_lens(T)
    c = _case(lens, EDGE_COLS, seed=T)
    rp = c.rp.astype(np.int64)
    p = plan(rp, T)
    tile_of = {r: t for t in p.tiles for r in range(t[0], t[1])}
    terms = lambda t: int(rp[t[1]] - rp[t[0]])
    # a one-row tile, full to T, whose first term index is 3 mod 4: the kernel's extra load slot
    t = tile_of[at["full_one_row"]]
    assert t[1] - t[0] == 1 and terms(t) == T and rp[t[0]] % 4 == 3 and t[2] & 1, t
    # long rows: three, the first chunk unaligned, the last one ending the arrays off a multiple of 4
    want_long = [at["long_unaligned"], at["long_second"], at["long_last"]]
    assert p.long_rows == want_long and p.max_row_nnz == 2 * T + 1, p.long_rows
    first = [c_ for c_ in p.chunks if c_[0] == 0]
    assert len(first) == -(-(T + 1) // CHUNK) and first[0][1] == 3 + T and first[-1][2] == 4 + 2 * T
    assert all(b % 4 == 3 for _, b, _ in first), first
    last = [c_ for c_ in p.chunks if c_[0] == 2]
    assert len(last) == -(-(2 * T + 1) // CHUNK) and last[-1][2] == rp[-1] and rp[-1] % 4 != 0, last
    # the 1024-row cap: one tile of exactly 1024 rows, the rest of the run in the next
    t = tile_of[at["row_cap"]]
    assert t == (at["row_cap"], at["row_cap"] + TILE_ROWS, 0) and terms(t) == 512, t
    assert tile_of[at["row_cap"] + TILE_ROWS] == (at["row_cap"] + TILE_ROWS, at["long_second"], 0)
    # a tile of several rows filled to exactly T, and the term after it in a new tile
    t = tile_of[at["full_many_rows"]]
    assert t == (at["full_many_rows"], at["opens_tile"], 0) and terms(t) == T and t[1] - t[0] == T // 64, t
    t = tile_of[at["opens_tile"]]
    assert t[0] == at["opens_tile"] and t[2] & 1, t
    # a wave-summed row beyond the first 256 rows of its tile, and the serial / wave edge
    assert tile_of[at["wave_strided"]] == t and at["wave_strided"] - t[0] == 257 and lens[at["wave_strided"]] == 65
    assert t[1] == at["almost_full"] and lens[at["serial_edge"]:at["almost_full"]].tolist() == [63, 64, 65, 127, 128, 129]
    # T - 1 terms alone in a tile; the last tile holds the 2-term row and the empty row
    t = tile_of[at["almost_full"]]
    assert t[1] - t[0] == 1 and terms(t) == T - 1, t
    assert p.tiles[-1] == (at["two"], at["long_last"], 0)
    assert (c.y0[c.lens == 0].view(np.uint32) == 0x80000000).all() and (c.lens == 0).sum() == 521
    return c


def _fill(fixed, n_rows, nnz):
    """`fixed` followed by rows that bring the matrix to n_rows rows and nnz terms, as even as
    the remainder allows."""
    m, rest = n_rows - len(fixed), nnz - sum(fixed)
    assert m > 0 and rest >= 0, (fixed, n_rows, nnz)
    return list(fixed) + [rest // m + (1 if i < rest % m else 0) for i in range(m)]


VECTOR_COLS = 4099


def _vector_shapes():
    """(name, n_rows, nnz) of the eleven vector cases: the mean row length exactly on each
    threshold of `L < mean` (2 .. 32), one term above it, and mean 40.  64 rows, except where the
    rows every case holds (0, 1, L-1, L, L+1, 2L+1, 300 terms) alone exceed 64 x the mean: 192
    rows at mean 2 and 128 at mean 4."""
    out = []
    for mean in (2, 4, 8, 16, 32):
        n = {2: 192, 4: 128}.get(mean, 64)
        out += [(f"mean{mean}", n, mean * n), (f"mean{mean}+1", n, mean * n + 1)]
    return out + [("mean40", 64, 40 * 64)]


@functools.lru_cache(maxsize=None)
def vector_cases():
    """{name: (Case, L)}, one matrix per lane width and threshold side."""
    cases = {}
    for i, (name, n, nnz) in enumerate(_vector_shapes()):
        L = vector_lanes(n, nnz)
        fixed = [L, 0, 1, L - 1, L + 1, 2 * L + 1, 300]   # row 0 gets y_in's NaN at beta = 0
        # seeds chosen so that, for every case, L/2 and 2L give other bits than L on some row
        # (tests/test_stream_plan_cpu.py asserts it: only the rows above 2 L terms can differ)
        c = _case(_fill(fixed, n, nnz), VECTOR_COLS, seed=600 + 2 * i)
        assert c.n_rows == n and c.rp[-1] == nnz and c.lens[:7].tolist() == fixed
        cases[name] = (c, L)
    widths = [L for _, L in cases.values()]
    assert widths == [2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64], widths
    return cases


@functools.lru_cache(maxsize=None)
def auto_cases():
    """{name: (Case, tile)} for tile_nnz = 0: 100 rows whose longest row is exactly 64 x the mean
    (2560 = 64 x 40: upload_plan keeps 4096), the same with one more term in that row (2048), and
    edges(4096) (its longest row, 8193 terms, is far past 64 x the mean: 2048).  The 2560-term
    row lies inside a tile at 4096 and is a long row at 2048."""
    at, over = _fill([5, 2560], 100, 4000), _fill([5, 2560], 100, 4000)
    over[1] += 1
    cases = {"longest=64mean": _case(at, EDGE_COLS, seed=71), "longest=64mean+1": _case(over, EDGE_COLS, seed=73),
             "edges4096": edges(4096)}
    return {k: (c, auto_tile(c.rp)) for k, c in cases.items()}


@functools.lru_cache(maxsize=None)
def exact_cases():
    """(a 300-row matrix whose longest row has 64 terms, the same with that row at 65): the two
    sides of exact_algo's max_row_nnz <= SM_SERIAL_ROW_MAX."""
    lens = [(7 * r) % 41 for r in range(300)]
    lens[0], lens[150], lens[299] = 0, 64, 40
    at64 = _case(lens, VECTOR_COLS, seed=81)
    lens[150] = 65
    return at64, _case(lens, VECTOR_COLS, seed=81)
