"""Timings of the table-matrix calls (SparseMatrix.from_csr_ids) on config 2's / config 3's shape
(2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth), ids uniform over a 255-entry table.

  grad     sddmm_table(G, X) at N = 32 on a matrix without SpMV layouts (config 3 as
           tools/sddmm_bench.py builds it), against what a caller could do before on the same
           build: sddmm into an nnz-sized array, then torch index_add_ by id into a zeroed
           T-vector.  us per call; the two results are compared.
  update   axpy_table on config 2 built with table_updatable = 1 (AUTO -> cband), us per call,
           against the rebuild through from_csr_ids from host arrays (wall clock, ms).
  spmv     the point of table_updatable: SpMV (AUTO) of that cband matrix against the same
           pattern built with updatable = 1 (AUTO -> band2), alternating windows in one run.
  --ab-nobin   (a -DSM_DEV build of the library through SM_LIB_PATH, tools/build_dev.sh): the
           fused gradient kernel with and without its per-id scan (SM_TABLE_NOBIN=1: the dots
           still go to LDS, no thread scans), alternating windows -- the cost of the binning.

Every figure is the median over `--windows` windows of `--reps` eager calls between two device
events, after a warm-up window.

    python tools/table_bench.py [--out profiles/table_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CSR_ONLY = {"layout": "no_bands", "sell": 0, "relabel": 0}


def window_us(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(torch, fns, reps, windows):
    """Median us per call of each fn, their windows alternating (after one warm-up window each)."""
    for fn in fns:
        window_us(torch, fn, max(2, reps // 4))
    t = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            t[i].append(window_us(torch, fn, reps))
    return [(round(float(np.median(v)), 2), [round(min(v), 2), round(max(v), 2)]) for v in t]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--per-row", type=int, default=16)
    ap.add_argument("--n-rhs", type=int, default=32)
    ap.add_argument("--table-size", type=int, default=255)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rebuilds", type=int, default=2)
    ap.add_argument("--parts", nargs="+", default=["grad", "update", "spmv"], choices=["grad", "update", "spmv"])
    ap.add_argument("--ab-nobin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/table_bench.py needs an MI355X: no timing without one")
    smd.load()
    n, N, T = 1 << args.log2_rows, args.n_rhs, args.table_size
    rp_d, ci_d, _ = synth.uniform_rows_device(n, n, args.per_row, seed=2)
    rp, ci = rp_d.cpu().numpy(), ci_d.cpu().numpy()
    nnz = int(ci.size)
    rng = np.random.default_rng(45)
    ids = rng.integers(0, T, nnz).astype(np.uint8)
    table = rng.uniform(-1, 1, T).astype(np.float32)
    gen = torch.Generator(device="cuda").manual_seed(46)
    G = torch.rand(n, N, generator=gen, device="cuda") * 2 - 1
    X = torch.rand(n, N, generator=gen, device="cuda") * 2 - 1
    lines = ["# python tools/table_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {args.per_row} per row, nnz {nnz}, T {T}; us per call: median [min, max] of "
             f"{args.windows} windows of {args.reps} eager calls between device events)"]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if args.ab_nobin or "grad" in args.parts:
        M = smd.SparseMatrix.from_csr_ids(rp, ci, ids, table, n, opts=CSR_ONLY)
        out = torch.zeros(T, device="cuda")
        fused = lambda: M.sddmm_table(G, X, out=out, alpha=1.0, beta=0.0)
        if args.ab_nobin:
            if not os.environ.get("SM_LIB_PATH"):
                raise SystemExit("--ab-nobin needs SM_LIB_PATH = a -DSM_DEV build (tools/build_dev.sh)")

            def nobin():
                os.environ["SM_TABLE_NOBIN"] = "1"
                try:
                    fused()
                finally:
                    os.environ["SM_TABLE_NOBIN"] = "0"
            (a, ar), (b, br) = alternate(torch, [fused, nobin], args.reps, args.windows)
            emit({"part": "binning A/B (dev build)", "n_rhs": N, "fused_us": a, "fused_min_max": ar,
                  "without_scan_us": b, "without_scan_min_max": br, "scan_us": round(a - b, 2)})
        else:
            buf = torch.zeros(nnz, device="cuda")
            acc = torch.zeros(T, device="cuda")
            idx = torch.from_numpy(ids.astype(np.int64)).cuda()

            def two_pass():
                M.sddmm(G, X, out=buf, alpha=1.0, beta=0.0)
                acc.zero_()
                acc.index_add_(0, idx, buf)
            sddmm_only = lambda: M.sddmm(G, X, out=buf, alpha=1.0, beta=0.0)
            (a, ar), (b, br), (c, cr) = alternate(torch, [fused, two_pass, sddmm_only], args.reps, args.windows)
            fused()
            two_pass()
            torch.cuda.synchronize()
            scale = float(acc.abs().max())
            emit({"part": "grad", "n_rhs": N, "sddmm_table_us": a, "sddmm_table_min_max": ar,
                  "sddmm_plus_index_add_us": b, "sddmm_plus_index_add_min_max": br,
                  "sddmm_alone_us": c, "sddmm_alone_min_max": cr,
                  "max_abs_diff_over_max_abs": float((out - acc).abs().max()) / scale})
        M.Destroy()

    if not args.ab_nobin and ("update" in args.parts or "spmv" in args.parts):
        opts = {"table_updatable": 1}
        Mt = smd.SparseMatrix.from_csr_ids(rp, ci, ids, table, n, opts=opts)
        info = Mt.info()
        if "update" in args.parts:
            delta = torch.rand(T, generator=gen, device="cuda") * 2 - 1
            ((u, ur),) = alternate(torch, [lambda: Mt.axpy_table(-1e-3, delta)], args.reps, args.windows)
            new_table = Mt.table_device().cpu().numpy()
            t_re, same = [], True
            for _ in range(args.rebuilds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F = smd.SparseMatrix.from_csr_ids(rp, ci, ids, new_table, n, opts=opts)
                torch.cuda.synchronize()
                t_re.append((time.perf_counter() - t0) * 1e3)
                same = same and bool(Mt == F) and Mt.layout_digest() == F.layout_digest()
                F.Destroy()
            emit({"part": "update", "has_xband": info["has_xband"], "device_bytes": info["device_bytes"],
                  "axpy_table_us": u, "axpy_table_min_max": ur, "alg_bytes": 5 * nnz,
                  "alg_gbs": round(5 * nnz / u / 1e3, 1), "rebuild_ms": round(float(np.median(t_re)), 1),
                  "rebuild_over_update": round(float(np.median(t_re)) * 1e3 / u, 1), "update_equals_rebuild": same})
        if "spmv" in args.parts:
            val = Mt.csr_device()[2]   # the values the table matrix holds now (after the update part)
            Mu = smd.SparseMatrix.from_csr(rp_d, ci_d, val, n, opts={"updatable": 1})
            iu = Mu.info()
            x = torch.rand(n, generator=gen, device="cuda") * 2 - 1
            y1, y2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
            (a, ar), (b, br) = alternate(torch, [lambda: Mt.spmv(x, y1, 1.0, 0.0), lambda: Mu.spmv(x, y2, 1.0, 0.0)],
                                         4 * args.reps, args.windows)
            torch.cuda.synchronize()
            emit({"part": "spmv", "table_updatable_has_xband": info["has_xband"], "table_updatable_us": a,
                  "table_updatable_min_max": ar, "table_updatable_device_bytes": info["device_bytes"],
                  "updatable_has_xband": iu["has_xband"], "updatable_us": b, "updatable_min_max": br,
                  "updatable_device_bytes": iu["device_bytes"],
                  "max_abs_diff": float((y1 - y2).abs().max())})
            Mu.Destroy()
        Mt.Destroy()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.ab_nobin else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
