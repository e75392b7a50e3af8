"""Timings of the device quantiser (SparseMatrix.quantize_assign / quantize_update / quantized) on
config 2's shape (2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth) with fp32 values uniform
in (-1, 1), T = 255.

  step       one Lloyd step, quantize_assign + quantize_update (each allocates its scratch and
             synchronises the stream), against the same step composed in torch on the same device:
             torch.bucketize on the sorted table plus the neighbour compare, then index_add_ into
             float64 sums and counts.  us per step; the two tables are compared.  Also a step
             inside quantized() (the same kernels without the calls' allocations and
             synchronises), as (quantized(iters=8) - quantized(iters=0)) / 8.
  quantized  quantized(T, iters=8) end to end (wall clock, ms) against the host route it replaces:
             csr() download, the same loop in numpy (searchsorted + bincount), from_csr_ids.
  spmv       the gain the feature buys: SpMV (AUTO) of the updatable source (band2) and of the
             quantised result (cband), alternating windows in one run.

Device figures are medians over `--windows` windows of `--reps` eager calls between two device
events, after a warm-up window; wall-clock figures medians of `--builds` runs.

    python tools/quantize_bench.py [--out profiles/quantize_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.table_bench import alternate  # noqa: E402


def numpy_lloyd(val, T, iters):
    """The loop of sm_create_quantized in vectorised numpy (float64 sums by bincount)."""
    lo, hi = float(val.min()), float(val.max())
    table = (lo + (hi - lo) * (np.arange(T) / max(T - 1, 1))).astype(np.float32)

    def assign(table):
        order = np.argsort(table, kind="stable")
        st = table[order]
        c = np.searchsorted(st, val, side="right")
        lo_i, hi_i = np.maximum(c - 1, 0), np.minimum(c, T - 1)
        take_hi = (c == 0) | ((st[hi_i] - val) < (val - st[lo_i]))
        return order[np.where(take_hi, hi_i, lo_i)].astype(np.uint8)

    for _ in range(iters):
        ids = assign(table)
        n = np.bincount(ids, minlength=T)
        s = np.bincount(ids, val.astype(np.float64), T)
        table = np.where(n > 0, s / np.maximum(n, 1), table).astype(np.float32)
    return assign(table), table


def wall_ms(torch, fn, runs):
    t = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 2), r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--per-row", type=int, default=16)
    ap.add_argument("--table-size", type=int, default=255)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--parts", nargs="+", default=["step", "quantized", "spmv"], choices=["step", "quantized", "spmv"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/quantize_bench.py needs an MI355X: no timing without one")
    smd.load()
    n, T = 1 << args.log2_rows, args.table_size
    rp_d, ci_d, _ = synth.uniform_rows_device(n, n, args.per_row, seed=2)
    nnz = int(ci_d.numel())
    gen = torch.Generator(device="cuda").manual_seed(47)
    val = torch.rand(nnz, generator=gen, device="cuda") * 2 - 1
    src = smd.SparseMatrix.from_csr(rp_d, ci_d, val, n, opts={"updatable": 1})
    lines = ["# python tools/quantize_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {args.per_row} per row, nnz {nnz}, T {T}; device figures: us, median [min, max] of "
             f"{args.windows} windows of {args.reps} eager calls between device events; wall clock: ms, median of "
             f"{args.builds})"]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if "step" in args.parts:
        table0 = torch.linspace(-1, 1, T, device="cuda")
        tab_a, tab_b = table0.clone(), table0.clone()

        def ours():
            tab_a.copy_(table0)
            src.quantize_update(src.quantize_assign(tab_a), tab_a)

        def composed():
            tab_b.copy_(table0)
            st, order = torch.sort(tab_b)
            c = torch.bucketize(val, st, right=True)
            lo_i, hi_i = (c - 1).clamp_(min=0), c.clamp(max=T - 1)
            take_hi = (c == 0) | ((st[hi_i] - val) < (val - st[lo_i]))
            ids = order[torch.where(take_hi, hi_i, lo_i)]
            s = torch.zeros(T, dtype=torch.float64, device="cuda").index_add_(0, ids, val.double())
            k = torch.zeros(T, dtype=torch.float64, device="cuda").index_add_(0, ids, torch.ones_like(val, dtype=torch.float64))
            tab_b.copy_(torch.where(k > 0, s / k.clamp(min=1), tab_b.double()).float())

        assign_only = lambda: src.quantize_assign(table0)
        ids0 = src.quantize_assign(table0)
        update_only = lambda: (tab_a.copy_(table0), src.quantize_update(ids0, tab_a))
        (a, ar), (b, br), (c_, cr), (d, dr) = alternate(torch, [ours, composed, assign_only, update_only],
                                                         args.reps, args.windows)
        ours()
        composed()
        torch.cuda.synchronize()
        emit({"part": "step", "assign_plus_update_us": a, "assign_plus_update_min_max": ar,
              "torch_composition_us": b, "torch_composition_min_max": br, "assign_us": c_, "assign_min_max": cr,
              "update_us": d, "update_min_max": dr,
              "max_abs_table_diff": float((tab_a - tab_b).abs().max())})

    Q = None
    if "quantized" in args.parts or "spmv" in args.parts:
        t_dev, Q = wall_ms(torch, lambda: src.quantized(table_size=T, iters=args.iters), args.builds)
    if "quantized" in args.parts:
        t_dev0, _ = wall_ms(torch, lambda: src.quantized(table_size=T, iters=0), args.builds)
        stage = {}

        def host_route():
            t0 = time.perf_counter()
            rp, ci, va = src.csr()
            t1 = time.perf_counter()
            ids, table = numpy_lloyd(va, T, args.iters)
            t2 = time.perf_counter()
            H = smd.SparseMatrix.from_csr_ids(rp, ci, ids, table, n)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            stage.update(download_ms=round((t1 - t0) * 1e3, 1), numpy_loop_ms=round((t2 - t1) * 1e3, 1),
                         from_csr_ids_ms=round((t3 - t2) * 1e3, 1))
            return H
        t_host, H = wall_ms(torch, host_route, 1)
        qi, hi = Q.info(), H.info()
        emit({"part": "quantized", "iters": args.iters, "device_ms": t_dev, "device_iters0_ms": t_dev0,
              "step_inside_ms": round((t_dev - t_dev0) / max(args.iters, 1), 3), "host_route_ms": t_host, **stage,
              "host_over_device": round(t_host / t_dev, 1), "has_xband": qi["has_xband"],
              "host_has_xband": hi["has_xband"], "built_on_device": Q.built_on_device(),
              "max_abs_table_diff_vs_numpy": float(np.abs(Q.table_device().cpu().numpy() -
                                                          H.table_device().cpu().numpy()).max())})
        H.Destroy()
    if "spmv" in args.parts:
        x = torch.rand(n, generator=gen, device="cuda") * 2 - 1
        y1, y2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        (a, ar), (b, br) = alternate(torch, [lambda: src.spmv(x, y1, 1.0, 0.0), lambda: Q.spmv(x, y2, 1.0, 0.0)],
                                     10 * args.reps, args.windows)
        torch.cuda.synchronize()
        si, qi = src.info(), Q.info()
        emit({"part": "spmv", "source_has_xband": si["has_xband"], "source_us": a, "source_min_max": ar,
              "source_device_bytes": si["device_bytes"], "quantized_has_xband": qi["has_xband"], "quantized_us": b,
              "quantized_min_max": br, "quantized_device_bytes": qi["device_bytes"],
              "max_abs_diff": float((y1 - y2).abs().max())})

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
