"""Timings of pruning on the device (SparseMatrix.prune_mask / pruned) on config 2's shape
(2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth) with fp32 values uniform in (-1, 1).

  mask    prune_mask(keep = nnz / 2) and prune_mask(per_row = 8) (each allocates its scratch and
          synchronises the stream) against the same selections composed in torch on the same
          device: val.abs(), torch.sort (rocPRIM's radix sort, the one hipCUB wraps) for the cut,
          a compare; per row a topk over the (rows, 16) view and a scatter.  us per call, the
          windows alternating in one run.  The masks are compared: the torch route keeps every
          term that ties with the cut, so it may keep a few more.
  pruned  pruned(keep = nnz / 2) end to end (wall clock, ms) against the two routes it replaces:
          torch on the device (abs, sort, mask, cumsum, three boolean gathers, a row recount,
          from_csr on device tensors) and the host (csr(), np.argpartition, from_csr); the first
          two also with layout "no_bands", where the device builders make the layouts and the
          constructor's tail weighs least.
  spmv    SpMV (AUTO) of the source and of the pruned result, alternating windows.

Device figures are medians over `--windows` windows of `--reps` eager calls between two device
events, after a warm-up window; wall-clock figures medians of `--builds` runs.

    python tools/prune_bench.py [--out profiles/prune_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.quantize_bench import wall_ms  # noqa: E402
from tools.table_bench import alternate  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--per-row", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--parts", nargs="+", default=["mask", "pruned", "spmv"], choices=["mask", "pruned", "spmv"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/prune_bench.py needs an MI355X: no timing without one")
    smd.load()
    n, per = 1 << args.log2_rows, args.per_row
    rp_d, ci_d, _ = synth.uniform_rows_device(n, n, per, seed=2)
    nnz = int(ci_d.numel())
    gen = torch.Generator(device="cuda").manual_seed(47)
    val = torch.rand(nnz, generator=gen, device="cuda") * 2 - 1
    src = smd.SparseMatrix.from_csr(rp_d, ci_d, val, n)
    k, k_row = nnz // 2, per // 2
    lines = ["# python tools/prune_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {per} per row, nnz {nnz}, keep {k} / {k_row} per row; device figures: us, median "
             f"[min, max] of {args.windows} windows of {args.reps} eager calls between device events; wall clock: ms, "
             f"median of {args.builds})"]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def torch_global_mask():
        a = val.abs()
        cut = torch.sort(a, descending=True).values[k - 1]
        return a >= cut

    def torch_row_mask():
        a = val.abs().view(n, per)
        idx = torch.topk(a, k_row, dim=1, sorted=False).indices
        return torch.zeros_like(a, dtype=torch.bool).scatter_(1, idx, True).view(-1)

    if "mask" in args.parts:
        ours_g = lambda: src.prune_mask(keep=k)
        ours_r = lambda: src.prune_mask(per_row=k_row)
        ours_t = lambda: src.prune_mask(threshold=0.5)
        (a, ar), (b, br), (c, cr), (d, dr), (e, er) = alternate(
            torch, [ours_g, torch_global_mask, ours_r, torch_row_mask, ours_t], args.reps, args.windows)
        mg, tg, mr, tr = ours_g().bool(), torch_global_mask(), ours_r().bool(), torch_row_mask()
        torch.cuda.synchronize()
        emit({"part": "mask", "global_us": a, "global_min_max": ar, "torch_global_us": b, "torch_global_min_max": br,
              "torch_over_global": round(b / a, 1), "row_us": c, "row_min_max": cr, "torch_row_us": d,
              "torch_row_min_max": dr, "torch_over_row": round(d / c, 1), "threshold_us": e, "threshold_min_max": er,
              "global_kept": int(mg.sum()), "torch_global_kept": int(tg.sum()),
              "global_dropped_but_kept_by_torch": int((tg & ~mg).sum()), "global_kept_but_dropped_by_torch": int((mg & ~tg).sum()),
              "row_kept": int(mr.sum()), "torch_row_kept": int(tr.sum()),
              "row_magnitudes_differ": int((val.abs().view(n, per) * (mr.view(n, per).float() - tr.view(n, per).float()))
                                           .sum(1).ne(0).sum())})

    P = None
    if "pruned" in args.parts or "spmv" in args.parts:
        t_dev, P = wall_ms(torch, lambda: src.pruned(keep=k), args.builds)
    if "pruned" in args.parts:
        def torch_route(opts=None):
            rp, ci, va = src.csr_device()
            keep = torch_global_mask()
            pos = torch.cumsum(keep, 0, dtype=torch.int32)
            new_rp = torch.cat([pos.new_zeros(1), pos])[rp.long()]
            return smd.SparseMatrix.from_csr(new_rp, ci[keep], va[keep], n, opts=opts)

        stage = {}

        def host_route():
            t0 = time.perf_counter()
            rp, ci, va = src.csr()
            t1 = time.perf_counter()
            keep = np.zeros(nnz, bool)
            keep[np.argpartition(-np.abs(va), k - 1)[:k]] = True
            new_rp = np.concatenate([[0], np.cumsum(keep)])[rp].astype(np.int32)
            t2 = time.perf_counter()
            H = smd.SparseMatrix.from_csr(new_rp, ci[keep], va[keep], n)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            stage.update(download_ms=round((t1 - t0) * 1e3, 1), numpy_select_ms=round((t2 - t1) * 1e3, 1),
                         from_csr_ms=round((t3 - t2) * 1e3, 1))
            return H
        t_torch, Tm = wall_ms(torch, torch_route, args.builds)
        t_host, H = wall_ms(torch, host_route, 1)
        t_masked, _ = wall_ms(torch, lambda: src.masked(src.prune_mask(keep=k)), args.builds)
        # The same two routes where the device builders make the layouts (no band layout asked for):
        # what the selection and the compaction themselves cost beside the constructor's tail.
        nb = {"layout": "no_bands"}
        t_dev_nb, Pn = wall_ms(torch, lambda: src.pruned(keep=k, opts=nb), args.builds)
        t_torch_nb, Tn = wall_ms(torch, lambda: torch_route(nb), args.builds)
        nb_built = Pn.built_on_device()
        Pn.Destroy()
        Tn.Destroy()
        pi, ti, hi = P.info(), Tm.info(), H.info()
        emit({"part": "pruned", "device_ms": t_dev, "mask_then_masked_ms": t_masked, "torch_route_ms": t_torch,
              "torch_over_device": round(t_torch / t_dev, 2), "host_route_ms": t_host, **stage,
              "host_over_device": round(t_host / t_dev, 1), "nnz": pi["nnz"], "torch_nnz": ti["nnz"], "host_nnz": hi["nnz"],
              "has_xband": pi["has_xband"], "torch_has_xband": ti["has_xband"], "host_has_xband": hi["has_xband"],
              "built_on_device": P.built_on_device(), "device_bytes": pi["device_bytes"],
              "no_bands_device_ms": t_dev_nb, "no_bands_torch_route_ms": t_torch_nb,
              "no_bands_torch_over_device": round(t_torch_nb / t_dev_nb, 2), "no_bands_built_on_device": nb_built})
        Tm.Destroy()
        H.Destroy()
    if "spmv" in args.parts:
        x = torch.rand(n, generator=gen, device="cuda") * 2 - 1
        y1, y2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        (a, ar), (b, br) = alternate(torch, [lambda: src.spmv(x, y1, 1.0, 0.0), lambda: P.spmv(x, y2, 1.0, 0.0)],
                                     10 * args.reps, args.windows)
        torch.cuda.synchronize()
        si, pi = src.info(), P.info()
        emit({"part": "spmv", "source_has_xband": si["has_xband"], "source_nnz": si["nnz"], "source_us": a,
              "source_min_max": ar, "source_device_bytes": si["device_bytes"], "pruned_has_xband": pi["has_xband"],
              "pruned_nnz": pi["nnz"], "pruned_us": b, "pruned_min_max": br, "pruned_device_bytes": pi["device_bytes"]})

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
