"""Timings of the dense entrance and exit (SparseMatrix.from_dense / dense_device) on a 16384 x
16384 fp32 weight matrix uniform in (-1, 1) on the device, so that keep = E / 16 gives config 2's
16.8 M terms.

  build   from_dense(keep = E / 16), from_dense(per_row = n / 16) and from_dense(threshold = 15 / 16),
          each end to end with layout "no_bands" (the device builders make the layouts, so the
          constructor's tail weighs least), against the composition in torch it replaces: abs, a
          sort (global) or topk (per row) for the cut, a compare, to_sparse_csr, two int64 ->
          int32 casts, from_csr.  Wall clock around a device synchronise, ms, the two routes
          alternating in one run.  The kept counts of both routes are recorded: the torch route
          keeps every element that ties with the cut.
  dense   dense_device(out=buf) against torch.sparse_csr_tensor(...).to_dense() of the same terms
          (us per call between device events, windows alternating) and against the host route
          CopyTo (wall clock, ms, once: a GiB comes down).
  ref     prune_mask(keep = E / 16) of the full matrix held as a CSR (from_dense(threshold = 0):
          every element a stored term): kernels_prune.hip's select streams the same 4 E bytes, the
          yardstick for the dense select's kernels in the trace.

Medians of `--builds` runs (wall clock) and of `--windows` windows of `--reps` eager calls (device
events), after a warm-up.  The kernel trace is a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/dense_bench.py --builds 1 --windows 2 --reps 3

    python tools/dense_bench.py [--out profiles/dense_bench.txt]
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
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--parts", nargs="+", default=["build", "dense", "ref"],
                    choices=["build", "dense", "ref"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    if not torch.cuda.is_available():
        raise SystemExit("tools/dense_bench.py needs an MI355X: no timing without one")
    smd.load()
    n = args.n
    E = n * n
    gen = torch.Generator(device="cuda").manual_seed(53)
    W = torch.rand((n, n), generator=gen, device="cuda") * 2 - 1
    k, k_row, thr = E // 16, n // 16, 15.0 / 16.0
    nb = {"layout": "no_bands"}
    lines = ["# python tools/dense_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n} fp32 uniform in (-1, 1), E {E}, keep {k} / {k_row} per row / threshold {thr}; layout "
             f"no_bands; wall clock: ms, median [min, max] of {args.builds} alternating runs; device figures: us, median "
             f"[min, max] of {args.windows} windows of {args.reps} eager calls between device events)"]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def from_mask(keep):
        s = (W * keep).to_sparse_csr()
        return smd.SparseMatrix.from_csr(s.crow_indices().to(torch.int32), s.col_indices().to(torch.int32), s.values(),
                                         n, opts=nb)

    def torch_global():
        a = W.abs()
        cut = torch.sort(a.reshape(-1), descending=True).values[k - 1]
        return from_mask(a >= cut)

    def torch_row():
        a = W.abs()
        idx = torch.topk(a, k_row, dim=1, sorted=False).indices
        return from_mask(torch.zeros_like(a, dtype=torch.bool).scatter_(1, idx, True))

    def torch_threshold():
        return from_mask(W.abs() >= thr)

    def pair_ms(ours, theirs):
        """Wall-clock ms of the two routes, alternating; (median, [min, max]) each and the last results."""
        t = ([], [])
        res = [None, None]
        for _ in range(args.builds + 1):                 # the first pair warms up
            for i, fn in enumerate((ours, theirs)):
                res[i] = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[i] = fn()
                torch.cuda.synchronize()
                t[i].append((time.perf_counter() - t0) * 1e3)
        stat = lambda v: (round(float(np.median(v[1:])), 2), [round(min(v[1:]), 2), round(max(v[1:]), 2)])
        return stat(t[0]), stat(t[1]), res

    if "build" in args.parts:
        for name, ours, theirs in (("keep", lambda: smd.SparseMatrix.from_dense(W, keep=k, opts=nb), torch_global),
                                   ("per_row", lambda: smd.SparseMatrix.from_dense(W, per_row=k_row, opts=nb), torch_row),
                                   ("threshold", lambda: smd.SparseMatrix.from_dense(W, threshold=thr, opts=nb),
                                    torch_threshold)):
            (a, ar), (b, br), (M, T) = pair_ms(ours, theirs)
            emit({"part": "build", "selector": name, "from_dense_ms": a, "from_dense_min_max": ar, "torch_route_ms": b,
                  "torch_route_min_max": br, "torch_over_from_dense": round(b / a, 2), "nnz": M.nnz, "torch_nnz": T.nnz,
                  "equal": bool(M == T), "built_on_device": M.built_on_device(), "torch_built_on_device": T.built_on_device()})
            M.Destroy()
            T.Destroy()
            torch.cuda.empty_cache()

    if "dense" in args.parts:
        M = smd.SparseMatrix.from_dense(W, keep=k, opts=nb)
        rp, ci, va = M.csr_device()
        crow, col = rp.long(), ci.long()
        buf = torch.empty((n, n), device="cuda")
        ours = lambda: M.dense_device(out=buf)
        theirs = lambda: torch.sparse_csr_tensor(crow, col, va, size=(n, n)).to_dense()
        (a, ar), (b, br) = alternate(torch, [ours, theirs], args.reps, args.windows)
        same = bool(torch.equal(ours().view(torch.int32), theirs().view(torch.int32)))
        t_host, h = wall_ms(torch, lambda: M.CopyTo(None, n, 1), 1)
        emit({"part": "dense", "nnz": M.nnz, "dense_device_us": a, "dense_device_min_max": ar,
              "out_GBps": round(E * 4 / a / 1e3, 1), "torch_to_dense_us": b, "torch_to_dense_min_max": br,
              "torch_over_dense_device": round(b / a, 2), "same_bits": same, "host_copyto_ms": t_host,
              "host_same_bits": bool(np.array_equal(h[:E].view(np.uint32), buf.cpu().numpy().reshape(-1).view(np.uint32)))})

    if "ref" in args.parts:
        # The yardstick for the trace: the full matrix as a CSR (every element a stored term), so
        # that prune_mask's kernels stream the same 4 E bytes from the matrix's own value array.
        F = smd.SparseMatrix.from_dense(W, threshold=0.0, opts=nb)
        (a, ar), = alternate(torch, [lambda: F.prune_mask(keep=k)], max(2, args.reps // 2), args.windows)
        same = bool(torch.equal(F.prune_mask(keep=k).view(n, n).nonzero()[:, 1].to(torch.int32),
                                smd.SparseMatrix.from_dense(W, keep=k, opts=nb).csr_device()[1]))
        emit({"part": "ref", "full_nnz": F.nnz, "prune_mask_us": a, "prune_mask_min_max": ar,
              "same_columns_as_from_dense": same})
        F.Destroy()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
