"""Timing of an in-place value update (SparseMatrix.axpy_values) against the rebuild it replaces.

Config 2's / config 3's matrix (2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth) with random
fp32 values, built with updatable = 1, in one process per layout:

  auto      config 2 as the SpMV runs it: AUTO -> band2 (8-byte entries; the CSR step and one
            entry refresh)
  no_bands  the sorted sliced ELL (the CSR step and one plain refresh)
  csr       config 3 as tools/sddmm_bench.py builds it for the SpMM / SDDMM kernels: no layout
            holds a copy of the values (the CSR step alone)

  update    m.axpy_values(a, delta): `--calls` calls captured serially into one graph
            (torch.cuda.graph) over `--replicas` delta buffers used in turn; the time of one call
            is a replay's device time / calls, the figure the median over `--replays` replays
  rebuild   SparseMatrix.from_csr(row_ptr, col_idx, new values, n_cols, opts) from device arrays
            with the same options, wall clock with a device synchronisation, median of
            `--rebuilds`: what a step cost before

The update's algorithmic bytes: 12 per term for the CSR step (value read and written, delta read)
plus 12 per value slot of the layout (4 map + 4 gather + 4 store); the slots are counted from the
maps' share of device_bytes (4 bytes per slot: the same build without the option holds none).

    python tools/update_values_bench.py [--out profiles/update_values_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = {
    "auto": {},
    "no_bands": {"layout": "no_bands"},
    "csr": {"layout": "no_bands", "sell": 0, "relabel": 0},
}


def replay_ms(torch, graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--per-row", type=int, default=16)
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS), choices=list(LAYOUTS))
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--replicas", type=int, default=4)
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--rebuilds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_values_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/update_values_bench.py needs an MI355X: no timing without one")
    smd.load()
    n = 1 << args.log2_rows
    rp, ci, _ = synth.uniform_rows_device(n, n, args.per_row, seed=2)
    nnz = int(ci.numel())
    gen = torch.Generator(device="cuda").manual_seed(44)
    va = torch.rand(nnz, generator=gen, device="cuda") * 2 - 1          # arbitrary fp32 values
    deltas = [torch.rand(nnz, generator=gen, device="cuda") * 2 - 1 for _ in range(args.replicas)]
    a = -1e-3
    lines = ["# python tools/update_values_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {args.per_row} per row, nnz {nnz}, random fp32 values, updatable = 1; "
             f"update: us per axpy_values call, median of {args.replays} graph replays of {args.calls} "
             f"calls over {args.replicas} delta buffers; rebuild: ms per from_csr from device arrays, "
             f"median of {args.rebuilds})"]
    for name in args.layouts:
        opts = dict(LAYOUTS[name], updatable=1)
        plain = smd.SparseMatrix.from_csr(rp, ci, va, n, opts=LAYOUTS[name])
        plain_bytes = plain.info()["device_bytes"]
        plain.Destroy()
        M = smd.SparseMatrix.from_csr(rp, ci, va, n, opts=opts)
        info = M.info()
        slots = (info["device_bytes"] - plain_bytes) // 4
        for d in deltas:   # warm-up: every delta buffer
            M.axpy_values(a, d)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(args.calls):
                M.axpy_values(a, deltas[i % args.replicas])
        for _ in range(3):
            replay_ms(torch, graph)
        t_up = [replay_ms(torch, graph) * 1e3 / args.calls for _ in range(args.replays)]
        # the update against a fresh build from the values the matrix now holds
        new_val = M.csr_device()[2]
        t_re = []
        for _ in range(args.rebuilds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F = smd.SparseMatrix.from_csr(rp, ci, new_val, n, opts=opts)
            torch.cuda.synchronize()
            t_re.append((time.perf_counter() - t0) * 1e3)
            same = bool(M == F) and M.layout_digest() == F.layout_digest()
            F.Destroy()
        up, re_ms = float(np.median(t_up)), float(np.median(t_re))
        alg = 12 * nnz + 12 * slots
        rec = {"layout": name, "has_xband": info["has_xband"], "sell_slices": info["sell_slices"],
               "value_slots": int(slots), "map_bytes": int(4 * slots), "device_bytes": info["device_bytes"],
               "update_us": round(up, 1), "update_us_min_max": [round(min(t_up), 1), round(max(t_up), 1)],
               "update_alg_bytes": int(alg), "update_alg_gbs": round(alg / up / 1e3, 1),
               "rebuild_ms": round(re_ms, 1), "rebuild_ms_min_max": [round(min(t_re), 1), round(max(t_re), 1)],
               "rebuild_over_update": round(re_ms * 1e3 / up, 1), "update_equals_rebuild": same}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del graph
        M.Destroy()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
