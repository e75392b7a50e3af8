"""Timing of the transposed matrix (sm_create_transpose) against the host route it replaces.

For config 2's shape (2^20 x 2^20, 16 per row) and an R-MAT graph (sparsematrix_amd.synth):

  (a) the device transposition alone: transposed() with layout = NO_BANDS, sell = 0,
      relabel = 0, so no layout build is in the figure (the constructor's plan is);
  (b) the host route with the same options: sm_copy_csr, a stable host transposition
      (scipy's csr -> csc counting sort where scipy is installed, else numpy's stable
      argsort), sm_create_from_csr_ex;
  (c) transposed() with default options, and the default-algorithm SpMV of the result
      beside the source's.

Every (case, leg) runs in a child process of its own under `timeout`; the driver stops at the
first child that fails.  One JSON line per leg, then a summary line per case with (b)/(a).

    python tools/transpose_bench.py [--rmat-scale 22] [--reps 3] [--out profiles/transpose_build.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN = {"layout": "no_bands", "sell": 0, "relabel": 0}
LEG_TIMEOUT_S = {"a": 240, "b": 420, "c": 420}


def make_source(case: str, rmat_scale: int):
    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if case == "config2":
        n = 1 << 20
        rp, ci, va = synth.uniform_rows_device(n, n, 16, seed=2)
    else:
        n = 1 << rmat_scale
        rp, ci, va = synth.rmat_device(rmat_scale)
    M = smd.SparseMatrix.from_csr(rp, ci, va, n, opts=PLAIN)
    del rp, ci, va
    torch.cuda.synchronize()
    return M


def host_transpose(rp, ci, va, n_rows, n_cols):
    """(t_rp, t_col, t_val, how): the terms stably sorted by column."""
    try:
        import scipy.sparse as sp
        t = sp.csr_matrix((va, ci, rp), shape=(n_rows, n_cols)).tocsc()   # counting sort, stable
        return (t.indptr.astype(np.int32), t.indices.astype(np.int32), t.data.astype(np.float32),
                "scipy csr->csc")
    except ImportError:
        order = np.argsort(ci, kind="stable")
        rows = np.repeat(np.arange(n_rows, dtype=np.int32), np.diff(rp))
        t_rp = np.zeros(n_cols + 1, np.int64)
        t_rp[1:] = np.cumsum(np.bincount(ci, minlength=n_cols))
        return t_rp.astype(np.int32), rows[order], va[order], "numpy stable argsort"


def spmv_us(M, iters: int = 50) -> float:
    import torch
    x = torch.rand(M.n_cols, device="cuda") * 2 - 1
    y = torch.zeros(M.n_rows, device="cuda")
    for _ in range(5):
        M.spmv(x, y, 1.0, 0.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        M.spmv(x, y, 1.0, 0.0)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def run_leg(case: str, leg: str, rmat_scale: int, reps: int) -> dict:
    import torch

    import sparsematrix_amd as smd
    smd.load()
    M = make_source(case, rmat_scale)
    info = M.info()
    out = {"case": case if case == "config2" else f"rmat{rmat_scale}", "leg": leg,
           "n_rows": info["n_rows"], "n_cols": info["n_cols"], "nnz": info["nnz"]}
    if leg == "a":
        ts = []
        for _ in range(reps + 1):   # the first call also pays hipCUB's kernel loading
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = M.transposed(opts=PLAIN)
            ts.append(time.perf_counter() - t0)
            t.Destroy()
        out.update(first_s=round(ts[0], 4), device_s=round(min(ts[1:]), 4),
                   all_s=[round(v, 4) for v in ts])
    elif leg == "b":
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            rp, ci, va = M.csr()
            t1 = time.perf_counter()
            t_rp, t_ci, t_va, how = host_transpose(rp, ci, va, info["n_rows"], info["n_cols"])
            t2 = time.perf_counter()
            t = smd.SparseMatrix.from_csr(t_rp, t_ci, t_va, info["n_rows"], opts=PLAIN)
            t3 = time.perf_counter()
            t.Destroy()
            cur = dict(host_s=round(t3 - t0, 4), copy_csr_s=round(t1 - t0, 4),
                       host_transpose_s=round(t2 - t1, 4), create_from_csr_s=round(t3 - t2, 4), how=how)
            if best is None or cur["host_s"] < best["host_s"]:
                best = cur
        out.update(best)
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = M.transposed()
        out["default_opts_s"] = round(time.perf_counter() - t0, 4)
        ti = t.info()
        out.update(result_layout={k: ti[k] for k in ("has_xband", "xband_slabs", "sell_slices", "col_relabel")},
                   result_device_bytes=ti["device_bytes"])
        D = make_source_default(M)
        out.update(spmv_source_us=round(spmv_us(D), 2), spmv_transposed_us=round(spmv_us(t), 2))
    return out


def make_source_default(M):
    """The same matrix with the constructors' default layouts (the SpMV yardstick)."""
    import torch

    import sparsematrix_amd as smd
    rp, ci, va = M.csr()
    D = smd.SparseMatrix.from_csr(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(),
                                  torch.from_numpy(va).cuda(), M.n_cols)
    torch.cuda.synchronize()
    return D


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rmat-scale", type=int, default=22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transpose_build.txt"))
    ap.add_argument("--case", choices=("config2", "rmat"))
    ap.add_argument("--leg", choices=("a", "b", "c"))
    args = ap.parse_args()
    if args.leg:   # child: one leg, one JSON line
        print(json.dumps(run_leg(args.case, args.leg, args.rmat_scale, args.reps)), flush=True)
        return
    lines = ["# tools/transpose_bench.py --rmat-scale %d --reps %d  (seconds: wall, best of reps)"
             % (args.rmat_scale, args.reps)]
    ok = True
    for case in ("config2", "rmat"):
        got = {}
        for leg in ("a", "b", "c"):
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__),
                   "--case", case, "--leg", leg, "--rmat-scale", str(args.rmat_scale), "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # a fault, an abort or a time limit: start nothing more on the GPU
                lines.append("# %s leg %s failed with exit status %d" % (case, leg, r.returncode))
                lines.append("# " + (r.stderr or "").strip()[-400:].replace("\n", "\n# "))
                ok = False
                break
            line = r.stdout.strip().splitlines()[-1]
            got[leg] = json.loads(line)
            lines.append(line)
            print(line, flush=True)
        if not ok:
            break
        a, b = got["a"]["device_s"], got["b"]["host_s"]
        lines.append(json.dumps({"case": got["a"]["case"], "summary": True, "device_s": a, "host_s": b,
                                 "host_over_device": round(b / a, 2)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
