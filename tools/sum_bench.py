"""Timings of the sum of two matrices on the device (SparseMatrix.sum) on config 2's shape
(2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth) with fp32 values uniform in (-1, 1).

Operand pairs:
  independent  A + an independent B of the same density: almost no overlap;
  subset       A + A.pruned(keep = nnz / 2): B's pattern is a subset of A's;
  regrow       A.sum(G, 1, 0), G a candidate matrix of nnz / 16 terms (one per row, as
               from_dense(|grad|, keep = nnz / 16) would hand over): the regrow step.

  sum      sum() end to end (wall clock, ms) with default options and with layout "no_bands" (where
           the device builders make the layouts and the constructor's tail weighs least), against
           the torch route on the same device: csr_device() of both operands, two sparse COO
           tensors, their sum, coalesce, to CSR, casts to int32, from_csr on device tensors.  That
           route yields no source maps and has no stated rounding rule.
  kernels  a few no_bands sums of every pair and nothing else: run it under
           `rocprofv3 --kernel-trace --stats` for the kernels' own time (profiles/sum_kernel_stats.txt).
           Byte floor of the five kernels together: 8 (nnzA + nnzB) read, 16 nnzC + 4 n_rows written.

Wall-clock figures are medians of `--builds` runs after one warm-up run.

    python tools/sum_bench.py [--out profiles/sum_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.quantize_bench import wall_ms  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--per-row", type=int, default=16)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--parts", nargs="+", default=["sum"], choices=["sum", "kernels"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/sum_bench.py needs an MI355X: no timing without one")
    smd.load()
    n, per = 1 << args.log2_rows, args.per_row
    gen = torch.Generator(device="cuda").manual_seed(53)

    def matrix(per_row, seed):
        rp, ci, _ = synth.uniform_rows_device(n, n, per_row, seed=seed)
        val = torch.rand(int(ci.numel()), generator=gen, device="cuda") * 2 - 1
        return smd.SparseMatrix.from_csr(rp, ci, val, n, opts={"layout": "no_bands"})

    A = matrix(per, 2)
    nnz = A.nnz
    pairs = {"independent": (matrix(per, 3), 1.0, 1.0),
             "subset": (A.pruned(keep=nnz // 2, opts={"layout": "no_bands"}), 1.0, 1.0),
             "regrow": (matrix(max(per // 16, 1), 4), 1.0, 0.0)}
    lines = ["# python tools/sum_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {per} per row, nnz {nnz}; wall clock: ms, median of {args.builds} after a warm-up run; "
             "byte floor of the five kernels: 8 (nnzA + nnzB) read + 16 nnzC + 4 n_rows written)"]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    rows = torch.arange(n, device="cuda")

    def coo(M, coef):
        rp, ci, va = M.csr_device()
        r = torch.repeat_interleave(rows, (rp[1:] - rp[:-1]).long())
        return torch.sparse_coo_tensor(torch.stack([r, ci.long()]), va * coef, (n, n))

    def torch_route(B, alpha, beta, opts):
        c = (coo(A, alpha) + coo(B, beta)).coalesce().to_sparse_csr()
        return smd.SparseMatrix.from_csr(c.crow_indices().to(torch.int32), c.col_indices().to(torch.int32),
                                         c.values(), n, opts=opts)

    nb = {"layout": "no_bands"}
    for name, (B, alpha, beta) in pairs.items():
        if "kernels" in args.parts:
            for _ in range(args.builds):
                A.sum(B, alpha, beta, opts=nb).Destroy()
            torch.cuda.synchronize()
        if "sum" not in args.parts:
            continue
        rec = {"part": "sum", "pair": name, "alpha": alpha, "beta": beta, "nnz_a": nnz, "nnz_b": B.nnz}
        for tag, opts in (("", None), ("no_bands_", nb)):
            A.sum(B, alpha, beta, opts=opts).Destroy()                       # warm-up
            t_dev, Cm = wall_ms(torch, lambda: A.sum(B, alpha, beta, opts=opts), args.builds)
            ci_ = Cm.info()
            rec.update({tag + "device_ms": t_dev, tag + "has_xband": ci_["has_xband"],
                        tag + "built_on_device": Cm.built_on_device()})
            if not tag:
                nnz_c = ci_["nnz"]
                floor = 8 * (nnz + B.nnz) + 16 * nnz_c + 4 * n
                rec.update(nnz_c=nnz_c, floor_bytes=floor, floor_us_at_6_tb_s=round(floor / 6.0e6, 1),
                           device_bytes=ci_["device_bytes"])
            try:
                torch_route(B, alpha, beta, opts).Destroy()                  # warm-up
                t_torch, Tm = wall_ms(torch, lambda: torch_route(B, alpha, beta, opts), args.builds)
                rec.update({tag + "torch_route_ms": t_torch, tag + "torch_over_device": round(t_torch / t_dev, 2),
                            tag + "torch_nnz": Tm.nnz})
                Tm.Destroy()
            except RuntimeError as e:                                        # the route itself failing is a finding
                rec[tag + "torch_route_error"] = str(e).splitlines()[0][:200]
            Cm.Destroy()
        emit(rec)

    if "sum" in args.parts:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
