"""Timing of sm_sddmm against sm_spmm on the same matrix, and the torch expression it replaces.

Config 3's shape (2^20 x 2^20, 16 terms per row, sparsematrix_amd.synth) at N = 32, 1 and 128.
Per N, in one process and on one matrix:

  sddmm   out = G (.) X over the pattern, SM_ALGO_AUTO, alpha = 1, beta = 0
  spmm    Y = B X, SM_ALGO_AUTO, alpha = 1, beta = 0 -- the yardstick: it gathers the same X rows and
          writes Y where SDDMM reads G; SDDMM adds 4 bytes per term (8 with the read that beta costs)
  torch   (G[rows] * X[cols]).sum(1), eager, where its two nnz x N temporaries fit

sddmm and spmm: `--calls` calls captured serially into one graph (torch.cuda.graph) over
`--replicas` operand sets used in turn, so no call finds its operands left in cache by the call
before; after warm-up replays the time of one call is a replay's device time / calls, and the
figure is the median over `--replays` replays, the two graphs replayed alternately.

    python tools/sddmm_bench.py [--out profiles/sddmm_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alg_bytes(n_rows, n_cols, nnz, N):
    """Bytes each algorithm must move at least once (compulsory traffic; X counted once)."""
    csr = 4 * (n_rows + 1) + 4 * nnz
    dense = 4 * N * (n_rows + n_cols)
    return {"sddmm": csr + dense + 8 * nnz,              # col, G, X, out read and written
            "spmm": csr + 4 * nnz + dense + 4 * N * n_rows}   # col, val, X, Y read and written


def graph_of(torch, fn, calls):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
    return g


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
    ap.add_argument("--n", type=int, nargs="+", default=[32, 1, 128])
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--replicas", type=int, default=4)
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--torch-limit-gib", type=float, default=40.0,
                    help="skip the torch expression when its temporaries exceed this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_bench.txt"))
    args = ap.parse_args()

    import torch

    import sparsematrix_amd as smd
    from sparsematrix_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("tools/sddmm_bench.py needs an MI355X: no timing without one")
    smd.load()
    n = 1 << args.log2_rows
    rp, ci, va = synth.uniform_rows_device(n, n, args.per_row, seed=2)
    M = smd.SparseMatrix.from_csr(rp, ci, va, n, opts={"layout": "no_bands", "sell": 0, "relabel": 0})
    nnz = int(ci.numel())
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), args.per_row)
    cols = ci.long()
    lines = ["# python tools/sddmm_bench.py " + " ".join(sys.argv[1:]) +
             f"   ({n} x {n}, {args.per_row} per row, nnz {nnz}; us per call, median of "
             f"{args.replays} graph replays of {args.calls} calls over {args.replicas} operand sets)"]
    gen = torch.Generator(device="cuda").manual_seed(33)
    for N in args.n:
        R = args.replicas
        shape = (lambda r: (r,)) if N == 1 else (lambda r: (r, N))
        Gs = [torch.rand(shape(n), generator=gen, device="cuda") * 2 - 1 for _ in range(R)]
        Xs = [torch.rand(shape(n), generator=gen, device="cuda") * 2 - 1 for _ in range(R)]
        Ys = [torch.zeros(shape(n), device="cuda") for _ in range(R)]
        outs = [torch.zeros(nnz, device="cuda") for _ in range(R)]
        G2 = [g.view(n, N) for g in Gs]
        X2 = [x.view(n, N) for x in Xs]
        Y2 = [y.view(n, N) for y in Ys]

        def sddmm(i):
            M.sddmm(Gs[i % R], Xs[i % R], outs[i % R], 1.0, 0.0)

        def spmm(i):
            M.spmm(X2[i % R], Y2[i % R], 1.0, 0.0)

        for i in range(R):   # warm-up: every operand set, both kernels
            sddmm(i)
            spmm(i)
        torch.cuda.synchronize()
        # the sampled product against the torch expression, once, on operand set 0
        want = (G2[0][rows[:1 << 16]].double() * X2[0][cols[:1 << 16]].double()).sum(1)
        err = float((outs[0][:1 << 16].double() - want).abs().max())
        g_sd, g_sp = graph_of(torch, sddmm, args.calls), graph_of(torch, spmm, args.calls)
        for _ in range(3):
            replay_ms(torch, g_sd)
            replay_ms(torch, g_sp)
        t_sd, t_sp = [], []
        for _ in range(args.replays):
            t_sd.append(replay_ms(torch, g_sd) * 1e3 / args.calls)
            t_sp.append(replay_ms(torch, g_sp) * 1e3 / args.calls)
        sd, sp = float(np.median(t_sd)), float(np.median(t_sp))
        b = alg_bytes(n, n, nnz, N)
        rec = {"n_rhs": N, "sddmm_us": round(sd, 1), "spmm_us": round(sp, 1), "sddmm_over_spmm": round(sd / sp, 3),
               "sddmm_us_min_max": [round(min(t_sd), 1), round(max(t_sd), 1)],
               "spmm_us_min_max": [round(min(t_sp), 1), round(max(t_sp), 1)],
               "sddmm_alg_bytes": b["sddmm"], "spmm_alg_bytes": b["spmm"],
               "alg_bytes_ratio": round(b["sddmm"] / b["spmm"], 3),
               "sddmm_alg_gbs": round(b["sddmm"] / sd / 1e3, 1), "spmm_alg_gbs": round(b["spmm"] / sp / 1e3, 1),
               "max_abs_err_vs_fp64_first_65536_terms": err}
        tmp_gib = 2.0 * nnz * N * 4 / 2 ** 30
        if tmp_gib <= args.torch_limit_gib:
            def expr():
                return (G2[0][rows] * X2[0][cols]).sum(1)
            for _ in range(2):
                expr()
            torch.cuda.synchronize()
            tt = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                expr()
                e1.record()
                torch.cuda.synchronize()
                tt.append(e0.elapsed_time(e1) * 1e3)
            rec["torch_us"] = round(float(np.median(tt)), 1)
            rec["torch_temporaries_gib"] = round(tmp_gib, 2)
        else:
            rec["torch_us"] = None
            rec["torch_skipped"] = f"temporaries {tmp_gib:.1f} GiB"
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Gs, Xs, Ys, outs, G2, X2, Y2, g_sd, g_sp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
