"""Build times of config 2's balanced bands, device builder (builddev_band2.hip) against host
builder (band2.cpp), and of the gathered chunk bands forced on the same input (builddev_gcb.hip
against gcb.cpp), for from_csr on device tensors and for transposed(): the figures of
profiles/band_devbuild.txt.  Usage: python tools/band_devbuild_bench.py"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsematrix_amd as sm
import sparsematrix_amd.synth as synth

sm.load()
n = 1 << 20


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M = fn()
    torch.cuda.synchronize()
    return M, time.perf_counter() - t0


def stats(v):
    return f"median {statistics.median(v):.4f} s  min {min(v):.4f}  max {max(v):.4f}  (n = {len(v)})"


say("device:", torch.cuda.get_device_name(0))
say("config 2: 2^20 x 2^20, 16 per row (synth.uniform_rows_device, seed 5); wall clock of the call between")
say("device synchronisations; host_build 0 and 1 alternate in one process; 1 untimed warm-up pair first")
CASES = (("cband (255-value codebook, AUTO)", {}), ("band2 (uniform fp32 values, AUTO)", {}),
         ("gcb (255-value codebook, layout gcb)", dict(layout="gcb")))
for enc, lay in CASES:
    rp, ci, va = synth.uniform_rows_device(n, n, 16, seed=5)
    if enc.startswith("band2"):
        va = torch.rand(va.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)) * 2 - 1
    t = {0: [], 1: []}
    tt = {0: [], 1: []}
    keep = None
    for rep in range(6):
        for hb in (0, 1):
            M, dt = timed(lambda: sm.SparseMatrix.from_csr(rp, ci, va, n, opts=dict(lay, host_build=hb)))
            if rep:
                t[hb].append(dt)
            else:
                say(f"  {enc}: host_build={hb} has_xband={M.info()['has_xband']} bands={M.info()['xband_bands']} "                    f"built_on_device={M.built_on_device()} digest={M.layout_digest()}")
            if hb == 0:
                keep = M
    for rep in range(6):
        for hb in (0, 1):
            T, dt = timed(lambda: keep.transposed(opts=dict(lay, host_build=hb)))
            if rep:
                tt[hb].append(dt)
            else:
                say(f"  {enc}: transposed host_build={hb} has_xband={T.info()['has_xband']} "
                    f"built_on_device={T.built_on_device()} digest={T.layout_digest()}")
            del T
    say(f"{enc}")
    say(f"  from_csr   device builder: {stats(t[0])}")
    say(f"  from_csr   host builder:   {stats(t[1])}")
    say(f"  transposed device builder: {stats(tt[0])}")
    say(f"  transposed host builder:   {stats(tt[1])}")
    del keep
