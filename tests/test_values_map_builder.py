"""Host logic of the slot -> term maps the layout builders emit for updatable matrices
(sm_build_opts.updatable; band2.cpp, xband.cpp, sell.cpp, ccsell.cpp, gcb.cpp), no GPU:
tests/native/valmap_asan.cpp is compiled with AddressSanitizer and run as its own process.
Per builder: every term in exactly one slot, slot bits = val[map[slot]], -1 slots hold the
padding, and writing val2[map[s]] into the layout built from val1 gives, byte for byte, the
layout built from val2; the map is empty when not asked for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_value_maps_under_asan(tmp_path):
    exe = tmp_path / "valmap_asan"
    csrc = os.path.join(ROOT, "sparsematrix_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "valmap_asan.cpp")] + [
        os.path.join(csrc, f) for f in ("band2.cpp", "xband.cpp", "sell.cpp", "ccsell.cpp", "gcb.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-I", csrc, *src, "-o", str(exe), "-pthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "valmap_asan: ok" in r.stdout
