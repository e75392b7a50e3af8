"""Host logic of the codebook forms built from given ids (sm_build_opts.table_updatable;
band2.cpp, sell.cpp, ccsell.cpp, sweep.cpp), no GPU: tests/native/table_asan.cpp is compiled with
AddressSanitizer and run as its own process.  Per builder: the words hold exactly the given ids
(two ids whose table entries are equal stay apart), and the layouts built with the same ids from
two tables are the same bytes -- a new table changes the table alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_given_ids_under_asan(tmp_path):
    exe = tmp_path / "table_asan"
    csrc = os.path.join(ROOT, "sparsematrix_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "table_asan.cpp")] + [
        os.path.join(csrc, f) for f in ("band2.cpp", "sell.cpp", "ccsell.cpp", "sweep.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-I", csrc, *src, "-o", str(exe), "-pthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "table_asan: ok" in r.stdout
