"""The bytes of the balanced-band builder (sparsematrix_amd/csrc/band2.cpp), no GPU:
tests/native/band2_pin.cpp is compiled with AddressSanitizer and run, and its per-case FNV-1a
digests of the layout are compared with tests/golden/band2_pin_c84adfc.json, recorded from the
builder as of commit c84adfc -- before its placement heuristics moved into band2_place.h, the
header the device builder (builddev_band2.hip) shares.  The GPU suite then compares the device
builder with this host builder byte for byte (tests/test_gpu_devbuild_band2.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "band2_pin_c84adfc.json")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_band2_builder_bytes_are_pinned(tmp_path):
    exe = tmp_path / "band2_pin"
    src = [os.path.join(ROOT, "tests", "native", "band2_pin.cpp"),
           os.path.join(ROOT, "sparsematrix_amd", "csrc", "band2.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sparsematrix_amd", "csrc"),
                    *src, "-o", str(exe), "-pthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
    # the fixture covers both encodings, both geometries, and the declined inputs
    assert any(v["codebook"] and v["built"] for v in want.values())
    assert any(not v["codebook"] and v["built"] for v in want.values())
    assert [k for k, v in want.items() if not v["built"]] == ["swapped/dma3", "repeated/dma3"]


def test_built_on_device_rejects_null_arguments():
    """sm_built_on_device without a GPU: the argument checks."""
    from sparsematrix_amd import _lib
    lib = _lib.load()
    mask = C.c_uint32(77)
    assert lib.sm_built_on_device(None, C.byref(mask)) == _lib.SM_ERR_INVALID_ARG
    assert mask.value == 77
