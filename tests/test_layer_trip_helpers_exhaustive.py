"""The statements of csrc/lnsfaid_swar.h that were rewritten to shorten the layer trip, each against the statement it replaced over
its WHOLE input domain: the LDS address of the new arg-min node (one v_perm_b32 instead of mask / shift / merge), the byte gather
and scatter around the two arg-min patches, the arg-min edge's v_perm selector, the index-bit masks taken from the decode words,
and the error-floor table picked on the table words.  tests/layer_trip_helpers_exhaustive.cpp is the host program; no GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")


def test_layer_trip_rewrites_equal_the_statements_they_replace(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "layer_trip_helpers_exhaustive"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "layer_trip_helpers_exhaustive.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "total mismatches: 0", lines[-1]
    for name in ("node_addr", "gather4 / scatter4", "selector", "index masks", "table pick"):
        assert any(l.startswith(name + ":") and l.endswith(" 0 mismatches") for l in lines), (name, lines)
