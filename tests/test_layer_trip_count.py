"""Ratchet on what ONE TRIP of the layer loop issues in the headline kernel lnsfaid_decode4_kernel<2, true, false>: the per-degree
layer block (as test_layer_step_count.py counts it, at the values this tree reaches) and everything the loop issues around it -
register-vector reads and writes, degree dispatch, table loads, the patch of the old arg-min nodes, the prefetch take-over
(at two waves per SIMD the launch time follows the NUMBER of issued instructions).  tools/isa_layer_trip.py defines
the walk; the *_BEFORE figures are the same script's output for the tree before the trip was gone through.  Cross-compiles
lnsfaid_kernel4.hip to gfx950 assembly like test_kernel_isa.py.  No GPU needed."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# degree: (VALU, LDS, s_waitcnt of the block; instructions of every kind around it), now and before
NOW = {23: (842, 58, 16, 95), 22: (812, 56, 15, 93)}
BEFORE = {23: (866, 58, 17, 104), 22: (835, 56, 15, 102)}
# s_set_gpr_idx_on per trip: one for the six reads, one for the six writes (before: one per write)
GPR_IDX_ON, GPR_IDX_ON_BEFORE = 2, 6


@pytest.fixture(scope="module")
def trips(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_trip") / "kernel4.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4.hip")], check=True, capture_output=True)
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(ROOT, "tools", "isa_layer_trip.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.measure(out.read_text())


@pytest.mark.parametrize("deg", [23, 22])
def test_layer_trip_issues_no_more_than_it_did(trips, deg):
    assert sorted(trips) == [22, 23], sorted(trips)
    t = trips[deg]
    valu, lds, waitcnt, around = NOW[deg]
    print("degree %d trip: block %d VALU, %d LDS, %d s_waitcnt, %d in all; around it %d (%s); before: %s"
          % (deg, t["block"]["valu"], t["block"]["lds"], t["block"]["waitcnt"], t["block"]["all"], t["around"]["all"], t["around"], BEFORE[deg]))
    assert valu < BEFORE[deg][0] and around <= BEFORE[deg][3] and waitcnt <= BEFORE[deg][2]
    assert t["block"]["valu"] <= valu, t
    assert t["block"]["lds"] <= lds, t
    assert t["block"]["waitcnt"] <= waitcnt, t
    assert t["block"]["vmem"] == 0, t
    assert t["around"]["all"] <= around, t
    assert t["around"]["vmem"] <= 1, t  # the one-dword prefetch of the next layer's edge table
    assert t["gpr_idx_on"] <= GPR_IDX_ON < GPR_IDX_ON_BEFORE, t
