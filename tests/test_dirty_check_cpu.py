"""The decision points' cheap "certainly dirty" test without a GPU: the per-lane row parity of the layer-static
kernel on its compile-time tables (sw50_row_parity, csrc/lnsfaid_static50.h: stage 1 on the layer with the most identity circulants,
stage 2 on layer 0) and of every other kernel on run-time tables (sw_row_parity, csrc/lnsfaid_swar.h) compiled for the host and run
over En images in the LDS layout (tests/dirty_check_emul.cpp) against the parity of the layer's 256 rows computed node by node from
the base matrix: 200 random images, the clean image, every single-node sign flip in a block column the layer has / lacks, the
boundary En = 0 / 1 of the hard decision; the run-time function also against the text it replaced."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("dirty_check") / "dirty_check_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "dirty_check_emul.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    return r


def test_row_parity_equals_the_base_matrix(report):
    out = report.stdout.strip().splitlines()
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-500:]
    assert out[-1] == "total mismatches: 0", out[-1]


def test_every_function_and_layer_was_run(report):
    """stage 1 is layer 1 (22 of 22 edges identities), stage 2 layer 0; the run-time function on a degree-23 and a degree-22 layer;
    a layer that mixes identity and rotating edges through the compile-time function"""
    out = report.stdout.strip().splitlines()
    assert out[0] == "stage 1 layer: 1"
    assert out[1:-1] == ["layer 1, compile-time tables: 0 mismatches", "layer 0, compile-time tables: 0 mismatches",
                         "layer 0, run-time tables: 0 mismatches", "layer 1, run-time tables: 0 mismatches",
                         "layer 7, compile-time tables: 0 mismatches", "layer 7, compile-time tables: 0 mismatches"], out
