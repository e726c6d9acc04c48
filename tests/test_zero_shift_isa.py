"""Build-time properties of the rotation-free decode kernel (lnsfaid_kernel4z.hip), on the headline instance
lnsfaid_decode4z_kernel<2>: what the one-wave kernels hold (no scratch, no spills, two waves per SIMD, no vector memory in a layer
block) and a ratchet on what every (degree, ZG) instance of the layer step and the trip around it issue.  Cross-compiles the file
to gfx950 assembly like test_layer_trip_count.py and walks it with tools/isa_layer_trip.py.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lnsfaid_decode4z_kernelILi2EE"

# (degree, ZG): (VALU, instructions of every kind) of the layer block - what this tree reaches, and what a scratch build that
# forced "the first 4 ZG edges are rotation-free" onto lnsfaid_kernel4.hip reached (ZG 0: that file as it is); a block is told
# from the others by its rotates, one after the read and one in front of the write-back per rotating edge
NOW = {(23, 0): (841, 919), (23, 1): (821, 899), (23, 2): (801, 879), (23, 4): (761, 839), (22, 0): (811, 889), (22, 5): (711, 788)}
SCRATCH = {(23, 0): (842, 928), (23, 1): (821, 908), (23, 2): (801, 888), (23, 4): (764, 850), (22, 0): (812, 892), (22, 5): (711, 794)}
# Instructions of every kind around the block per trip of the layer loop.  lnsfaid_kernel4.hip issues 95 on its degree-23 way
# (tests/test_layer_trip_count.py).  Here the (23, 0) way, first in the chain and 6 of the 12 layers of the 50G-PON code, issues
# 90: 5 FEWER (by class: 3 VALU, 1 SALU and 3 branches fewer, 2 scalar loads more - the block itself issues no scalar load here,
# the parent's two are counted inside its block).  Every later way pays for the bit tests in front of it, about 3.5 each.
AROUND = {(23, 0): 90, (23, 1): 94, (23, 2): 100, (23, 4): 104, (22, 5): 106, (22, 0): 113}
PARENT_AROUND_DEG23 = 95


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa4z") / "kernel4z.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4z.hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def trips(asm):
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(ROOT, "tools", "isa_layer_trip.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ps = tool.pieces(tool.kernel_body(asm, HEADLINE))
    big = sorted(range(len(ps)), key=lambda i: -tool.classes(ps[i]["ins"])["valu"])[:len(NOW)]
    out = {}
    for b in big:
        block = tool.classes(ps[b]["ins"])
        key = [k for k in NOW if 2 * (k[0] - 4 * k[1]) == block["rotates"]]
        assert len(key) == 1 and key[0] not in out, (block, sorted(out))
        ins = [x for i in tool.trip(ps, b) for x in ps[i]["ins"]]
        out[key[0]] = {"block": block, "around": tool.classes(ins)}
    return out


def test_no_scratch_no_spills_two_waves_per_simd(asm):
    names = re.findall(r"\.name:\s+(_Z23lnsfaid_decode4z_kernelILi\dEEv12LfKernelArgs)\s", asm)
    assert len(set(names)) == 5, names  # DecodeMethods 1..5
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    assert sizes and all(s == 0 for s in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", asm))
    vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    assert vgprs and max(vgprs) <= 256, vgprs
    assert not re.findall(r"^\s*scratch_", asm, flags=re.M)


@pytest.mark.parametrize("deg,zg", sorted(NOW))
def test_layer_block_and_the_trip_around_it(trips, deg, zg):
    assert sorted(trips) == sorted(NOW), sorted(trips)
    t = trips[(deg, zg)]
    valu, every = NOW[(deg, zg)]
    print("(%d, %d): block %d VALU, %d in all (scratch build %s); around it %d (%s)"
          % (deg, zg, t["block"]["valu"], t["block"]["all"], SCRATCH[(deg, zg)], t["around"]["all"], t["around"]))
    assert valu <= SCRATCH[(deg, zg)][0] and every <= SCRATCH[(deg, zg)][1]
    assert t["block"]["valu"] <= valu, t
    assert t["block"]["all"] <= every, t
    assert t["block"]["vmem"] == 0, t
    assert t["around"]["all"] <= AROUND[(deg, zg)], t
    assert t["around"]["vmem"] <= 1, t  # the one-dword prefetch of the next layer's edge table
    assert AROUND[(23, 0)] <= PARENT_AROUND_DEG23


def test_an_iteration_of_the_50gpon_code_issues_fewer_instructions_than_on_the_rotating_kernel(trips):
    """12 layers: 6 x (23, 0), 3 x (23, 1), (23, 2), (23, 4), (22, 5), against 11 x (928 + 95) + (892 + 93) = 12 238"""
    ways = [(23, 0)] * 6 + [(23, 1)] * 3 + [(23, 2), (23, 4), (22, 5)]
    total = sum(trips[w]["block"]["all"] + trips[w]["around"]["all"] for w in ways)
    print("issued per layered iteration: %d (rotating kernel: 12238)" % total)
    assert total <= 11849
