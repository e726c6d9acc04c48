"""Ratchet on the instruction count of the layer step (at two waves per SIMD the launch time follows the NUMBER
of issued instructions).  Cross-compiles lnsfaid_kernel4.hip to gfx950 assembly like test_kernel_isa.py and counts the two
per-degree instances of the layer step inside the headline kernel lnsfaid_decode4_kernel<2, true, false>.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# VALU instructions of the block: what this tree reaches, and what it was before the layer step was gone through for its count
# (thermometer code -> number by table, one masked magnitude and one range test per edge in pass 2, the minimum search and the
# sign words merged four edges at a time).
VALU_DEG23, VALU_DEG23_BEFORE = 866, 938
VALU_DEG22, VALU_DEG22_BEFORE = 835, 904
# everything else the block issues may not grow either
LDS_DEG23, WAITCNT_DEG23 = 58, 23
LDS_DEG22, WAITCNT_DEG22 = 56, 21


@pytest.fixture(scope="module")
def layer_blocks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_count") / "kernel4.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4.hip")], check=True, capture_output=True)
    parts = re.split(r"^(_Z\w+):", out.read_text(), flags=re.M)
    bodies = [parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if "lnsfaid_decode4_kernelILi2ELb1ELb0E" in parts[i]]
    assert len(bodies) == 1
    blocks = []
    for chunk in re.split(r"^\.LBB\d+_\d+:", bodies[0], flags=re.M):
        ins = [l.split(";")[0].strip() for l in chunk.split("\n")]
        ins = [i for i in ins if re.match(r"^[a-z]", i)]
        blocks.append({"valu": sum(1 for i in ins if i.startswith("v_")), "lds": sum(1 for i in ins if i.startswith("ds_")),
                       "waitcnt": sum(1 for i in ins if i.startswith("s_waitcnt")),
                       "rotates": sum(1 for i in ins if i.startswith("v_alignbyte_b32")),
                       "vmem": sum(1 for i in ins if re.match(r"(global|flat|buffer|scratch)_", i))})
    blocks.sort(key=lambda b: -b["valu"])
    return blocks[:2]


@pytest.mark.parametrize("deg,valu,before,lds,waitcnt", [(23, VALU_DEG23, VALU_DEG23_BEFORE, LDS_DEG23, WAITCNT_DEG23),
                                                          (22, VALU_DEG22, VALU_DEG22_BEFORE, LDS_DEG22, WAITCNT_DEG22)])
def test_layer_block_issues_no_more_than_it_did(layer_blocks, deg, valu, before, lds, waitcnt):
    # one read rotate and one write-back rotate per edge tell the two instances apart
    block = [b for b in layer_blocks if b["rotates"] == 2 * deg]
    assert len(block) == 1, layer_blocks
    b = block[0]
    print("degree %d layer block: %d VALU (before: %d), %d LDS, %d s_waitcnt" % (deg, b["valu"], before, b["lds"], b["waitcnt"]))
    assert valu < before
    assert b["valu"] <= valu, b
    assert b["lds"] <= lds, b
    assert b["waitcnt"] <= waitcnt, b
    assert b["vmem"] == 0, b
