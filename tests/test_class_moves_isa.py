"""Build-time ratchet of the issue-class moves in the window-free kernel, on lnsfaid_decode4w_kernel<2>: per
straight-line layer of the middle form - classified by tools/isa_issue_classes.py - the single v_lshlrev_b32 and the full-rate
opcodes that read an SGPR or VCC are at most what this tree leaves, and the VALU instructions are not above what the tree before
issued in that layer; the first form likewise; 256 VGPRs or fewer and no scratch.  The numbers are read off the compiled kernel.
Cross-compiles lnsfaid_kernel4w.hip to gfx950 assembly.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# what this tree leaves per layer, either form: the shift by 3 that packs c1 into the record; the record's sign bit (AND with 0x40 in
# every byte, merged into a v_bitop3_b32) and, in the layer of degree 22 (layer 1), its valid mask 0x3f, for which SwK holds no register
SHL_B32 = [1] * 12
FULL_RATE_WITH_SGPR = [1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
# before: 15 single left shifts (13 in layer 1, 14 in layer 11) and 7 such SGPR readers in every layer of the middle form
SHL_B32_BEFORE = [15, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14]
# VALU instructions per layer in the tree before this change, and what this tree issues
VALU_BEFORE = {"middle": [832, 676, 832, 820, 808, 836, 824, 770, 735, 796, 832, 799],
               "first": [734, 581, 734, 722, 710, 738, 726, 672, 637, 698, 733, 701]}
VALU = {"middle": [826, 670, 826, 814, 802, 830, 818, 764, 729, 790, 826, 794],
        "first": [729, 576, 729, 717, 705, 733, 721, 667, 632, 693, 728, 697]}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_issue_classes", os.path.join(ROOT, "tools", "isa_issue_classes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_class_moves") / "kernel4w.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4w.hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.mark.parametrize("form", ["middle", "first"])
def test_slow_class_ratchet(asm, tool, form):
    rows = [tool.measure(asm, form, layer) for layer in range(12)]
    shl = [r["shl_b32"] for r in rows]
    sgpr = [r["full_rate_with_sgpr"] for r in rows]
    valu = [r["valu"] for r in rows]
    print("%s form: single v_lshlrev_b32 %s, full-rate opcodes with an SGPR source %s, VALU %s = %d" % (form, shl, sgpr, valu, sum(valu)))
    assert all(g <= w for g, w in zip(shl, SHL_B32)), shl
    assert all(g <= w for g, w in zip(sgpr, FULL_RATE_WITH_SGPR)), sgpr
    assert all(g <= w for g, w in zip(valu, VALU[form])), valu
    assert all(w <= b for w, b in zip(VALU[form], VALU_BEFORE[form]))  # not above the parent's, layer for layer
    assert all(w < b for w, b in zip(SHL_B32, SHL_B32_BEFORE))


def test_the_multiply_is_the_compilers_own(asm, tool):
    """the mask expander's single shifts are v_mul_u32_u24 by a register (no literal, no SGPR), and nothing became a v_mad_u32_u24 or a
    32-bit multiply on the way"""
    for form in ("middle", "first"):
        for layer in (0, 1, 11):
            lines = [ins for ins, _ in tool.layer_lines(asm, form, layer)]
            muls = [i for i in lines if i.startswith("v_mul_u32_u24")]
            assert muls and all(re.match(r"v_mul_u32_u24_e32 v\d+, v\d+, v\d+$", i) for i in muls), muls
            assert not [i for i in lines if i.startswith(("v_mad_u32_u24", "v_mul_lo_u32"))]


def test_registers_and_scratch(asm):
    notes = asm[re.search(r"^_Z\w*%s\w*:" % "lnsfaid_decode4w_kernelILi2EE", asm, flags=re.M).end():]
    vgprs = int(re.search(r"; NumVgprs: (\d+)", notes).group(1))
    print("lnsfaid_decode4w_kernel<2>: %d VGPRs" % vgprs)
    assert vgprs <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", notes).group(1)) == 0
    assert all(int(x) == 0 for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm))
    assert all(int(x) <= 256 for x in re.findall(r"\.vgpr_count:\s*(\d+)", asm))
