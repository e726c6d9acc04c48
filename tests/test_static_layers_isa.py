"""Build-time properties of the layer-static decode kernel (lnsfaid_kernel4s.hip), on the headline instance
lnsfaid_decode4s_kernel<2>: what the one-wave kernels hold (no scratch, no spills, two waves per SIMD), its code size, and a ratchet
on what one layered iteration issues - the twelve straight-line layers between the kernel's own comment lines in the assembly,
classified by tools/isa_layer_trip.py - against the 11 849 of the rotation-free kernel's layer loop (tests/test_zero_shift_isa.py).
Cross-compiles the file to gfx950 assembly.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lnsfaid_decode4s_kernelILi2EE"

LOOP_KERNEL_ITERATION = 11849  # lnsfaid_kernel4z.hip: 12 trips of its layer loop, block and everything around it
# what this tree reaches: instructions of every kind per layer on the way an iteration after the first takes outside the
# error-floor window (the patch of the old arg-min nodes counted, the rows' syndrome bits not), and their split over the iteration
PER_LAYER = [972, 781, 950, 936, 921, 955, 941, 878, 840, 907, 949, 911]
ITERATION = {"all": 10941, "valu": 9961, "lds": 716, "other": 264}
ROTATES = 2 * (275 - 69)  # one after the read, one in front of the write-back, on the edges that are no identity circulants
CODE_BYTES = 125040  # the whole kernel; the rotation-free kernel has 101 160
VGPRS = 229


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa4s") / "kernel4s.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4s.hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(ROOT, "tools", "isa_layer_trip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _layers(body):
    """instructions issued per layer between the kernel's begin / end comment lines.  The code is straight-line but for forward
    branches over two blocks per layer: the rows' syndrome bits (wanted inside the error-floor window only: skipped) and the patch
    of the old arg-min nodes (skipped by the first iteration only: walked; it is the block with byte writes to LDS)."""
    lines = body[body.index("; lf4s layers begin"):body.index("; lf4s layers end")].split("\n")
    per, layer, skip = {}, None, None
    for n, raw in enumerate(lines):
        m = re.search(r";\s*lf4s layer (\d+)", raw)
        if m:
            layer = int(m.group(1))
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", raw)
        if m:
            if skip == m.group(1):
                skip = None
            continue
        ins = raw.split(";")[0].strip()
        if skip or not re.match(r"^[a-z]", ins):
            continue
        assert not ins.startswith(("s_branch", "s_endpgm", "s_setpc")), ins
        per.setdefault(layer, []).append(ins)
        if ins.startswith("s_cbranch"):
            target = ins.split()[1]
            end = [k for k in range(n + 1, len(lines)) if lines[k].startswith(target + ":")]
            assert len(end) == 1, ins  # forward, inside the iteration
            if not any("ds_write_b8" in x for x in lines[n + 1:end[0]]):
                skip = target
    return per


@pytest.fixture(scope="module")
def layers(asm, tool):
    per = _layers(tool.kernel_body(asm, HEADLINE))
    assert sorted(per) == list(range(12)), sorted(per, key=str)
    return [tool.classes(per[br]) for br in range(12)]


def test_no_scratch_no_spills_two_waves_per_simd(asm):
    names = re.findall(r"\.name:\s+(_Z23lnsfaid_decode4s_kernelILi\dEEv12LfKernelArgs)\s", asm)
    assert len(set(names)) == 5, names  # DecodeMethods 1..5
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    assert sizes and all(s == 0 for s in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", asm))
    vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    assert vgprs and max(vgprs) <= 256, vgprs
    assert not re.findall(r"^\s*scratch_", asm, flags=re.M)
    assert all(int(x) == 0 for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm))  # En is addressed from LDS offset 0


def test_headline_registers_and_code_size(asm):
    notes = asm[re.search(r"^_Z\w*%s\w*:" % HEADLINE, asm, flags=re.M).end():]  # the compiler's notes follow the kernel's text
    size = int(re.search(r"; codeLenInByte = (\d+)", notes).group(1))
    vgprs = int(re.search(r"; NumVgprs: (\d+)", notes).group(1))
    print("lnsfaid_decode4s_kernel<2>: %d bytes of code, %d VGPRs" % (size, vgprs))
    assert size <= CODE_BYTES and vgprs <= VGPRS
    assert int(re.search(r"; ScratchSize: (\d+)", notes).group(1)) == 0


def test_a_layer_knows_which_layer_it_is(layers, asm, tool):
    """no indexed register moves, no dispatch, no table loads: one vector load (the next layer's arg-min table) per layer, scalar
    loads only where the iteration's parameters arrive (layer 0), and rotates on the edges with a shift only"""
    body = tool.kernel_body(asm, HEADLINE)
    hot = body[body.index("; lf4s layers begin"):body.index("; lf4s layers end")]
    assert "s_set_gpr_idx" not in hot and "v_movrel" not in hot
    assert "s_load_dwordx16" not in hot and "s_load_dwordx8" not in hot
    assert all(c["vmem"] <= 1 for c in layers) and layers[11]["vmem"] == 0, [c["vmem"] for c in layers]
    assert all(c["smem"] == 0 for c in layers[1:]), [c["smem"] for c in layers]
    assert sum(c["rotates"] for c in layers) == ROTATES
    assert layers[1]["rotates"] == 0  # 22 identity circulants


def test_an_iteration_issues_fewer_instructions_than_the_layer_loop(layers):
    total = {k: sum(c[k] for c in layers) for k in ("all", "valu", "lds")}
    total["other"] = total["all"] - total["valu"] - total["lds"]
    print("issued per layered iteration: %s (layer loop of lnsfaid_kernel4z.hip: %d); per layer %s"
          % (total, LOOP_KERNEL_ITERATION, [c["all"] for c in layers]))
    assert ITERATION["all"] < LOOP_KERNEL_ITERATION and sum(PER_LAYER) == ITERATION["all"]
    assert total["all"] <= ITERATION["all"], total
    assert total["valu"] <= ITERATION["valu"] and total["lds"] <= ITERATION["lds"] and total["other"] <= ITERATION["other"], total
    assert all(c["all"] <= want for c, want in zip(layers, PER_LAYER)), [c["all"] for c in layers]
