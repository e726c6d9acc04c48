"""Build-time properties of the window-free kernel's edge-word twin (lnsfaid_kernel4e.hip), on the headline instance
lnsfaid_decode4e_kernel<2>, against lnsfaid_decode4w_kernel<2> compiled in the same test: no scratch, no spills, at most 256 VGPRs,
no static LDS; per layer and form the VALU instructions are at most the window-free kernel's less two per rotating edge (the address
addition and the rotate amount's negation that the table replaces) plus a slack of four; and per layer the vector-memory
instructions are the next layer's groups of four edge words and the arg-min table's one load.  Cross-compiles both files to gfx950
assembly.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FORMS = ("first", "middle")
ROTATING_EDGES = [23, 0, 23, 21, 19, 23, 21, 12, 6, 17, 23, 18]  # per layer of the 50G-PON code (tests/test_edge_words_cpu.py checks them)
SLACK = 4


def _compile(tmp, name):
    out = tmp / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_%s.hip" % name)], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("isa4e")
    return {"4e": _compile(tmp, "kernel4e"), "4w": _compile(tmp, "kernel4w")}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(ROOT, "tools", "isa_layer_trip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _layers(tool, text, tag, form):
    """instruction classes per layer of one form of lnsfaid_decode<tag>_kernel<2>, between the kernel's own comment lines"""
    body = tool.kernel_body(text, "lnsfaid_decode%s_kernelILi2EE" % tag)
    begin, end = "; lf%s %s begin" % (tag, form), "; lf%s %s end" % (tag, form)
    assert body.count(begin) == 1 and body.count(end) == 1, (tag, form)
    per, layer = {}, None
    for raw in body[body.index(begin):body.index(end)].split("\n"):
        m = re.search(r";\s*lf%s layer (\d+)" % tag, raw)
        if m:
            layer = int(m.group(1))
            continue
        ins = raw.split(";")[0].strip()
        if not re.match(r"^[a-z]", ins):
            continue
        assert not ins.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")), ins  # straight-line
        assert layer is not None, ins
        per.setdefault(layer, []).append(ins)
    assert sorted(per) == list(range(12)), (tag, form)
    return [tool.classes(per[br]) for br in range(12)]


def test_no_scratch_no_spills_no_static_lds(asm):
    text = asm["4e"]
    names = re.findall(r"\.name:\s+(_Z23lnsfaid_decode4e_kernelILi\dEEv12LfKernelArgs)\s", text)
    assert len(set(names)) == 5, names  # DecodeMethods 1..5
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes and all(s == 0 for s in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s*(\d+)", text)]
    print("VGPRs of DecodeMethods 1..5: %s" % vgprs)
    assert vgprs and max(vgprs) <= 256, vgprs
    assert not re.findall(r"^\s*scratch_", text, flags=re.M)
    assert all(int(x) == 0 for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text))  # En is addressed from LDS offset 0


def test_headline_registers(asm):
    text = asm["4e"]
    notes = text[re.search(r"^_Z\w*lnsfaid_decode4e_kernelILi2EE\w*:", text, flags=re.M).end():]
    vgprs = int(re.search(r"; NumVgprs: (\d+)", notes).group(1))
    print("lnsfaid_decode4e_kernel<2>: %d VGPRs, %d bytes of code" % (vgprs, int(re.search(r"; codeLenInByte = (\d+)", notes).group(1))))
    assert vgprs <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", notes).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", notes).group(1)) == 2  # two waves per SIMD


@pytest.mark.parametrize("form", FORMS)
def test_two_valu_instructions_less_per_rotating_edge(asm, tool, form):
    new, old = _layers(tool, asm["4e"], "4e", form), _layers(tool, asm["4w"], "4w", form)
    got, ref = [c["valu"] for c in new], [c["valu"] for c in old]
    print("%s form, VALU per layer: %s = %d (lnsfaid_kernel4w.hip: %s = %d)" % (form, got, sum(got), ref, sum(ref)))
    for br in range(12):
        assert got[br] <= ref[br] - 2 * ROTATING_EDGES[br] + SLACK, (br, got[br], ref[br])
    assert [c["rotates"] for c in new] == [c["rotates"] for c in old]  # the rotations themselves stay


@pytest.mark.parametrize("form", FORMS)
def test_vector_memory_instructions_per_layer(asm, tool, form):
    new = _layers(tool, asm["4e"], "4e", form)
    got = [c["vmem"] for c in new]
    print("%s form, vector-memory instructions per layer: %s" % (form, got))
    for br in range(12):
        nxt = ROTATING_EDGES[br + 1] if br + 1 < 12 else 0  # layer 0's words arrive in front of the iteration
        assert got[br] <= (nxt + 3) // 4 + 1, (br, got[br])
    body = tool.kernel_body(asm["4e"], "lnsfaid_decode4e_kernelILi2EE")
    hot = body[body.index("; lf4e %s begin" % form):body.index("; lf4e %s end" % form)]
    assert "s_load_dword" not in hot and "s_set_gpr_idx" not in hot and "v_movrel" not in hot
    # every load has its base in SGPRs and ONE offset register (a group whose padding nobody reads is loaded narrower than 16 bytes)
    loads = re.findall(r"^\s*(global_load_dword\w*) (.*)$", hot, flags=re.M)
    assert len(loads) == sum(got), (len(loads), got)
    assert all(re.match(r"v(\d+|\[\d+:\d+\]), v\d+, s\[\d+:\d+\]", ops) for _, ops in loads), [l for l in loads if "off" in l[1]][:3]
