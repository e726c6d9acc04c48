"""Build-time properties of the window-free layer-static kernel (lnsfaid_kernel4w.hip), on the headline instance
lnsfaid_decode4w_kernel<2>: what the one-wave kernels hold (no scratch, no spills, two waves per SIMD, no static LDS), its code size,
and a ratchet on what a layered iteration issues in each of its two forms - the twelve straight-line layers between the kernel's own
comment lines in the assembly, classified by tools/isa_layer_trip.py - against the layer-static kernel's iteration
(tests/test_static_layers_isa.py: PER_LAYER, the way an iteration after the first takes outside the error-floor window).  Counts are
exact, so the ceilings are the counts this tree reaches.  Cross-compiles the file to gfx950 assembly.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lnsfaid_decode4w_kernelILi2EE"
FORMS = ("first", "middle")

# the layer-static kernel's iteration, layer by layer, the reference of this ratchet: what lnsfaid_decode4s_kernel<2> issues in the tree
# this kernel was added to, walked as tests/test_static_layers_isa.py walks it (10 640 per iteration; that file's PER_LAYER holds older,
# higher ceilings, which these are below layer for layer), and the same walk of its first iteration (no patch of old arg-min nodes)
STATIC_PER_LAYER = [946, 757, 924, 911, 896, 930, 915, 852, 817, 883, 923, 886]
STATIC_FIRST_PER_LAYER = [919, 730, 897, 884, 869, 903, 888, 825, 790, 856, 896, 859]
STATIC_CEILINGS = [972, 781, 950, 936, 921, 955, 941, 878, 840, 907, 949, 911]
# what this tree reaches: instructions of every kind per layer, in either form, and their split over the iteration
PER_LAYER = {"first": [807, 638, 807, 792, 778, 812, 798, 736, 696, 766, 806, 770],
             "middle": [910, 743, 912, 898, 884, 917, 905, 842, 805, 872, 912, 873]}
ITERATION = {"first": {"all": 9206, "valu": 8386, "lds": 620}, "middle": {"all": 10473, "valu": 9560, "lds": 716}}
ROTATES = 2 * (275 - 69)  # as in the layer-static kernel: the edges that are no identity circulants, read and write-back
CODE_BYTES = 187500  # the whole kernel: two texts of the iteration (the layer-static kernel with one: 125 040)
VGPRS = 226


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa4w") / "kernel4w.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4w.hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(ROOT, "tools", "isa_layer_trip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _region(body, form):
    assert body.count("; lf4w %s begin" % form) == 1 and body.count("; lf4w %s end" % form) == 1, form
    return body[body.index("; lf4w %s begin" % form):body.index("; lf4w %s end" % form)]


def _layers(region):
    """instructions per layer of one form.  Either form is straight-line: the window's block is not compiled, the first iteration
    has no patch of old arg-min nodes and the later ones always have it, so what is counted is what an iteration issues."""
    per, layer = {}, None
    for raw in region.split("\n"):
        m = re.search(r";\s*lf4w layer (\d+)", raw)
        if m:
            layer = int(m.group(1))
            continue
        ins = raw.split(";")[0].strip()
        if not re.match(r"^[a-z]", ins):
            continue
        assert not ins.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")), ins
        assert layer is not None, ins  # nothing between the form's first comment line and its layer 0
        per.setdefault(layer, []).append(ins)
    return per


@pytest.fixture(scope="module")
def forms(asm, tool):
    body = tool.kernel_body(asm, HEADLINE)
    out = {}
    for form in FORMS:
        per = _layers(_region(body, form))
        assert sorted(per) == list(range(12)), (form, sorted(per, key=str))
        out[form] = [tool.classes(per[br]) for br in range(12)]
    return out


def test_no_scratch_no_spills_two_waves_per_simd(asm):
    names = re.findall(r"\.name:\s+(_Z23lnsfaid_decode4w_kernelILi\dEEv12LfKernelArgs)\s", asm)
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
    print("lnsfaid_decode4w_kernel<2>: %d bytes of code, %d VGPRs" % (size, vgprs))
    assert size <= CODE_BYTES and vgprs <= VGPRS
    assert int(re.search(r"; ScratchSize: (\d+)", notes).group(1)) == 0


def test_every_method_has_both_forms(asm, tool):
    for method in range(1, 6):
        body = tool.kernel_body(asm, "lnsfaid_decode4w_kernelILi%dEE" % method)
        for form in FORMS:
            assert sorted(_layers(_region(body, form))) == list(range(12)), (method, form)


def test_a_layer_knows_which_layer_it_is(forms, asm, tool):
    """as the layer-static kernel: no indexed register moves, no dispatch, no table loads; one vector load (the next layer's arg-min
    table) per layer; no scalar loads inside the layers at all (the iteration's parameters arrive in front of the forms)"""
    body = tool.kernel_body(asm, HEADLINE)
    for form in FORMS:
        hot = _region(body, form)
        assert "s_set_gpr_idx" not in hot and "v_movrel" not in hot
        assert "s_load_dword" not in hot
        layers = forms[form]
        assert all(c["vmem"] <= 1 for c in layers) and layers[11]["vmem"] == 0, [c["vmem"] for c in layers]
        assert sum(c["rotates"] for c in layers) == ROTATES
        assert layers[1]["rotates"] == 0  # 22 identity circulants


def test_the_middle_form_issues_less_than_the_layer_static_kernel(forms):
    got = [c["all"] for c in forms["middle"]]
    print("middle form, issued per layer: %s = %d (layer-static kernel: %s = %d)" % (got, sum(got), STATIC_PER_LAYER, sum(STATIC_PER_LAYER)))
    assert all(g < s for g, s in zip(got, STATIC_PER_LAYER)), got
    assert all(w < s for w, s in zip(PER_LAYER["middle"], STATIC_PER_LAYER))
    assert all(s <= c for s, c in zip(STATIC_PER_LAYER, STATIC_CEILINGS))


def test_the_first_form_issues_less_than_the_middle_form(forms):
    first, middle = [c["all"] for c in forms["first"]], [c["all"] for c in forms["middle"]]
    print("first form, issued per layer: %s = %d" % (first, sum(first)))
    assert all(f < m for f, m in zip(first, middle)), (first, middle)
    assert all(f < m for f, m in zip(PER_LAYER["first"], PER_LAYER["middle"]))
    assert all(f < s for f, s in zip(first, STATIC_FIRST_PER_LAYER)), first  # and below the layer-static kernel's own first iteration


@pytest.mark.parametrize("form", FORMS)
def test_ceilings(forms, form):
    layers = forms[form]
    total = {k: sum(c[k] for c in layers) for k in ("all", "valu", "lds")}
    print("%s form: %s per iteration; per layer %s" % (form, total, [c["all"] for c in layers]))
    assert sum(PER_LAYER[form]) == ITERATION[form]["all"]
    assert all(total[k] <= ITERATION[form][k] for k in total), total
    assert all(c["all"] <= want for c, want in zip(layers, PER_LAYER[form])), [c["all"] for c in layers]
