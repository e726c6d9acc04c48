"""Build-time properties of what a layered iteration issues OUTSIDE its layers: the decision point with its cheap
"certainly dirty" test and the iteration's set-up.  On the headline instance lnsfaid_decode4s_kernel<2> the way from the kernel's
comment line "lf4s layers end" to "lf4s layers begin" is walked by tools/isa_decision_point.py as an iteration after the first takes
it outside the error-floor window with stage 1 of the test reporting dirty; on the kernels that run their layers through a loop
and take the run-time form of the test (lnsfaid_kernel4z.hip, lnsfaid_kernel4cw.hip) the span from the layered loop's header to the
layer loop is looked at.  The parent of this test issued about 580 instructions on that way, 46 of them scalar loads of the code's tables each waited for on its own, and
about 70 conditional branches.  Cross-compiles the files to gfx950 assembly.  No GPU needed."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# what this tree reaches on lnsfaid_decode4s_kernel<2>
WAY = 131           # instructions of every kind from the end of the layers to their begin (bound set by the issue: below 300)
COND_BRANCHES = 7   # loop condition, METHOD / window / front tests, the ballot of stage 1, the two skips over the syndrome stage
CONFIG_LOADS = 1    # floor_iter_thresh; the iteration's tables are loaded inside layer 0, where the parent loaded them
STAGE1 = 49         # 22 edges: 11 ds_read2_b32, 22 adds, 11 three-input XORs, and, compare, two waits, the branch


def _compile(tmp, name):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, name + ".hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_decision_point", os.path.join(ROOT, "tools", "isa_decision_point.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def way(tmp_path_factory, tool):
    res = tool.measure(_compile(tmp_path_factory.mktemp("isa_dp4s"), "lnsfaid_kernel4s"))
    print("lnsfaid_decode4s_kernel<2>, outside the layers: %s" % res)
    return res


def test_no_code_table_is_loaded_at_a_decision_point(way):
    """layer degrees, shifts and block columns are compile-time constants of the static kernel: what is left of scalar loads on the
    way are words of the decoder's configuration, none of them from the code (the parent: 46 from s4tab / cbtab)"""
    assert len(way["scalar_loads"]) <= CONFIG_LOADS <= 3, way["scalar_loads"]
    assert way["way"]["smem"] == len(way["scalar_loads"])
    assert all(re.match(r"s_load_dword\s", x) for x in way["scalar_loads"]), way["scalar_loads"]  # single words, no table rows


def test_no_scalar_load_is_waited_for_on_its_own_inside_the_check(way):
    assert way["stage1"]["smem"] == 0 and way["stage1_waited_alone"] == 0, way["stage1"]
    assert way["stage2"]["smem"] == 0, way["stage2"]
    # stage 1: straight-line, every read from the lane's own dword (no rotation), nothing scalar but the waits and the branch
    assert way["stage1"]["rotates"] == 0 and way["stage1"]["salu"] == 0 and way["stage1"]["branch"] == 1, way["stage1"]
    assert way["stage1"]["all"] <= STAGE1, way["stage1"]
    # stage 2 (layer 0: no identity circulant): one rotate per edge, one branch (on its ballot)
    assert way["stage2"]["rotates"] == 23 and way["stage2"]["branch"] == 1, way["stage2"]


def test_a_handful_of_branches_and_fewer_than_300_instructions(way):
    assert way["cond_branches"] <= COND_BRANCHES <= 8, way["cond_branches"]
    assert way["way"]["branch"] == way["cond_branches"]  # no unconditional jump on the way
    assert WAY < 300
    assert way["way"]["all"] <= WAY, way["way"]


@pytest.mark.parametrize("name,kernel", [("lnsfaid_kernel4z", "lnsfaid_decode4z_kernelILi2EE"),
                                         ("lnsfaid_kernel4cw", "lnsfaid_decode4cw_kernelILi2ELb1ELb0E")])
def test_the_loop_kernels_fetch_the_check_tables_together(tmp_path_factory, tool, name, kernel):
    """the run-time check (sw_row_parity) loads whole table rows: from the layered loop's header to the layer loop at most three
    scalar loads are directly followed by a wait of their own (the old text: one per edge and table; 24 such pairs in
    lnsfaid_decode4z_kernel<2>).  lnsfaid_kernel4.hip is not asserted: it stays on the old text, with which alone the ratchets of
    tests/test_layer_trip_count.py on its layer blocks hold."""
    res = tool.loop_span(_compile(tmp_path_factory.mktemp("isa_dp_" + name), name), kernel)
    print("%s: %s" % (kernel, res))
    assert res["waited_alone"] <= 3, res
