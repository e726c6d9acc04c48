"""The layer step written for the issue classes (SW_FORM_VK | SW_FORM_MUL of sw_layer_step), compiled for the host:
tests/class_moves_emul.cpp checks every new helper against the expression it replaces - exhaustively over one byte lane in every
byte position crossed with every shift amount the multiply form can serve (8 .. 23; the step uses 8, and an addition for its shift by one), and on 10^6 random
dwords, three quarters of which and more have bits 24 .. 31 set: where a 24-bit multiply differs from a shift - and runs the forms
lnsfaid_kernel4w.hip instantiated before and the new ones (both bits, and each alone) over every lane of every layer of the built-in
code (degrees 23 and 22) for four iterations, first-iteration and middle forms: En images and rows' records byte for byte.  Three kinds
of En image: the channel's range, the whole range, corner values only.  DecodeMethods 2, 1 and 5.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from test_static_layers_cpu import CSRC, ROOT, _zero_first_rows

N_ITER, N_SEEDS, N_RANDOM = 4, 3, 1000000


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("class_moves") / "class_moves_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests"), "-o", str(exe), os.path.join(ROOT, "tests", "class_moves_emul.cpp")], check=True)
    return str(exe)


@pytest.mark.parametrize("method", [2, 1, 5])
def test_class_moves_equal_the_default_forms(abi, lib, code50, emul, tmp_path, method):
    rows = _zero_first_rows(abi, lib, code50)
    cfg = abi.default_cfg(method, 10, lib)
    lines = ["%d %s" % (len(row), " ".join(map(str, row))) for row in rows]
    lines.append("%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value))
    for tab in (cfg.v2c_map, cfg.v2c_map_ef):
        for it in range(6):
            lines.append(" ".join(str(int(tab[it][0][a])) for a in range(8)))
    lines.append("%d %d %d" % (N_ITER, N_SEEDS, N_RANDOM))
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    high = re.match(r"random dwords with bits 24..31 set: (\d+) of (\d+)", out[0])
    assert high and int(high.group(2)) == N_RANDOM and int(high.group(1)) > N_RANDOM // 2, out[0]
    # the bound on the shift amount is a real one: a 24-bit multiply by 4 is not the shift by 2
    assert int(re.match(r"dwords on which a 24-bit multiply by 4 is not the shift: (\d+)", out[1]).group(1)) > 0, out[1]
    per_dword = 4 + 16  # sw_shl8_mul, sw_mask7_mul, sw_mask6_mul, sw_gather4_perm, sw_mul_u24 by 1 << 8 .. 1 << 23
    assert int(re.match(r"helper results compared: (\d+)", out[2]).group(1)) >= per_dword * (N_RANDOM + 4 * 256 * 6), out[2]
    assert out[3] == "helper mismatches: 0", out[3]
    degs = re.match(r"layer runs of degree 22 / 23: (\d+) / (\d+)", out[-3])
    assert degs and int(degs.group(1)) > 0 and int(degs.group(2)) > 0, out[-3]
    assert out[-2] == "rows compared: %d" % (12 * 256 * N_ITER * N_SEEDS), out[-2]
    assert out[-1] == "total mismatches: 0", out[-1]
