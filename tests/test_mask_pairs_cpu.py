"""The layer step with its masks expanded in pairs (PAIRS = SW_PAIRS_ALL), compiled for the host, against the single
form: tests/mask_pairs_emul.cpp runs the statements of lnsfaid_kernel4s.hip's layer step - compile-time table view, pairs - and the
run-time view on the single form over every lane of every layer of the built-in code for four iterations (the first one fresh, the
last inside the error-floor window) and compares En images and rows' records byte for byte.  Layers of degree 23 (an odd last edge
in the last group) and 22; DecodeMethods 2, 1 and 5.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from test_static_layers_cpu import CSRC, ROOT, _zero_first_rows


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("mask_pairs") / "mask_pairs_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests"), "-o", str(exe), os.path.join(ROOT, "tests", "mask_pairs_emul.cpp")], check=True)
    return str(exe)


@pytest.mark.parametrize("method", [2, 1, 5])
def test_paired_step_equals_the_single_one(abi, lib, code50, emul, tmp_path, method):
    rows = _zero_first_rows(abi, lib, code50)
    cfg = abi.default_cfg(method, 10, lib)
    lines = ["%d %s" % (len(row), " ".join(map(str, row))) for row in rows]
    lines.append("%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value))
    for tab in (cfg.v2c_map, cfg.v2c_map_ef):
        for it in range(6):
            lines.append(" ".join(str(int(tab[it][0][a])) for a in range(8)))
    lines.append("4 2")
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "total mismatches: 0", out[-1]
    assert out[-2] == "rows compared: %d" % (12 * 256 * 4 * 2), out[-2]
