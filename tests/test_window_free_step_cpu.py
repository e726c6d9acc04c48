"""The iteration forms of the layer step (FORM of sw_layer_step), compiled for the host, against the generic step:
tests/window_free_emul.cpp checks the thermometer -> magnitude tables of SW_FORM_NOWIN exhaustively (every table of the preset, every
code, every byte) and runs the generic instance (rowpar = 0, lme = false, window = false), the SW_FORM_NOWIN instance and the forms
lnsfaid_kernel4w.hip picks per iteration (SW_FORM_NOWIN | SW_FORM_FRESH first, on a record of garbage) over every lane of every layer
of the built-in code for four iterations: En images and rows' records byte for byte.  Three kinds of En image: the channel's range,
the whole range, corner values only.  DecodeMethods 2, 1 and 5.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from test_static_layers_cpu import CSRC, ROOT, _zero_first_rows

N_ITER, N_SEEDS = 4, 3
TABLES = 6 + 6 + 2 + 2  # per iteration slot the table and the error-floor table, the two min-sum tables, two synthetic ones


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("window_free") / "window_free_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests"), "-o", str(exe), os.path.join(ROOT, "tests", "window_free_emul.cpp")], check=True)
    return str(exe)


@pytest.mark.parametrize("method", [2, 1, 5])
def test_forms_equal_the_generic_step(abi, lib, code50, emul, tmp_path, method):
    rows = _zero_first_rows(abi, lib, code50)
    cfg = abi.default_cfg(method, 10, lib)
    lines = ["%d %s" % (len(row), " ".join(map(str, row))) for row in rows]
    lines.append("%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value))
    for tab in (cfg.v2c_map, cfg.v2c_map_ef):
        for it in range(6):
            lines.append(" ".join(str(int(tab[it][0][a])) for a in range(8)))
    lines.append("%d %d" % (N_ITER, N_SEEDS))
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    assert out[0] == "table look-ups compared: %d" % (TABLES * 4 * 9 * 9), out[0]
    assert out[1] == "table mismatches: 0", out[1]
    assert out[-1] == "total mismatches: 0", out[-1]
    assert out[-2] == "rows compared: %d" % (12 * 256 * N_ITER * N_SEEDS), out[-2]
