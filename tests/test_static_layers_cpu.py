"""The layer-static decode kernel without a GPU (lnsfaid_kernel4s.hip): its compile-time description of the
50G-PON code (csrc/lnsfaid_static50.h) against the zero-first tables the library builds, entry by entry, and the layer step of
csrc/lnsfaid_swar.h compiled for the host and run through that static table view against the run-time view of the same tables
(tests/static_layers_emul.cpp): every layer, random En and messages, identical records and En images."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")

IDENTITY_EDGES = [0, 22, 0, 2, 4, 0, 2, 11, 17, 6, 0, 5]  # per layer of the 50G-PON code: 69 in all


def _zero_first_rows(abi, lib, code50):
    """block column * 256 + shift of every layer's edges in the order of the library's rotation-free tables"""
    pos = np.ctypeslib.as_array(code50.pos_vn)
    degs = [d for d, n in zip(code50.deg, code50.deg_rows) for _ in range(n // 256)]
    _, order = abi.code_zero_shift_order(code50.code, lib)
    rows, e = [], 0
    for br, d in enumerate(degs):
        row = [int(v) for v in pos[e:e + d]]
        rows.append([row[j] for j in order[br][:d]])
        e += 256 * d
    assert len(rows) == 12 and e == 70400
    return rows


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("static_layers") / "static_layers_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "static_layers_emul.cpp")], check=True)
    return str(exe)


def test_identity_edges_of_the_built_in_code(abi, lib, code50):
    rows = _zero_first_rows(abi, lib, code50)
    assert [sum(1 for sb in row if sb % 256 == 0) for row in rows] == IDENTITY_EDGES and sum(IDENTITY_EDGES) == 69
    for row, nz in zip(rows, IDENTITY_EDGES):
        assert all(sb % 256 == 0 for sb in row[:nz]) and all(sb % 256 != 0 for sb in row[nz:])


@pytest.mark.parametrize("method", [2, 1, 5])
def test_static_table_view_equals_the_library_tables_and_the_run_time_view(abi, lib, code50, emul, tmp_path, method):
    rows = _zero_first_rows(abi, lib, code50)
    cfg = abi.default_cfg(method, 10, lib)
    lines = ["%d %s" % (len(row), " ".join(map(str, row))) for row in rows]
    lines.append("%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value))
    for tab in (cfg.v2c_map, cfg.v2c_map_ef):
        for it in range(6):
            lines.append(" ".join(str(int(tab[it][0][a])) for a in range(8)))
    lines.append("4 2")  # four iterations (the first one fresh, the last one inside the error-floor window), two random En images
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    assert out[0] == "table mismatches: 0", out[0]
    assert out[-1] == "total mismatches: 0", out[-1]
    assert out[-2] == "rows compared: %d" % (12 * 256 * 4 * 2), out[-2]


def test_a_changed_table_is_told_apart(abi, lib, code50, emul, tmp_path):
    """one shift of one layer moved by one: the entry-by-entry comparison names it"""
    rows = _zero_first_rows(abi, lib, code50)
    rows[2][0] += 1
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join("%d %s" % (len(row), " ".join(map(str, row))) for row in rows) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "table mismatches: 1" in r.stdout, r.stdout[-500:]
