"""The rotation-free layer step without a GPU (lnsfaid_kernel4z.hip): the edge order the host builds for it, and
the layer step of csrc/lnsfaid_swar.h compiled for the host and run with that order and the rotation-free instances against the
code's own order and the rotating instances (tests/zero_shift_emul.cpp): equal En images after every layer, equal records after
undoing the permutation."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")

ZG_50GPON = [0, 5, 0, 0, 1, 0, 0, 2, 4, 1, 0, 1]
COMPILED = {23: (0, 1, 2, 4), 22: (0, 5)}  # the (degree, ZG) instances of lnsfaid_kernel4z.hip


def _rows_50gpon(code50):
    """block column * 256 + shift of every layer's edges, in the code's own order"""
    pos = np.ctypeslib.as_array(code50.pos_vn)
    degs = [d for d, n in zip(code50.deg, code50.deg_rows) for _ in range(n // 256)]
    rows, e = [], 0
    for d in degs:
        rows.append([int(v) for v in pos[e:e + d]])
        e += 256 * d
    assert e == 70400 and len(rows) == 12
    return rows


def _zero_first(row):
    order = [j for j, sb in enumerate(row) if sb % 256 == 0] + [j for j, sb in enumerate(row) if sb % 256 != 0]
    return order, sum(1 for sb in row if sb % 256 == 0) // 4


def _in_use(lib, deg, zg):
    """the library's rounding to a compiled instance: (lf_decode4z_inst >> 8) & 0xff"""
    C.CDLL(lib._name).lf_decode4z_inst.restype = C.c_int
    got = (C.CDLL(lib._name).lf_decode4z_inst(C.c_int(deg), C.c_int(zg)) >> 8) & 0xff
    assert got == max([g for g in COMPILED.get(deg, (0,)) if g <= zg]), (deg, zg, got)
    return got


def test_edge_order_of_the_built_in_code(abi, lib, code50):
    groups, order = abi.code_zero_shift_order(code50.code, lib)
    assert groups == ZG_50GPON
    rows = _rows_50gpon(code50)
    assert sum(len(r) for r in rows) == 275
    for br, row in enumerate(rows):
        assert sorted(order[br]) == list(range(len(row))), br  # a permutation of the reference row
        shifts = [row[j] % 256 for j in order[br]]
        n_zero = shifts.count(0)
        assert all(s == 0 for s in shifts[:n_zero]) and all(s != 0 for s in shifts[n_zero:]), br
        cols = [row[j] // 256 for j in order[br]]
        assert cols[:n_zero] == sorted(cols[:n_zero]) and cols[n_zero:] == sorted(cols[n_zero:]), br  # ascending in either class
        assert order[br] == _zero_first(row)[0] and groups[br] == n_zero // 4
        assert _in_use(lib, len(row), groups[br]) == groups[br]  # every layer of this code has an instance of its own


def test_rounding_to_a_compiled_instance(lib):
    for deg in (23, 22, 21, 8):
        for zg in range(0, deg // 4 + 1):
            _in_use(lib, deg, zg)
    assert _in_use(lib, 23, 5) == 4 and _in_use(lib, 23, 3) == 2 and _in_use(lib, 22, 4) == 0 and _in_use(lib, 21, 5) == 0


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("zero_shift") / "zero_shift_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "zero_shift_emul.cpp")], check=True)
    return str(exe)


def _synthetic(kind):
    rng = np.random.default_rng(7)
    def row(deg, zero_at):
        return [256 * cb + (0 if j in zero_at else int(rng.integers(1, 256))) for j, cb in enumerate(sorted(rng.choice(26, deg, replace=False).tolist()))]
    if kind == "all_zero":  # a degree-23 layer of identity circulants only: 5 groups, no such instance, runs on ZG 4
        return [row(23, range(23)), row(23, ()), row(22, range(22))]
    return [row(23, (2, 9, 20)), row(22, (0, 1, 21)), row(23, (22,)), row(17, (3, 4, 5, 6, 16))]  # three zero shifts: ZG 0; a generic degree


@pytest.mark.parametrize("method", [2, 1, 5])
@pytest.mark.parametrize("matrix", ["50gpon", "all_zero", "three_zeros"])
def test_rotation_free_step_equals_the_rotating_step(abi, lib, code50, emul, tmp_path, matrix, method):
    rows = _rows_50gpon(code50) if matrix == "50gpon" else _synthetic(matrix)
    cfg = abi.default_cfg(method, 10, lib)
    lines = [str(len(rows))]
    used = []
    for row in rows:
        order, zg = _zero_first(row)
        used.append(_in_use(lib, len(row), zg))
        lines.append("%d %d %s %s" % (len(row), used[-1], " ".join(map(str, row)), " ".join(map(str, order))))
    if matrix == "50gpon":
        assert used == ZG_50GPON
    elif matrix == "all_zero":
        assert used == [4, 0, 5]
    else:
        assert used == [0, 0, 0, 0]
    lines.append("%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value))
    for tab in (cfg.v2c_map, cfg.v2c_map_ef):
        for it in range(6):
            lines.append(" ".join(str(int(tab[it][0][a])) for a in range(8)))
    lines.append("3 2")  # three iterations (the first one fresh), two random En images
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "total mismatches: 0", out[-1]
    assert out[-2].startswith("rows compared: %d," % (len(rows) * 256 * 3 * 2)), out[-2]
