"""The edge words of the window-free kernel's twin without a GPU (lnsfaid_kernel4e.hip).  The table: every field of
sw50_edge_word (csrc/lnsfaid_static50.h) for every layer, rotating edge and lane - 206 x 64 words - against the shifts of the
library's zero-first tables, and the memory image the kernel loads, [layer][group of four rotating edges][lane][4] with zero padding.
The step: sw_layer_step of csrc/lnsfaid_swar.h compiled for the host, in the two forms of lnsfaid_kernel4w.hip with and without
SW_FORM_EDGEW on the same random En images, every layer of the built-in code, DecodeMethods 1, 2 and 5: identical En images and
records (tests/edge_words_emul.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")

ROTATING_EDGES = [23, 0, 23, 21, 19, 23, 21, 12, 6, 17, 23, 18]  # per layer of the 50G-PON code: 275 circulants less 69 identities


def _zero_first_shifts(abi, lib, code50):
    """the shift of every layer's edges in the order of the library's rotation-free tables (identities first)"""
    pos = np.ctypeslib.as_array(code50.pos_vn)
    degs = [d for d, n in zip(code50.deg, code50.deg_rows) for _ in range(n // 256)]
    _, order = abi.code_zero_shift_order(code50.code, lib)
    rows, e = [], 0
    for br, d in enumerate(degs):
        row = [int(v) % 256 for v in pos[e:e + d]]
        rows.append([row[j] for j in order[br][:d]])
        e += 256 * d
    assert len(rows) == 12 and e == 70400
    return rows


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("edge_words") / "edge_words_emul"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "edge_words_emul.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def dumped(emul, tmp_path_factory):
    d = tmp_path_factory.mktemp("edge_words_dump")
    r = subprocess.run([emul, "dump", str(d / "words.bin"), str(d / "image.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    layers = [tuple(int(x) for x in line.split()) for line in r.stdout.strip().splitlines()]
    return layers, np.fromfile(d / "words.bin", dtype=np.uint32), np.fromfile(d / "image.bin", dtype=np.uint32)


def test_every_field_of_every_word(abi, lib, code50, dumped):
    layers, words, _ = dumped
    shifts = _zero_first_shifts(abi, lib, code50)
    assert [deg - nz for _, deg, nz in layers] == ROTATING_EDGES and sum(ROTATING_EDGES) == 206
    assert words.size == 206 * 64
    lane = np.arange(64, dtype=np.uint32)
    at, checked = 0, 0
    for (br, deg, nz), row in zip(layers, shifts):
        assert len(row) == deg and all(s == 0 for s in row[:nz]) and all(s != 0 for s in row[nz:])
        for j in range(nz, deg):
            w = words[at:at + 64]
            at += 64
            x4 = 4 * (lane + np.uint32(row[j]))
            rq = (x4 >> 8) & 3
            assert np.array_equal(w & 0xfc, x4 & 0xfc), (br, j)
            assert np.array_equal(w & 3, rq), (br, j)
            assert np.array_equal((w >> 8) & 3, (4 - rq) & 3), (br, j)
            assert not (w & ~np.uint32(0x3ff)).any(), (br, j)  # nothing else in the word
            checked += 64
    assert at == words.size and checked == 206 * 64


def test_memory_image(dumped):
    layers, words, image = dumped
    groups = [(r + 3) // 4 for r in ROTATING_EDGES]
    assert sum(groups) == 56 and image.size == 56 * 256  # 1 KB per group: one 16-byte load per lane
    image = image.reshape(56, 64, 4)
    g0, at = 0, 0
    for (br, deg, nz), ng in zip(layers, groups):
        rot = deg - nz
        for e in range(4 * ng):
            got = image[g0 + e // 4, :, e % 4]
            if e < rot:
                assert np.array_equal(got, words[at:at + 64]), (br, e)
                at += 64
            else:
                assert not got.any(), (br, e)  # the padding of the layer's last group
        g0 += ng
    assert g0 == 56 and at == words.size


@pytest.mark.parametrize("method", [2, 1, 5])
def test_step_with_edge_words_equals_the_step_without(abi, lib, emul, tmp_path, method):
    cfg = abi.default_cfg(method, 10, lib)
    lines = ["%d %d %d" % (method, C.c_int8(cfg.factor_1).value, C.c_int8(cfg.factor_2).value)]
    for it in range(6):
        lines.append(" ".join(str(int(cfg.v2c_map[it][0][a])) for a in range(8)))
    lines.append("4 3")  # four iterations (the first in the first form, three in the later one), three random En images
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, "step", str(spec)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "total mismatches: 0", out[-1]
    assert out[-2] == "rows compared: %d" % (12 * 256 * 4 * 3), out[-2]
