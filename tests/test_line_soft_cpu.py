"""Line-format soft channel without a GPU (include/lnsfaid.h "line-format soft channel"): the host form - the
definition of what the device call returns - byte for byte against the independent numpy restatement (tests/line_soft_ref.py),
paging, domain separation, the level histogram at a fixed key, the flip counts, the table helper against math.erfc, the error rules,
the stand-alone sanitizer program, the compiled kernel's resources and the driver's argument handling."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import line_link_ref as ll
import line_soft_ref as ls
from test_line_cpu import _header_prototype
from test_line_link_cpu import _codes, _dims, _line
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL = -1
KEY = 0x5EED0F50C0DE2025
FIRSTS = [0, 7, 2 ** 32 + 5]
NEW_SYMBOLS = {"lnsfaid_line_awgn_table": 3, "lnsfaid_line_soft_device": 9, "lnsfaid_line_soft_host": 9}
K50, L50 = 14592, 17280


def tables():
    """the four tables of the tests: AWGN at 4.2 dB with the default scale; all zero (every level +-7, no flips); the lower seven 0 and
    the upper seven 0xFFFFFFFF (every level 0 except where u is 0xFFFFFFFF); all 0xFFFFFFFF"""
    return {"awgn": ls.awgn_table(ls.ebn0_sigma(4.2, K50, L50), ls.DEFAULT_SCALE), "zero": [0] * 14,
            "middle": [0] * 7 + [0xFFFFFFFF] * 7, "ones": [0xFFFFFFFF] * 14}


@pytest.mark.parametrize("which", ["50gpon", "small"])
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [1, 31, 33])
def test_host_form_equals_the_numpy_reference(abi, lib, code50, which, first, n):
    code = _codes(abi, code50)[which]
    _, L = _dims(code)
    line = _line(n, L, 17 * n)
    for name, table in tables().items():
        out, flips, total = abi.line_soft_host(code, line, n, KEY, first, table, total=11, lib=lib)
        want, want_flips, want_total = ls.soft(line, KEY, first, table, L)
        assert out.shape == want.shape == (n, L // 2)
        assert out.tobytes() == want.tobytes(), name
        assert np.array_equal(flips, want_flips) and total == 11 + want_total, name
        lev = ls.levels(out)
        assert lev.min() >= -7, name
        if name == "zero":
            assert (np.abs(lev) == 7).all() and total == 11
        if name == "middle":
            assert (lev == 0).all()  # u == 0xFFFFFFFF does not occur in these draws (numpy agrees byte for byte either way)


def test_codeword_number_wraps(abi, lib, code50):
    """C = first_codeword + i is a uint64 that wraps: the run over the wrap is the two runs on either side of it"""
    code = code50.code
    _, L = _dims(code)
    first = 2 ** 64 - 2
    line = _line(4, L, 3)
    table = tables()["awgn"]
    out, flips, total = abi.line_soft_host(code, line, 4, KEY, first, table, lib=lib)
    want = ls.soft(line, KEY, first, table, L)
    assert out.tobytes() == want[0].tobytes() and np.array_equal(flips, want[1]) and total == want[2]
    assert np.array_equal(out[2:], abi.line_soft_host(code, line[2:], 2, KEY, 0, table, lib=lib)[0])


@pytest.mark.parametrize("a,m,n", [(0, 1, 33), (7, 16, 33), (2 ** 32 + 5, 32, 33), (5, 31, 31)])
def test_paging(abi, lib, code50, a, m, n):
    """two calls over [a, a + m) and [a + m, a + n) concatenate to the one-shot bytes, flips and total"""
    code = code50.code
    _, L = _dims(code)
    line = _line(n, L, 99)
    table = tables()["awgn"]
    out, flips, total = abi.line_soft_host(code, line, n, KEY, a, table, lib=lib)
    o1, f1, t1 = abi.line_soft_host(code, line[:m], m, KEY, a, table, lib=lib)
    o2, f2, t2 = abi.line_soft_host(code, line[m:], n - m, KEY, a + m, table, total=t1, lib=lib)
    assert np.array_equal(np.concatenate([o1, o2]), out) and np.array_equal(np.concatenate([f1, f2]), flips) and t2 == total


def test_soft_draws_differ_from_payload_and_bsc(abi, lib, code50):
    """domain separation: with table[6] = 2^31 and the rest at the ends, the level's sign is the top bit of every half draw; neither the
    payload's words nor the BSC's flips of the same key, codeword and q are the numbers it was made from"""
    code = code50.code
    K, L = _dims(code)
    n = 4
    table = [0] * 6 + [2 ** 31] + [0xFFFFFFFF] * 7   # m = 0 where u >= 2^31, -1 below
    ones = np.full((n, L // 32), 0xFFFFFFFF, np.uint32)
    out, _, _ = abi.line_soft_host(code, ones, n, KEY, 0, table, lib=lib)
    top_set = ls.levels(out) == 0  # one bit per half draw
    pay = abi.line_payload_random_host(code, KEY, 0, n, lib)
    agree = (top_set[:, :K // 32] == ((pay >> np.uint32(31)) == 1)).mean()
    assert 0.45 < agree < 0.55, agree
    bsc, _, _ = abi.line_bsc_host(code, np.zeros((n, L // 32), np.uint32), n, KEY, 0, 2 ** 31, lib=lib)
    clear = np.unpackbits(bsc.view(np.uint8).reshape(n, -1), axis=1, bitorder="little").astype(bool)  # set where the BSC's top bit is clear
    agree = (top_set == ~clear).mean()
    assert 0.49 < agree < 0.51, agree
    cw = ll.codeword_numbers(0, n)
    for d in (1, 2):
        assert not np.array_equal(ll.draw(KEY, cw, d, np.arange(8)), ll.draw(KEY, cw, 3, np.arange(8)))


def test_level_histogram_at_a_fixed_key(abi, lib, code50):
    """96 codewords of an alternating line at the 3.6 dB table: each of the fifteen counts of m is binomial with
    p_l = (table[l + 7] - table[l + 6]) / 2^32 over n = 96 * 17 280 positions and must lie within 5 sigma of n p_l.  The key is fixed,
    so each count is one number; a count outside its band means the generator or the level rule is wrong, not the key."""
    code = code50.code
    K, L = _dims(code)
    n = 96
    table = abi.line_awgn_table(ls.ebn0_sigma(3.6, K, L), ls.DEFAULT_SCALE, lib)
    line = np.full((n, L // 32), 0xAAAAAAAA, np.uint32)
    out, flips, total = abi.line_soft_host(code, line, n, KEY, 0, table, lib=lib)
    lev = ls.levels(out)
    bits = np.tile(np.array([0, 1], np.int64), L // 2)[None, :]
    m = np.where(bits == 1, lev, -lev)
    edges = [0] + [int(t) for t in table] + [2 ** 32]
    positions = n * L
    got = [int((m == l).sum()) for l in range(-7, 8)]
    print("counts of m = -7 .. 7:", got)
    assert sum(got) == positions
    for l, count in zip(range(-7, 8), got):
        p = (edges[l + 8] - edges[l + 7]) / 2 ** 32
        sigma = math.sqrt(positions * p * (1 - p))
        print("m %+d: %d, mean %.1f, sigma %.1f" % (l, count, positions * p, sigma))
        assert abs(count - positions * p) <= 5 * sigma, (l, count, positions * p, sigma)
    # both position classes and both bit values see the same channel
    for sel in (slice(0, None, 2), slice(1, None, 2)):
        part = int((m[:, sel] < 0).sum())
        p = edges[7] / 2 ** 32
        assert abs(part - positions / 2 * p) <= 5 * math.sqrt(positions / 2 * p * (1 - p))


@pytest.mark.parametrize("which", ["50gpon", "small"])
def test_flips_are_the_channels_decisions_against_the_line(abi, lib, code50, which):
    code = _codes(abi, code50)[which]
    _, L = _dims(code)
    n = 7
    line = _line(n, L, 5)
    bits = np.unpackbits(line.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
    for name, table in tables().items():
        out, flips, total = abi.line_soft_host(code, line, n, KEY, 3, table, total=5, lib=lib)
        lev = ls.levels(out)
        want = ((lev > 0) != (bits == 1)).sum(axis=1)
        assert np.array_equal(flips, want) and total == 5 + int(want.sum()), name
        if name == "middle":  # every level 0: exactly the sent ones count
            assert np.array_equal(flips, bits.sum(axis=1))
        if name == "ones":    # every level the wrong sign
            assert total == 5 + n * L


@pytest.mark.parametrize("sigma,scale", [(0.474, 9.19238816), (0.6, 13.0), (0.05, 9.19238816), (5.0, 1.0)])
def test_awgn_table_against_erfc(abi, lib, sigma, scale):
    """every entry within +-1 of the same formula through math.erfc: one ulp of a double erfc times 2^32 is far below 1, so a differing
    last bit moves the floor only when the fraction sits on an integer"""
    got = abi.line_awgn_table(sigma, scale, lib)
    want = ls.awgn_table(sigma, scale)
    assert got.dtype == np.uint32 and got.shape == (14,)
    assert all(abs(int(g) - w) <= 1 for g, w in zip(got, want)), (got.tolist(), want)
    assert all(int(a) <= int(b) for a, b in zip(got[:-1], got[1:]))


def test_awgn_table_refusals(abi, lib):
    table = np.full(14, 123, np.uint32)
    for sigma, scale in ((0.0, 9.0), (-0.5, 9.0), (float("nan"), 9.0), (float("inf"), 9.0), (0.5, 0.0), (0.5, -1.0), (0.5, float("nan")),
                         (0.5, float("inf"))):
        assert lib.lnsfaid_line_awgn_table(sigma, scale, table.ctypes.data) == E_INVAL, (sigma, scale)
        assert (table == 123).all()
        with pytest.raises(ValueError):
            abi.line_awgn_table(sigma, scale, lib)
    assert lib.lnsfaid_line_awgn_table(0.5, 9.0, None) == E_INVAL


def test_error_rules(abi, lib, code50):
    code = code50.code
    _, L = _dims(code)
    n = 2
    line = _line(n, L, 2).reshape(-1)
    out = np.full(n * L // 2, 0x5A, np.uint8)
    flips = np.full(n, 0x5A5A5A5A, np.uint32)
    table = np.array(tables()["awgn"], np.uint32)
    down = table.copy()
    down[9] = down[8] - 1
    total = C.c_uint64(77)
    pc = C.byref(code)
    soft = lib.lnsfaid_line_soft_host
    good = (line.ctypes.data, n, KEY, 0, table.ctypes.data, out.ctypes.data, flips.ctypes.data, C.byref(total))
    assert soft(None, *good) == E_INVAL
    assert soft(pc, None, *good[1:]) == E_INVAL
    assert soft(pc, *good[:4], None, *good[5:]) == E_INVAL
    assert soft(pc, *good[:5], None, *good[6:]) == E_INVAL
    assert soft(pc, *good[:4], down.ctypes.data, *good[5:]) == E_INVAL                     # a table that decreases
    # overlapping byte ranges: the input at the first byte of the output, at its last byte, and the output inside the input
    both = np.full(n * L // 2 + n * L // 8, 0x5A, np.uint8)
    o = both.ctypes.data
    assert soft(pc, o, n, KEY, 0, table.ctypes.data, o, None, C.byref(total)) == E_INVAL
    assert soft(pc, o + n * L // 2 - 1, n, KEY, 0, table.ctypes.data, o, None, C.byref(total)) == E_INVAL
    assert soft(pc, o, n, KEY, 0, table.ctypes.data, o + n * L // 8 - 1, None, C.byref(total)) == E_INVAL
    # L or K not a multiple of 32
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert soft(C.byref(broken), *good) == E_INVAL, field
    assert (out == 0x5A).all() and (flips == 0x5A5A5A5A).all() and (both == 0x5A).all() and total.value == 77
    # n_codewords 0: a no-op, NULL buffers allowed
    assert soft(pc, None, 0, KEY, 0, None, None, None, None) == 0
    assert soft(pc, line.ctypes.data, 0, KEY, 0, table.ctypes.data, out.ctypes.data, flips.ctypes.data, C.byref(total)) == 0
    assert (out == 0x5A).all() and (flips == 0x5A5A5A5A).all() and total.value == 77
    # ranges that touch but do not overlap are fine, and exactly n codewords are written; the optional outputs may be NULL
    both[:n * L // 8] = line.view(np.uint8)
    assert soft(pc, o, n, KEY, 0, table.ctypes.data, o + n * L // 8, None, None) == 0
    assert both[n * L // 8:].tobytes() == ls.soft(line.reshape(n, -1), KEY, 0, table, L)[0].tobytes()
    wide = np.full((n + 1) * L // 2, 0x5A, np.uint8)
    assert soft(pc, line.ctypes.data, n, KEY, 0, table.ctypes.data, wide.ctypes.data, None, None) == 0
    assert (wide[n * L // 2:] == 0x5A).all() and wide[:n * L // 2].tobytes() == both[n * L // 8:].tobytes()


def test_device_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(1 << 12, np.uint32)
    table = np.zeros(14, np.uint32)
    total = C.c_uint64(0)
    p = buf.ctypes.data
    assert lib.lnsfaid_line_soft_device(None, p, 1, KEY, 0, table.ctypes.data, p + 8192, None, C.byref(total)) == E_INVAL
    assert lib.lnsfaid_line_soft_device(None, None, 0, KEY, 0, None, None, None, None) == E_INVAL
    assert not buf.any() and total.value == 0


@pytest.mark.parametrize("name", sorted(NEW_SYMBOLS))
def test_abi_surface(abi, lib, name):
    assert getattr(lib, name) is not None
    res, args = abi.SYMBOLS[name]
    assert res is C.c_int
    proto = _header_prototype(name)
    assert len(args) == len(proto) == NEW_SYMBOLS[name], (name, args, proto)
    for a, t in zip(args, proto):
        if t == "const lnsfaid_code*":
            assert a == C.POINTER(abi.Code)
        elif t == "uint64_t":
            assert a is C.c_uint64
        elif t == "size_t":
            assert a is C.c_size_t
        elif t == "double":
            assert a is C.c_double
        elif t == "uint64_t*":
            assert a == C.POINTER(C.c_uint64)


def test_stand_alone_program_under_the_sanitizers():
    """host/line_soft_selftest.cpp: the host form and the helper on heap buffers of exactly the documented sizes at odd addresses, built
    with the Makefile's $(SANITIZE) flags and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "line_soft_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "line_soft_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "line_soft_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_kernel_resources(tmp_path):
    """no scratch, no spills, at most 64 VGPRs: eight waves per SIMD stay resident"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / "line_soft.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_line_soft.hip")], check=True, capture_output=True)
    meta = {k: v for k, v in kernel_meta(out.read_text()).items() if "lnsfaid_line_soft_kernel" in k}
    assert len(meta) == 2, sorted(meta)  # the 16-byte and the 4-byte store form
    for name, (vgpr, spill, scratch) in meta.items():
        assert vgpr <= 64 and spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


@pytest.mark.parametrize("args", [
    ["--ebn0", "4.2", "--ber", "0.01", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ebn0", "4.2", "--magnitude", "4", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--scale", "9.0", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ebn0", "x", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
], ids=["ebn0_with_ber", "ebn0_with_magnitude", "scale_without_ebn0", "ebn0_x"])
def test_line_sim_bad_arguments(tmp_path, args):
    """the usage line and status 2, before anything touches a GPU or writes a file"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert r.stderr.startswith("usage: ") and "--ber" in r.stderr and "--ebn0" in r.stderr and r.stderr.count("\n") == 1
    assert not os.listdir(str(tmp_path))
