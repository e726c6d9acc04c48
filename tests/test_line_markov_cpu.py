"""Line-format error-propagation channel without a GPU (include/lnsfaid.h "line-format error-propagation channel"):
the host form - the definition of what the device call returns - byte for byte against the independent numpy restatement
(tests/line_markov_ref.py), the three consequences the header states, paging, the threshold helper, the statistics of the helper's
chain at a fixed key, the error rules, the stand-alone sanitizer program, the compiled kernel's resources and the driver's argument
handling."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_markov_ref as lm
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
FIRSTS = [0, 2 ** 32 + 5]
NEW_SYMBOLS = {"lnsfaid_line_markov_thresholds": 3, "lnsfaid_line_markov_device": 11, "lnsfaid_line_markov_host": 11}


def threshold_sets():
    """the four sets of the tests: a copy; the helper's chain at (0.01, 0.5); long runs (mean 100); all or nothing"""
    return {"copy": [0, 0, 0], "helper": lm.thresholds(0.01, 0.5), "long": [2 ** 32 // 500, int(math.floor(0.99 * 2 ** 32)), 0],
            "all": [0, 0xFFFFFFFF, 2 ** 31]}


@pytest.mark.parametrize("which", ["50gpon", "small"])
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [1, 3])
def test_host_form_equals_the_numpy_reference(abi, lib, code50, which, first, n):
    code = _codes(abi, code50)[which]
    _, L = _dims(code)
    line = _line(n, L, 17 * n)
    for name, t in threshold_sets().items():
        out, flips, runs, total, total_runs = abi.line_markov_host(code, line, n, KEY, first, t, total=11, total_runs=7, lib=lib)
        want, want_flips, want_runs, want_total, want_total_runs = lm.markov(line, KEY, first, t, L)
        assert out.shape == want.shape == (n, L // 32)
        assert out.tobytes() == want.tobytes(), name
        assert np.array_equal(flips, want_flips) and np.array_equal(runs, want_runs), name
        assert total == 11 + want_total and total_runs == 7 + want_total_runs, name


@pytest.mark.parametrize("which", ["50gpon", "small"])
def test_equal_thresholds_are_the_bsc_whatever_the_start(abi, lib, code50, which):
    """consequence 1: with t_idle == t_after the line, flips and total_flips are those of lnsfaid_line_bsc_host with that threshold"""
    code = _codes(abi, code50)[which]
    _, L = _dims(code)
    n = 3
    line = _line(n, L, 8)
    for threshold in (abi.line_bsc_threshold(0.01, lib), 2 ** 31):
        want, want_flips, want_total = abi.line_bsc_host(code, line, n, KEY, 5, threshold, total=3, lib=lib)
        for t_start in (0, threshold, 0xFFFFFFFF):
            out, flips, runs, total, _ = abi.line_markov_host(code, line, n, KEY, 5, [threshold, threshold, t_start], total=3, lib=lib)
            assert out.tobytes() == want.tobytes() and np.array_equal(flips, want_flips) and total == want_total, (threshold, t_start)
            assert np.array_equal(runs, lm.count_runs(np.unpackbits((out ^ line).view(np.uint8).reshape(n, -1), axis=1, bitorder="little")))


def test_all_or_nothing(abi, lib, code50):
    """consequence 2: with { 0, 0xFFFFFFFF, t_start } a codeword is untouched (s >= t_start) or inverted from position 0 on; the
    decision is the low half of draw L / 2 alone, and the next codeword starts afresh"""
    import line_link_ref as ll
    code = code50.code
    _, L = _dims(code)
    n = 24
    line = _line(n, L, 4)
    out, flips, runs, total, total_runs = abi.line_markov_host(code, line, n, KEY, 0, [0, 0xFFFFFFFF, 2 ** 31], lib=lib)
    s = ll.draw(KEY, ll.codeword_numbers(0, n), 2, np.array([L // 2]))[:, 0] & np.uint64(0xFFFFFFFF)
    hit = s < np.uint64(2 ** 31)
    assert hit.any() and not hit.all()  # both kinds among the 24, and a hit followed by a miss
    assert (hit[:-1] & ~hit[1:]).any()
    assert np.array_equal(out[~hit], line[~hit]) and np.array_equal(out[hit], ~line[hit])  # no u of these draws is 0xFFFFFFFF
    assert np.array_equal(flips, np.where(hit, L, 0)) and np.array_equal(runs, hit.astype(np.uint32))
    assert total == L * int(hit.sum()) and total_runs == int(hit.sum())
    # t_start 0: nothing ever starts; t_start 0xFFFFFFFF: everything does (s is not 0xFFFFFFFF here)
    assert np.array_equal(abi.line_markov_host(code, line, n, KEY, 0, [0, 0xFFFFFFFF, 0], lib=lib)[0], line)
    assert np.array_equal(abi.line_markov_host(code, line, n, KEY, 0, [0, 0xFFFFFFFF, 0xFFFFFFFF], lib=lib)[0], ~line)


@pytest.mark.parametrize("t_start", [0, 12345, 0xFFFFFFFF])
def test_zero_thresholds_copy_the_line(abi, lib, code50, t_start):
    """consequence 3"""
    code = code50.code
    _, L = _dims(code)
    line = _line(2, L, 6)
    out, flips, runs, total, total_runs = abi.line_markov_host(code, line, 2, KEY, 9, [0, 0, t_start], total=4, total_runs=5, lib=lib)
    assert np.array_equal(out, line) and not flips.any() and not runs.any() and (total, total_runs) == (4, 5)


@pytest.mark.parametrize("a,m,n", [(0, 1, 5), (7, 3, 5), (2 ** 32 + 5, 2, 4)])
def test_paging(abi, lib, code50, a, m, n):
    """two calls over [a, a + m) and [a + m, a + n) concatenate to the one-shot bytes, flips, runs and totals"""
    code = code50.code
    _, L = _dims(code)
    line = _line(n, L, 99)
    for name, t in threshold_sets().items():
        out, flips, runs, total, total_runs = abi.line_markov_host(code, line, n, KEY, a, t, lib=lib)
        o1, f1, r1, t1, tr1 = abi.line_markov_host(code, line[:m], m, KEY, a, t, lib=lib)
        o2, f2, r2, t2, tr2 = abi.line_markov_host(code, line[m:], n - m, KEY, a + m, t, total=t1, total_runs=tr1, lib=lib)
        assert np.array_equal(np.concatenate([o1, o2]), out) and np.array_equal(np.concatenate([f1, f2]), flips), name
        assert np.array_equal(np.concatenate([r1, r2]), runs) and (t2, tr2) == (total, total_runs), name


def test_threshold_helper(abi, lib):
    assert abi.line_markov_thresholds(0.01, 0.5, lib).tolist() == [21691754, 2147483648, 42949672]
    assert lm.thresholds(0.01, 0.5) == [21691754, 2147483648, 42949672]
    for p in (0.0, 0.01, 0.3):  # a == p: the BSC's threshold three times
        assert abi.line_markov_thresholds(p, p, lib).tolist() == [abi.line_bsc_threshold(p, lib)] * 3
    for p, a in ((0.0, 0.5), (0.005, 0.5), (0.01, 0.9), (0.03, 0.5), (0.012, 0.012000001), (0.2, 0.999)):
        t = abi.line_markov_thresholds(p, a, lib).tolist()
        assert t == lm.thresholds(p, a) and t[0] <= t[1] and t[2] == abi.line_bsc_threshold(p, lib), (p, a)


def test_threshold_helper_refusals(abi, lib):
    t = np.full(3, 123, np.uint32)
    nan = float("nan")
    for p, a in ((0.5, 0.01), (-0.1, 0.5), (0.01, 1.0), (1.0, 1.0), (0.01, 1.5), (nan, 0.5), (0.01, nan), (nan, nan), (0.01, float("inf"))):
        assert lib.lnsfaid_line_markov_thresholds(p, a, t.ctypes.data) == E_INVAL, (p, a)
        assert (t == 123).all()
        with pytest.raises(ValueError):
            abi.line_markov_thresholds(p, a, lib)
    assert lib.lnsfaid_line_markov_thresholds(0.01, 0.5, None) == E_INVAL


def test_statistics_of_the_helpers_chain(abi, lib, code50):
    """64 codewords through the helper's chain at (0.01, 0.5), host form.  The chain is stationary with P(e) = p and lag-one correlation
    rho = (a - p) / (1 - p), so the flips have mean n L p and variance n L p (1 - p) (1 + rho) / (1 - rho); they must lie within five
    standard deviations, and the mean run within the same relative width of 1 / (1 - a).  The key is fixed, so each figure is one
    number (the numpy prototype gave 11 124 flips in 5 590 runs, mean run 1.990; the bound is about +- 900 flips)."""
    code = code50.code
    _, L = _dims(code)
    n, p, a = 64, 0.01, 0.5
    t = abi.line_markov_thresholds(p, a, lib)
    line = _line(n, L, 1)
    out, flips, runs, total, total_runs = abi.line_markov_host(code, line, n, KEY, 0, t, lib=lib)
    rho = (a - p) / (1 - p)
    mean = n * L * p
    sigma = math.sqrt(n * L * p * (1 - p) * (1 + rho) / (1 - rho))
    mean_run = total / total_runs
    print("flips %d (mean %.1f, sigma %.1f), runs %d, mean run %.4f (1 / (1 - a) = %.4f)" % (total, mean, sigma, total_runs, mean_run, 1 / (1 - a)))
    assert total == int(flips.sum()) and total_runs == int(runs.sum())
    assert abs(total - mean) <= 5 * sigma, (total, mean, sigma)
    assert abs(mean_run - 1 / (1 - a)) <= 5 * sigma / mean * (1 / (1 - a)), (mean_run, 5 * sigma / mean)


def test_error_rules(abi, lib, code50):
    code = code50.code
    _, L = _dims(code)
    n = 2
    line = _line(n, L, 2).reshape(-1)
    out = np.full(n * L // 32, 0x5A5A5A5A, np.uint32)
    flips = np.full(n, 0x5A5A5A5A, np.uint32)
    runs = np.full(n, 0x5A5A5A5A, np.uint32)
    t = np.array(threshold_sets()["helper"], np.uint32)
    down = np.array([t[1] + 1, t[1], t[2]], np.uint32)
    total, total_runs = C.c_uint64(77), C.c_uint64(55)
    pc = C.byref(code)
    markov = lib.lnsfaid_line_markov_host
    good = (line.ctypes.data, n, KEY, 0, t.ctypes.data, out.ctypes.data, flips.ctypes.data, runs.ctypes.data, C.byref(total), C.byref(total_runs))
    assert markov(None, *good) == E_INVAL
    assert markov(pc, None, *good[1:]) == E_INVAL
    assert markov(pc, *good[:4], None, *good[5:]) == E_INVAL                 # t
    assert markov(pc, *good[:5], None, *good[6:]) == E_INVAL                 # line_out
    assert markov(pc, *good[:4], down.ctypes.data, *good[5:]) == E_INVAL     # t_idle > t_after
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16)):  # L or K not a multiple of 32
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert markov(C.byref(broken), *good) == E_INVAL, field

    def untouched():
        return (out == 0x5A5A5A5A).all() and (flips == 0x5A5A5A5A).all() and (runs == 0x5A5A5A5A).all() and (total.value, total_runs.value) == (77, 55)

    assert untouched()
    # n_codewords 0: a no-op, NULL buffers allowed
    assert markov(pc, None, 0, KEY, 0, None, None, None, None, None, None) == 0
    assert markov(pc, line.ctypes.data, 0, *good[2:]) == 0
    assert untouched()
    # exactly n codewords are written; each optional output may be NULL on its own; in place gives the same bytes
    want = lm.markov(line.reshape(n, -1), KEY, 0, t, L)
    wide = np.full((n + 1) * L // 32, 0x5A5A5A5A, np.uint32)
    for drop in (None, 6, 7, 8, 9):
        args = list(good)
        args[5] = wide.ctypes.data
        if drop is not None:
            args[drop] = None
        flips[:] = runs[:] = 0x5A5A5A5A
        total.value, total_runs.value = 77, 55
        wide[:] = 0x5A5A5A5A
        assert markov(pc, *args) == 0
        assert (wide[n * L // 32:] == 0x5A5A5A5A).all() and wide[:n * L // 32].tobytes() == want[0].tobytes(), drop
        assert np.array_equal(flips, want[1]) if drop != 6 else (flips == 0x5A5A5A5A).all()
        assert np.array_equal(runs, want[2]) if drop != 7 else (runs == 0x5A5A5A5A).all()
        assert total.value == 77 + (want[3] if drop != 8 else 0) and total_runs.value == 55 + (want[4] if drop != 9 else 0)
    inplace = line.copy()
    assert markov(pc, inplace.ctypes.data, n, KEY, 0, t.ctypes.data, inplace.ctypes.data, None, None, None, None) == 0
    assert inplace.tobytes() == want[0].tobytes()


def test_device_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(1 << 12, np.uint32)
    t = np.array([1, 2, 3], np.uint32)
    total, total_runs = C.c_uint64(0), C.c_uint64(0)
    p = buf.ctypes.data
    assert lib.lnsfaid_line_markov_device(None, p, 1, KEY, 0, t.ctypes.data, p, None, None, C.byref(total), C.byref(total_runs)) == E_INVAL
    assert lib.lnsfaid_line_markov_device(None, None, 0, KEY, 0, None, None, None, None, None, None) == E_INVAL
    assert not buf.any() and total.value == 0 and total_runs.value == 0


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
    """host/line_markov_selftest.cpp: the host form and the helper on heap buffers of exactly the documented sizes at odd addresses,
    built with the Makefile's $(SANITIZE) flags and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "line_markov_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "line_markov_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "line_markov_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_kernel_resources(tmp_path):
    """one kernel (a lane takes one word, so the alignment classes share it), no scratch, no spills, at most 64 VGPRs (eight waves per
    SIMD stay resident), no LDS and no barrier"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / "line_markov.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_line_markov.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {k: v for k, v in kernel_meta(text).items() if "lnsfaid_line_markov_kernel" in k}
    assert len(meta) == 1, sorted(meta)
    for name, (vgpr, spill, scratch) in meta.items():
        assert vgpr <= 64 and spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
    assert ".group_segment_fixed_size: 0" in text and "s_barrier" not in text


@pytest.mark.parametrize("args", [
    ["--ebn0", "4.2", "--propagation", "0.5", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--propagation", "1.0", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--propagation", "-0.1", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--propagation", "nan", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--propagation", "x", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
], ids=["propagation_with_ebn0", "one", "negative", "nan", "x"])
def test_line_sim_bad_arguments(tmp_path, args):
    """the usage line and status 2, before anything touches a GPU or writes a file"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert r.stderr.startswith("usage: ") and "--propagation" in r.stderr and r.stderr.count("\n") == 1
    assert not os.listdir(str(tmp_path))
