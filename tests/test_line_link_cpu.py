"""Line-format link without a GPU (include/lnsfaid.h "line-format link"): the host forms - the definition of what the
device calls return - byte for byte against the independent numpy restatement (tests/line_link_ref.py), paging, in-place use,
domain separation, the channel's rate at a fixed key, the counters on planted batches, the error rules, the stand-alone sanitizer
program, the driver's argument handling and the build-time properties of lnsfaid_line_link.hip from a cross-compile for gfx950."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_link_ref as ll
from test_line_cpu import _header_prototype
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL = -1
KEY = 0x5EED0F50C0DE2025
FIRSTS = [0, 7, 2 ** 32 + 5]
THRESHOLDS = [0, int(math.floor(0.005 * 2 ** 32)), 2 ** 31, 0xFFFFFFFF]
NEW_SYMBOLS = {"lnsfaid_line_payload_random_device": 5, "lnsfaid_line_payload_random_host": 5, "lnsfaid_line_bsc_threshold": 2,
               "lnsfaid_line_bsc_device": 9, "lnsfaid_line_bsc_host": 9, "lnsfaid_line_count_errors_device": 8,
               "lnsfaid_line_count_errors_host": 8}


def _small(abi):
    """a made-up shape, L = 96 and K = 32: one payload word per codeword, so the high half of its only draw is unused.  The host
    forms read nothing but these three numbers."""
    code = abi.Code()
    code.n_var, code.n_check, code.puncture_tail = 128, 96, 32
    return code


def _codes(abi, code50):
    return {"50gpon": code50.code, "small": _small(abi)}


def _dims(code):
    return code.n_var - code.n_check, code.n_var - code.puncture_tail


def _line(n, L, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(n, L // 32), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("which", ["50gpon", "small"])
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [1, 31, 33])
def test_payload_equals_the_numpy_reference(abi, lib, code50, which, first, n):
    code = _codes(abi, code50)[which]
    K, _ = _dims(code)
    got = abi.line_payload_random_host(code, KEY, first, n, lib)
    want = ll.payload(KEY, first, n, K)
    assert got.shape == want.shape == (n, K // 32)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("which", ["50gpon", "small"])
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [1, 31, 33])
def test_bsc_equals_the_numpy_reference(abi, lib, code50, which, first, n):
    code = _codes(abi, code50)[which]
    _, L = _dims(code)
    line = _line(n, L, 17 * n)
    for threshold in THRESHOLDS:
        out, flips, total = abi.line_bsc_host(code, line, n, KEY, first, threshold, total=11, lib=lib)
        want, want_flips, want_total = ll.bsc(line, KEY, first, threshold, L)
        assert out.tobytes() == want.tobytes(), threshold
        assert np.array_equal(flips, want_flips) and total == 11 + want_total, threshold


def test_codeword_number_wraps(abi, lib, code50):
    """C = first_codeword + i is a uint64 that wraps: the run over the wrap is the two runs on either side of it"""
    code = code50.code
    K, L = _dims(code)
    first = 2 ** 64 - 2
    pay = abi.line_payload_random_host(code, KEY, first, 4, lib)
    assert pay.tobytes() == ll.payload(KEY, first, 4, K).tobytes()
    assert np.array_equal(pay[2:], abi.line_payload_random_host(code, KEY, 0, 2, lib))
    line = _line(4, L, 3)
    out, flips, total = abi.line_bsc_host(code, line, 4, KEY, first, THRESHOLDS[1], lib=lib)
    assert out.tobytes() == ll.bsc(line, KEY, first, THRESHOLDS[1], L)[0].tobytes()


@pytest.mark.parametrize("a,m,n", [(0, 1, 33), (7, 16, 33), (2 ** 32 + 5, 32, 33), (5, 31, 31)])
def test_paging(abi, lib, code50, a, m, n):
    """two calls over [a, a + m) and [a + m, a + n) concatenate to the one-shot output"""
    code = code50.code
    _, L = _dims(code)
    whole = abi.line_payload_random_host(code, KEY, a, n, lib)
    parts = [abi.line_payload_random_host(code, KEY, a, m, lib), abi.line_payload_random_host(code, KEY, a + m, n - m, lib)]
    assert np.array_equal(np.concatenate(parts), whole)
    line = _line(n, L, 99)
    out, flips, total = abi.line_bsc_host(code, line, n, KEY, a, THRESHOLDS[1], lib=lib)
    o1, f1, t1 = abi.line_bsc_host(code, line[:m], m, KEY, a, THRESHOLDS[1], lib=lib)
    o2, f2, t2 = abi.line_bsc_host(code, line[m:], n - m, KEY, a + m, THRESHOLDS[1], total=t1, lib=lib)
    assert np.array_equal(np.concatenate([o1, o2]), out) and np.array_equal(np.concatenate([f1, f2]), flips) and t2 == total


def test_threshold_zero_and_in_place(abi, lib, code50):
    code = code50.code
    _, L = _dims(code)
    n = 5
    line = _line(n, L, 1)
    out, flips, total = abi.line_bsc_host(code, line, n, KEY, 3, 0, lib=lib)
    assert np.array_equal(out, line) and not flips.any() and total == 0
    want, want_flips, want_total = abi.line_bsc_host(code, line, n, KEY, 3, 2 ** 31, lib=lib)
    work = line.copy()
    same, flips, total = abi.line_bsc_host(code, work, n, KEY, 3, 2 ** 31, in_place=True, lib=lib)
    assert same is work and np.array_equal(work, want) and np.array_equal(flips, want_flips) and total == want_total
    assert not np.array_equal(want, line)


def test_payload_and_channel_draws_differ(abi, lib, code50):
    """domain separation: with threshold 2^31 the channel's flip mask is the top bit of every half draw; the payload's words of the
    same key, codeword and q must not be the numbers it was made from"""
    code = code50.code
    K, L = _dims(code)
    n = 4
    pay = abi.line_payload_random_host(code, KEY, 0, n, lib)
    out, _, _ = abi.line_bsc_host(code, np.zeros((n, L // 32), np.uint32), n, KEY, 0, 2 ** 31, lib=lib)
    mask = np.unpackbits(out.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :K // 32]  # one bit per half draw
    top_clear = (pay >> np.uint32(31)) == 0  # what the mask would be had the channel used the payload's draws
    agree = (mask.astype(bool) == top_clear).mean()
    assert 0.45 < agree < 0.55, agree
    assert not np.array_equal(ll.draw(KEY, ll.codeword_numbers(0, n), 1, np.arange(8)), ll.draw(KEY, ll.codeword_numbers(0, n), 2, np.arange(8)))


def test_rate_at_a_fixed_key(abi, lib, code50):
    """p = 0.01 over 96 codewords: n = 96 * 17 280 positions, mean n p = 16 589, sigma = sqrt(n p (1 - p)) = 128.  The key is fixed, so
    the count is one number; if it misses the 5 sigma band the generator is wrong, not the key."""
    code = code50.code
    _, L = _dims(code)
    n = 96
    threshold = abi.line_bsc_threshold(0.01, lib)
    out, flips, total = abi.line_bsc_host(code, np.zeros((n, L // 32), np.uint32), n, KEY, 0, threshold, lib=lib)
    positions = n * L
    p = threshold / 2 ** 32
    sigma = math.sqrt(positions * p * (1 - p))
    print("flips %d, mean %.1f, sigma %.1f" % (total, positions * p, sigma))
    assert abs(total - positions * p) < 5 * sigma
    assert int(flips.sum()) == total == int(np.unpackbits(out.view(np.uint8)).sum())
    # no codeword and no position class is left out: every codeword has flips, odd and even positions in equal measure
    assert flips.min() > 0
    bits = np.unpackbits(out.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
    even, odd = int(bits[:, 0::2].sum()), int(bits[:, 1::2].sum())
    assert abs(even - odd) < 5 * sigma


def test_bsc_threshold(abi, lib):
    assert abi.line_bsc_threshold(0.0, lib) == 0
    assert abi.line_bsc_threshold(0.01, lib) == int(math.floor(0.01 * 2 ** 32)) == 42949672
    assert abi.line_bsc_threshold(1 - 2.0 ** -32, lib) == 0xFFFFFFFF
    t = C.c_uint32(123)
    for p in (1.0, -0.0001, float("nan"), float("inf"), 2.0):
        assert lib.lnsfaid_line_bsc_threshold(p, C.byref(t)) == E_INVAL and t.value == 123, p
        with pytest.raises(ValueError):
            abi.line_bsc_threshold(p, lib)
    assert lib.lnsfaid_line_bsc_threshold(0.5, None) == E_INVAL


@pytest.mark.parametrize("which,n", [("50gpon", 41), ("50gpon", 1), ("small", 21)])
def test_counters_on_planted_batches(abi, lib, code50, which, n):
    code = _codes(abi, code50)[which]
    K, _ = _dims(code)
    got, sent, stats = ll.planted(n, K, 1000 + n, abi.line_stats_dtype())
    want = ll.count(got, sent, stats, K)
    assert want[0][0] == n and (n == 1 or (want[0][1] > 0 and want[0][3] > 0 and want[2][2] > 0 and want[2][3] > 0 and want[1][2] > 0))
    assert abi.line_count_errors_host(code, got, sent, stats, n, True, True, True, lib) == want
    # added to, not overwritten; each output on its own
    start = ([5, 6, 7, 8], [1, 0, 2, 0], [9, 9, 9, 9])
    added = abi.line_count_errors_host(code, got, sent, stats, n, *start, lib=lib)
    assert added == tuple([s + w for s, w in zip(st, wa)] for st, wa in zip(start, want))
    assert abi.line_count_errors_host(code, got, sent, stats, n, None, True, None, lib) == (None, want[1], None)
    assert abi.line_count_errors_host(code, got, sent, stats, n, None, None, True, lib) == (None, None, want[2])
    assert abi.line_count_errors_host(code, got, sent, None, n, True, None, None, lib) == (want[0], None, None)
    # NULL sent: the all-zero payload
    zero = ll.count(got, None, stats, K)
    assert abi.line_count_errors_host(code, got, None, stats, n, True, True, True, lib) == zero
    assert zero[0][2] == int(np.unpackbits(got.view(np.uint8)).sum())


def test_error_rules(abi, lib, code50):
    code = code50.code
    K, L = _dims(code)
    n = 2
    pay, line, out = np.full(n * K // 32, 0x5A5A5A5A, np.uint32), _line(n, L, 2).reshape(-1), np.full(n * L // 32, 0x5A5A5A5A, np.uint32)
    flips = np.full(n, 0x5A5A5A5A, np.uint32)
    stats = np.zeros(n, abi.line_stats_dtype())
    total = C.c_uint64(77)
    cnt = [(C.c_uint64 * 4)(1, 2, 3, 4) for _ in range(3)]
    pc = C.byref(code)
    payload, bsc, count = lib.lnsfaid_line_payload_random_host, lib.lnsfaid_line_bsc_host, lib.lnsfaid_line_count_errors_host
    assert payload(None, KEY, 0, n, pay.ctypes.data) == E_INVAL
    assert payload(pc, KEY, 0, n, None) == E_INVAL
    assert bsc(None, line.ctypes.data, n, KEY, 0, 5, out.ctypes.data, flips.ctypes.data, C.byref(total)) == E_INVAL
    assert bsc(pc, None, n, KEY, 0, 5, out.ctypes.data, flips.ctypes.data, C.byref(total)) == E_INVAL
    assert bsc(pc, line.ctypes.data, n, KEY, 0, 5, None, flips.ctypes.data, C.byref(total)) == E_INVAL
    assert count(None, pay.ctypes.data, None, stats.ctypes.data, n, *cnt) == E_INVAL
    assert count(pc, None, None, stats.ctypes.data, n, *cnt) == E_INVAL
    assert count(pc, pay.ctypes.data, None, None, n, cnt[0], cnt[1], None) == E_INVAL   # fec without stats
    assert count(pc, pay.ctypes.data, None, None, n, cnt[0], None, cnt[2]) == E_INVAL   # vs_sent without stats
    # L or K not a multiple of 32
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        pb = C.byref(broken)
        bad_k = field == "n_check"
        assert payload(pb, KEY, 0, n, pay.ctypes.data) == E_INVAL, field
        assert bsc(pb, line.ctypes.data, n, KEY, 0, 5, out.ctypes.data, flips.ctypes.data, C.byref(total)) == E_INVAL, field
        assert count(pb, pay.ctypes.data, None, stats.ctypes.data, n, *cnt) == E_INVAL, (field, bad_k)
    # nothing was written, nothing added
    assert (pay == 0x5A5A5A5A).all() and (out == 0x5A5A5A5A).all() and (flips == 0x5A5A5A5A).all() and total.value == 77
    assert all(list(c) == [1, 2, 3, 4] for c in cnt)
    # n_codewords 0: a no-op, NULL buffers allowed
    assert payload(pc, KEY, 0, 0, None) == 0 and bsc(pc, None, 0, KEY, 0, 5, None, None, None) == 0
    assert count(pc, None, None, None, 0, *cnt) == 0
    assert bsc(pc, line.ctypes.data, 0, KEY, 0, 5, out.ctypes.data, flips.ctypes.data, C.byref(total)) == 0
    assert (out == 0x5A5A5A5A).all() and (flips == 0x5A5A5A5A).all() and total.value == 77 and all(list(c) == [1, 2, 3, 4] for c in cnt)
    # and with the arguments right exactly n codewords of each output are written; the optional outputs may be NULL
    wide = np.full((n + 1) * L // 32, 0x5A5A5A5A, np.uint32)
    assert bsc(pc, line.ctypes.data, n, KEY, 0, 5, wide.ctypes.data, None, None) == 0
    assert (wide[n * L // 32:] == 0x5A5A5A5A).all() and np.array_equal(wide[:n * L // 32], line)  # threshold 5: no flip in 34 560 draws
    wide = np.full((n + 1) * K // 32, 0x5A5A5A5A, np.uint32)
    assert payload(pc, KEY, 0, n, wide.ctypes.data) == 0
    assert (wide[n * K // 32:] == 0x5A5A5A5A).all() and not (wide[:n * K // 32] == 0x5A5A5A5A).any()


def test_device_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(1 << 12, np.uint32)
    p = buf.ctypes.data
    cnt = (C.c_uint64 * 4)()
    total = C.c_uint64(0)
    assert lib.lnsfaid_line_payload_random_device(None, KEY, 0, 1, p) == E_INVAL
    assert lib.lnsfaid_line_bsc_device(None, p, 1, KEY, 0, 5, p, None, C.byref(total)) == E_INVAL
    assert lib.lnsfaid_line_count_errors_device(None, p, None, None, 1, cnt, None, None) == E_INVAL
    assert lib.lnsfaid_line_payload_random_device(None, KEY, 0, 0, None) == E_INVAL
    assert not buf.any() and total.value == 0 and list(cnt) == [0, 0, 0, 0]


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
        elif t == "uint32_t":
            assert a is C.c_uint32
        elif t == "size_t":
            assert a is C.c_size_t
        elif t == "double":
            assert a is C.c_double


def test_stand_alone_program_under_the_sanitizers():
    """host/line_link_selftest.cpp: the host forms on heap buffers of exactly the documented sizes at odd addresses, built with the
    Makefile's $(SANITIZE) flags and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "line_link_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "line_link_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "line_link_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("args", [
    [],
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "2"],                                   # --min-errors missing
    ["--ber", "1.0", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],               # not a probability below 1
    ["--ber", "0.01,", "--codewords", "96", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--codewords", "0", "--max-calls", "2", "--min-errors", "1"],
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "x", "--min-errors", "1"],
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "2", "--min-errors", "1", "--magnitude", "8"],
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "2", "--min-errors", "1", "--frobnicate"],
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "2", "--min-errors", "1", "--key"],
], ids=lambda a: "_".join(a[-2:]) or "none")
def test_line_sim_bad_arguments(tmp_path, args):
    """a bad or missing argument: the usage line and status 2, before anything touches a GPU or writes a file"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert r.stderr.startswith("usage: ") and "--ber" in r.stderr and r.stderr.count("\n") == 1
    assert not os.listdir(str(tmp_path))


# ---- build-time properties of the kernel file ----
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_line_link") / "lnsfaid_line_link.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_line_link.hip")], check=True, capture_output=True)
    return out.read_text()


def test_kernels_build_for_gfx950_without_scratch_or_spills(isa):
    """the nine instances (channel, payload source and counters, each at 1, 2 and 4 words per access), each without scratch and
    without spills, and few enough vector registers for eight waves per SIMD (at most 64)"""
    meta = {n: m for n, m in kernel_meta(isa).items() if "lnsfaid_line_" in n}
    kinds = {k: [n for n in meta if "lnsfaid_line_%s_kernel" % k in n] for k in ("bsc", "payload", "count")}
    assert {k: len(v) for k, v in kinds.items()} == {"bsc": 3, "payload": 3, "count": 3} and len(meta) == 9, sorted(meta)
    for name, (vgpr, spill, scratch) in meta.items():
        print(name, vgpr, spill, scratch)
        assert spill == 0 and scratch == 0 and vgpr <= 64, (name, vgpr, spill, scratch)
