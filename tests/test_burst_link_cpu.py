"""Burst-format link without a GPU (include/lnsfaid.h "burst-format link"): the four host forms against the numpy
restatement (tests/burst_link_ref.py), against expand -> lnsfaid_line_*_host -> drop, against the line calls when nothing is shortened,
split invariance, the wrap of the codeword number, the constant channels, the error rules, the ABI surface, the stand-alone sanitizer
program, and the build-time properties of lnsfaid_burst_link.hip from a cross-compile for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import burst_link_ref as bl
import burst_ref as br
import line_soft_ref as ls
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL = -1
TAIL, HEAD = br.TAIL, br.HEAD
KEY = 0xB0257F0E5EED2026
NEW_SYMBOLS = {"lnsfaid_burst_payload_random_device": 7, "lnsfaid_burst_payload_random_host": 7, "lnsfaid_burst_bsc_device": 11,
               "lnsfaid_burst_bsc_host": 11, "lnsfaid_burst_soft_device": 11, "lnsfaid_burst_soft_host": 11,
               "lnsfaid_burst_count_errors_device": 10, "lnsfaid_burst_count_errors_host": 10}
BATCHES = [("cycle", 1), ("cycle", 33), ("burst", 33), ("cycle", 65), ("burst", 65)]
BATCH_IDS = ["one", "cycle33", "burst33", "cycle65", "burst65"]
WHERE = pytest.mark.parametrize("where", [TAIL, HEAD], ids=["tail", "head"])
BATCH = pytest.mark.parametrize("name,n", BATCHES, ids=BATCH_IDS)


def _dims(code50):
    N, K = code50.N, code50.K
    return N, K, N - code50.code.puncture_tail


def _line(n, L, s, seed):
    bits, _ = br.burst_words(n, 0, L, s)
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=bits // 32, dtype=np.uint64).astype(np.uint32)


def _table(code50):
    N, K, L = _dims(code50)
    return ls.awgn_table(ls.ebn0_sigma(4.2, K, L), ls.DEFAULT_SCALE)


# ---- the host forms against the numpy restatement ----
@WHERE
@BATCH
def test_payload_host_equals_numpy(abi, lib, code50, name, n, where):
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    got = abi.burst_payload_random_host(code50.code, KEY, 7, s, where, n, lib)
    assert got.size == br.burst_words(n, K, L, s)[1] // 32
    assert got.tobytes() == bl.payload(KEY, 7, s, where, K).tobytes()
    # the payload of codeword C is the line payload of C with the known words dropped
    full = abi.line_payload_random_host(code50.code, KEY, 7, n, lib)
    assert got.tobytes() == bl.drop_words(full, s, where, K, K).tobytes()


@WHERE
@BATCH
def test_bsc_host_equals_numpy_and_expand_run_drop(abi, lib, code50, name, n, where):
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    line = _line(n, L, s, 100 + n)
    threshold = abi.line_bsc_threshold(0.01, lib)
    out, flips, total = abi.burst_bsc_host(code50.code, line, s, where, n, KEY, 3, threshold, total=500, lib=lib)
    want, want_flips, want_total = bl.bsc(line, s, where, KEY, 3, threshold, K, L)
    assert out.tobytes() == want.tobytes() and np.array_equal(flips, want_flips) and total == 500 + want_total and want_total > 0
    # expand with anything in the known range, run the line call, drop the known words
    for fill in (0, 0xFFFFFFFF, 0x12345678):
        full = bl.expand_line(line, s, where, K, L, fill)
        full_out, full_flips, _ = abi.line_bsc_host(code50.code, full, n, KEY, 3, threshold, lib=lib)
        assert out.tobytes() == bl.drop_words(full_out, s, where, K, L).tobytes(), fill
        mask = full_out ^ full
        inside = np.array([int(np.unpackbits(mask[c, ~bl.kept_words(L, K, S, where)].view(np.uint8)).sum()) for c, S in enumerate(s)])
        assert np.array_equal(flips, full_flips - inside), fill
    # in place
    work = line.copy()
    same, flips2, _ = abi.burst_bsc_host(code50.code, work, s, where, n, KEY, 3, threshold, in_place=True, lib=lib)
    assert same is work and work.tobytes() == want.tobytes() and np.array_equal(flips2, want_flips)


@WHERE
@BATCH
def test_soft_host_equals_numpy_and_expand_run_drop(abi, lib, code50, name, n, where):
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    line = _line(n, L, s, 200 + n)
    table = _table(code50)
    out, flips, total = abi.burst_soft_host(code50.code, line, s, where, n, KEY, 11, table, total=9, lib=lib)
    want, want_flips, want_total = bl.soft(line, s, where, KEY, 11, table, K, L)
    assert out.size == br.burst_words(n, K, L, s)[0] // 2
    assert out.tobytes() == want.tobytes() and np.array_equal(flips, want_flips) and total == 9 + want_total and want_total > 0
    for fill in (0, 0xFFFFFFFF):
        full = bl.expand_line(line, s, where, K, L, fill)
        full_out, full_flips, _ = abi.line_soft_host(code50.code, full, n, KEY, 11, table, lib=lib)
        assert out.tobytes() == bl.drop_words(full_out, s, where, K, L, 16).tobytes(), fill
        level = ls.levels(full_out)
        bits = np.unpackbits(full.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
        wrong = (level > 0) != (bits == 1)
        inside = np.array([int(wrong[c, ~br.kept(L, K, S, where)].sum()) for c, S in enumerate(s)])
        assert np.array_equal(flips, full_flips - inside), fill


@BATCH
def test_counters_host_equal_numpy(abi, lib, code50, name, n):
    """planted streams; among them codewords with unsatisfied == 0 and short_ones > 0, which must count as failed"""
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    got, sent, stats, ones = bl.planted(s, K, 300 + n, abi.line_stats_dtype())
    if n >= 33:
        quiet = (stats["unsatisfied"] == 0) & (ones > 0)
        assert quiet.any() and ((stats["unsatisfied"] == 0) & (ones == 0) & (stats["corrected"] > 0)).any()
    host = abi.burst_count_errors_host
    assert host(code50.code, got, sent, stats, ones, s, n, True, True, True, lib) == tuple(bl.count(got, sent, stats, ones, s, K))
    assert host(code50.code, got, sent, stats, None, s, n, True, True, True, lib) == tuple(bl.count(got, sent, stats, None, s, K))
    assert host(code50.code, got, None, stats, ones, s, n, True, True, True, lib) == tuple(bl.count(got, None, stats, ones, s, K))
    e, f, v = host(code50.code, got, sent, None, None, s, n, True, None, None, lib)
    assert (e, f, v) == (bl.count(got, sent, None, None, s, K)[0], None, None)
    # ADDED to
    start = ([5, 6, 7, 8], [1, 0, 2, 0], [9, 9, 9, 9])
    want = [[a + b for a, b in zip(x, y)] for x, y in zip(start, bl.count(got, sent, stats, ones, s, K))]
    assert list(host(code50.code, got, sent, stats, ones, s, n, *start, lib=lib)) == want
    if n >= 33:  # short_ones changes the outcome: more failed codewords than unsatisfied ones
        with_ones, without = bl.count(got, sent, stats, ones, s, K), bl.count(got, sent, stats, None, s, K)
        assert with_ones[1][1] == without[1][1] + int(quiet.sum()) and with_ones[2][3] > without[2][3]


# ---- no shortening: the line calls, byte for byte ----
@WHERE
def test_no_shortening_is_the_line_calls(abi, lib, code50, where):
    N, K, L = _dims(code50)
    n = 33
    code = code50.code
    line = _line(n, L, np.zeros(n, np.uint32), 5)
    threshold = abi.line_bsc_threshold(0.02, lib)
    table = _table(code50)
    pay = abi.line_payload_random_host(code, KEY, 40, n, lib)
    bsc = abi.line_bsc_host(code, line, n, KEY, 40, threshold, lib=lib)
    soft = abi.line_soft_host(code, line, n, KEY, 40, table, lib=lib)
    got, sent, stats, ones = bl.planted(np.zeros(n, np.uint32), K, 6, abi.line_stats_dtype())
    cnt = abi.line_count_errors_host(code, got, sent, stats, n, True, True, True, lib)
    for s in (None, np.zeros(n, np.uint32)):
        assert abi.burst_payload_random_host(code, KEY, 40, s, where, n, lib).tobytes() == pay.tobytes()
        o, f, t = abi.burst_bsc_host(code, line, s, where, n, KEY, 40, threshold, lib=lib)
        assert o.tobytes() == bsc[0].tobytes() and np.array_equal(f, bsc[1]) and t == bsc[2]
        o, f, t = abi.burst_soft_host(code, line, s, where, n, KEY, 40, table, lib=lib)
        assert o.tobytes() == soft[0].tobytes() and np.array_equal(f, soft[1]) and t == soft[2]
        assert abi.burst_count_errors_host(code, got, sent, stats, None, s, n, True, True, True, lib) == cnt
        assert abi.burst_count_errors_host(code, got, sent, stats, np.zeros(n, np.uint32), s, n, True, True, True, lib) == cnt


# ---- split invariance and the wrap of the codeword number ----
@WHERE
@pytest.mark.parametrize("first", [0, 2 ** 64 - 3], ids=["first0", "wrap"])
def test_split_20_45_and_wrap(abi, lib, code50, where, first):
    N, K, L = _dims(code50)
    n, cut = 65, 20
    code = code50.code
    s = br.batch("cycle", n)
    line = _line(n, L, s, 8)
    threshold = abi.line_bsc_threshold(0.01, lib)
    table = _table(code50)
    second = (first + cut) % 2 ** 64
    lcut = br.burst_words(cut, K, L, s[:cut])[0] // 32
    pay = abi.burst_payload_random_host(code, KEY, first, s, where, n, lib)
    assert pay.tobytes() == bl.payload(KEY, first, s, where, K).tobytes()  # the restatement wraps C = first + i
    parts = [abi.burst_payload_random_host(code, KEY, first, s[:cut], where, cut, lib),
             abi.burst_payload_random_host(code, KEY, second, s[cut:], where, n - cut, lib)]
    assert np.concatenate(parts).tobytes() == pay.tobytes()
    o, f, t = abi.burst_bsc_host(code, line, s, where, n, KEY, first, threshold, lib=lib)
    assert o.tobytes() == bl.bsc(line, s, where, KEY, first, threshold, K, L)[0].tobytes()
    o1, f1, t1 = abi.burst_bsc_host(code, line[:lcut], s[:cut], where, cut, KEY, first, threshold, lib=lib)
    o2, f2, t2 = abi.burst_bsc_host(code, line[lcut:], s[cut:], where, n - cut, KEY, second, threshold, total=t1, lib=lib)
    assert np.concatenate([o1, o2]).tobytes() == o.tobytes() and np.array_equal(np.concatenate([f1, f2]), f) and t2 == t
    o, f, t = abi.burst_soft_host(code, line, s, where, n, KEY, first, table, lib=lib)
    o1, f1, t1 = abi.burst_soft_host(code, line[:lcut], s[:cut], where, cut, KEY, first, table, lib=lib)
    o2, f2, t2 = abi.burst_soft_host(code, line[lcut:], s[cut:], where, n - cut, KEY, second, table, total=t1, lib=lib)
    assert np.concatenate([o1, o2]).tobytes() == o.tobytes() and np.array_equal(np.concatenate([f1, f2]), f) and t2 == t
    if first:
        assert o.tobytes() == bl.soft(line, s, where, KEY, first, table, K, L)[0].tobytes()
    got, sent, stats, ones = bl.planted(s, K, 9, abi.line_stats_dtype())
    pcut = br.burst_words(cut, K, L, s[:cut])[1] // 32
    whole = abi.burst_count_errors_host(code, got, sent, stats, ones, s, n, True, True, True, lib)
    a = abi.burst_count_errors_host(code, got[:pcut], sent[:pcut], stats[:cut], ones[:cut], s[:cut], cut, True, True, True, lib)
    b = abi.burst_count_errors_host(code, got[pcut:], sent[pcut:], stats[cut:], ones[cut:], s[cut:], n - cut, *a, lib=lib)
    assert b == whole


def test_common_random_numbers(abi, lib, code50):
    """a sweep over S on one key sees the same noise on every position that survives"""
    N, K, L = _dims(code50)
    code = code50.code
    threshold = abi.line_bsc_threshold(0.01, lib)
    zero = np.zeros(L // 32, np.uint32)
    ref, _, _ = abi.line_bsc_host(code, zero, 1, KEY, 77, threshold, lib=lib)
    for where in (TAIL, HEAD):
        for S in br.SHORT:
            s = np.array([S], np.uint32)
            out, _, _ = abi.burst_bsc_host(code, np.zeros((L - S) // 32, np.uint32), s, where, 1, KEY, 77, threshold, lib=lib)
            assert out.tobytes() == ref.reshape(-1)[bl.kept_words(L, K, S, where)].tobytes(), (where, S)


# ---- the constant channels ----
@WHERE
def test_threshold_zero_copies_and_constant_tables(abi, lib, code50, where):
    N, K, L = _dims(code50)
    n = 33
    code = code50.code
    s = br.batch("cycle", n)
    line = _line(n, L, s, 12)
    out, flips, total = abi.burst_bsc_host(code, line, s, where, n, KEY, 0, 0, total=3, lib=lib)
    assert out.tobytes() == line.tobytes() and not flips.any() and total == 3
    bits = np.unpackbits(line.view(np.uint8), bitorder="little").astype(np.int64)
    per_cw = bl.split(bits, [L - int(S) for S in s])
    # every u >= 0: m = +7, level +7 for a 1 and -7 for a 0, no flips
    out, flips, total = abi.burst_soft_host(code, line, s, where, n, KEY, 0, [0] * 14, lib=lib)
    nib = np.where(bits == 1, 7, -7) & 15
    assert out.tobytes() == (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8).tobytes() and not flips.any() and total == 0
    # (almost) no u >= 2^32 - 1: m = -7, every position decided against its bit; a sent 0 at level +7 and a sent 1 at -7 both count
    out, flips, total = abi.burst_soft_host(code, line, s, where, n, KEY, 0, [0xFFFFFFFF] * 14, lib=lib)
    nib = np.where(bits == 1, -7, 7) & 15
    assert out.tobytes() == (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8).tobytes()
    assert np.array_equal(flips, [b.size for b in per_cw]) and total == bits.size


# ---- the rules ----
def test_error_rules(abi, lib, code50):
    """every refusal leaves the patterned outputs and the ADDED-to words untouched"""
    N, K, L = _dims(code50)
    code = code50.code
    n = 3
    good = np.array([0, 32, 256], np.uint32)
    line = np.full(n * L // 32, 0x5A5A5A5A, np.uint32)
    out = np.full(n * L // 32, 0x5A5A5A5A, np.uint32)
    llr4 = np.full(n * L // 2, 0x5A, np.uint8)
    payload = np.full(n * K // 32, 0x5A5A5A5A, np.uint32)
    flips = np.full(n, 0x5A5A5A5A, np.uint32)
    stats = np.zeros(n, abi.line_stats_dtype())
    ones = np.zeros(n, np.uint32)
    table = np.array(_table(code50), np.uint32)
    total = C.c_uint64(77)
    cnt = [(C.c_uint64 * 4)(1, 2, 3, 4) for _ in range(3)]
    pl, po, p4, pp, pf, pst, pon, ptab = (a.ctypes.data for a in (line, out, llr4, payload, flips, stats, ones, table))
    pay, bsc, soft, count = (lib.lnsfaid_burst_payload_random_host, lib.lnsfaid_burst_bsc_host, lib.lnsfaid_burst_soft_host,
                             lib.lnsfaid_burst_count_errors_host)
    cb, tb = C.byref(code), C.byref(total)

    def refused(ps, where, code_ref=cb):
        assert pay(code_ref, KEY, 0, ps, where, n, pp) == E_INVAL
        assert bsc(code_ref, pl, ps, where, n, KEY, 0, 5, po, pf, tb) == E_INVAL
        assert soft(code_ref, pl, ps, where, n, KEY, 0, ptab, p4, pf, tb) == E_INVAL

    for bad in (31, 33, 16, K, K + 32, 2 ** 32 - 32):  # S not a multiple of 32, S = K, S > K
        s = good.copy()
        s[1] = bad
        refused(s.ctypes.data, TAIL)
        refused(s.ctypes.data, HEAD)
        assert count(cb, pp, None, pst, pon, s.ctypes.data, n, *cnt) == E_INVAL, bad
    ps = good.ctypes.data
    for where in (2, -1, 99):
        refused(ps, where)
    refused(ps, TAIL, None)  # a NULL code
    assert count(None, pp, None, pst, pon, ps, n, *cnt) == E_INVAL
    broken = type(code)()
    C.memmove(C.byref(broken), C.byref(code), C.sizeof(code))
    broken.puncture_tail -= 8  # L no multiple of 32
    refused(ps, TAIL, C.byref(broken))
    assert count(C.byref(broken), pp, None, pst, pon, ps, n, *cnt) == E_INVAL
    # NULL required buffers
    assert pay(cb, KEY, 0, ps, TAIL, n, None) == E_INVAL
    assert bsc(cb, None, ps, TAIL, n, KEY, 0, 5, po, pf, tb) == E_INVAL
    assert bsc(cb, pl, ps, TAIL, n, KEY, 0, 5, None, pf, tb) == E_INVAL
    assert soft(cb, None, ps, TAIL, n, KEY, 0, ptab, p4, pf, tb) == E_INVAL
    assert soft(cb, pl, ps, TAIL, n, KEY, 0, ptab, None, pf, tb) == E_INVAL
    assert soft(cb, pl, ps, TAIL, n, KEY, 0, None, p4, pf, tb) == E_INVAL
    assert count(cb, None, pp, pst, pon, ps, n, *cnt) == E_INVAL
    # fec or vs_sent without stats
    assert count(cb, pp, None, None, pon, ps, n, cnt[0], cnt[1], None) == E_INVAL
    assert count(cb, pp, None, None, pon, ps, n, cnt[0], None, cnt[2]) == E_INVAL
    # a table that decreases
    down = table.copy()
    down[9] = down[8] - 1
    assert soft(cb, pl, ps, TAIL, n, KEY, 0, down.ctypes.data, p4, pf, tb) == E_INVAL
    # overlap of the soft channel's byte ranges: the input inside the output, and just behind its last byte is fine
    lbytes = (n * L - 288) // 8
    assert soft(cb, p4, ps, TAIL, n, KEY, 0, ptab, p4, pf, tb) == E_INVAL
    assert soft(cb, p4 + 4 * lbytes - 4, ps, TAIL, n, KEY, 0, ptab, p4, pf, tb) == E_INVAL
    assert soft(cb, p4, ps, TAIL, n, KEY, 0, ptab, p4 + lbytes - 1, pf, tb) == E_INVAL
    # n_codewords 0 is a no-op, with buffers or without
    assert pay(cb, KEY, 0, None, TAIL, 0, None) == 0 and pay(cb, KEY, 0, ps, HEAD, 0, pp) == 0
    assert bsc(cb, None, None, TAIL, 0, KEY, 0, 5, None, None, None) == 0 and bsc(cb, pl, ps, TAIL, 0, KEY, 0, 5, po, pf, tb) == 0
    assert soft(cb, None, None, TAIL, 0, KEY, 0, None, None, None, None) == 0 and soft(cb, pl, ps, TAIL, 0, KEY, 0, ptab, p4, pf, tb) == 0
    assert count(cb, None, None, None, None, None, 0, *cnt) == 0 and count(cb, pp, None, pst, pon, ps, 0, *cnt) == 0
    for a in (line, out, payload, flips):
        assert (a == 0x5A5A5A5A).all()
    assert (llr4 == 0x5A).all() and total.value == 77 and all(list(c) == [1, 2, 3, 4] for c in cnt)
    # and a good call right behind the input's last byte works and adds
    buf = np.zeros(5 * lbytes, np.uint8)
    assert soft(cb, buf.ctypes.data + 4 * lbytes, ps, TAIL, n, KEY, 0, ptab, buf.ctypes.data, pf, tb) == 0 and total.value > 77


def test_device_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    total = C.c_uint64(5)
    cnt = [(C.c_uint64 * 4)(1, 2, 3, 4) for _ in range(3)]
    for n in (0, 1):
        assert lib.lnsfaid_burst_payload_random_device(None, 1, 0, None, TAIL, n, p) == E_INVAL
        assert lib.lnsfaid_burst_bsc_device(None, p, None, TAIL, n, 1, 0, 5, p, None, C.byref(total)) == E_INVAL
        assert lib.lnsfaid_burst_soft_device(None, p, None, TAIL, n, 1, 0, p, p, None, C.byref(total)) == E_INVAL
        assert lib.lnsfaid_burst_count_errors_device(None, p, None, None, None, None, n, *cnt) == E_INVAL
    assert total.value == 5 and not buf.any() and all(list(c) == [1, 2, 3, 4] for c in cnt)


# ---- the ABI surface ----
_CTYPES = {"int32_t": C.c_int32, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}


def _header_prototype(name):
    header = open(os.path.join(ROOT, "include", "lnsfaid.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    types = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        array = arg.endswith("]")
        t = re.sub(r"\s*\b\w+(\[\d+\])?\s*$", "", arg).replace(" *", "*")
        types.append(t + "*" if array else t)
    return types


@pytest.mark.parametrize("name", sorted(NEW_SYMBOLS))
def test_abi_surface(abi, lib, name):
    assert getattr(lib, name) is not None
    res, args = abi.SYMBOLS[name]
    assert res is C.c_int
    want = []
    for t in _header_prototype(name):
        if t == "const lnsfaid_code*":
            want.append(C.POINTER(abi.Code))
        elif t == "uint64_t*":  # total_flips and the counter sets: host words the call adds to
            want.append(C.POINTER(C.c_uint64))
        elif t.endswith("*"):
            want.append(C.c_void_p)
        else:
            want.append(_CTYPES[t])
    assert args == want, (name, args, want)
    assert len(args) == NEW_SYMBOLS[name]


def test_methods(abi):
    for m in ("burst_payload_random_device", "burst_bsc_device", "burst_soft_device", "burst_count_errors_device"):
        assert callable(getattr(abi.Decoder, m))
    for f in ("burst_payload_random_host", "burst_bsc_host", "burst_soft_host", "burst_count_errors_host"):
        assert callable(getattr(abi, f))


def test_stand_alone_program_under_the_sanitizers():
    """host/burst_link_selftest.cpp: the host forms on heap buffers of exactly the documented sizes at odd addresses, built with the
    Makefile's $(SANITIZE) flags (address and undefined behaviour) against lnsfaid_tables.c and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "burst_link_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "burst_link_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "burst_link_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


_SIM = ["--codewords", "64", "--max-calls", "2", "--min-errors", "1"]


@pytest.mark.parametrize("args", [
    ["--ber", "0.005", "--burst-length", "4"],                                                  # --shorten missing
    ["--ber", "0.005", "--shorten", "288"],                                                     # --burst-length missing
    ["--ber", "0.005", "--where", "head"],
    ["--ber", "0.005", "--burst-length", "0", "--shorten", "288"],
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "288,"],
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "288,31"],                           # not a multiple of 32
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "14592"],                            # S = K
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "288", "--where", "middle"],
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "288", "--propagation", "0.1"],
    ["--ber", "0.005", "--burst-length", "4", "--shorten", "288", "--capture-failures", "8"],
    ["--ebn0", "4.2", "--burst-length", "4", "--shorten", "288", "--capture-failures", "8"],
], ids=lambda a: "_".join(a[2:]))
def test_line_sim_bad_burst_arguments(tmp_path, args):
    """the usage line and status 2, before anything touches a GPU or writes a file"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe] + args + _SIM, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert r.stderr.startswith("usage: ") and "--burst-length" in r.stderr and "--shorten" in r.stderr and r.stderr.count("\n") == 1
    assert not os.listdir(str(tmp_path))


# ---- build-time properties of the new kernel file ----
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_burst_link") / "lnsfaid_burst_link.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_burst_link.hip")], check=True, capture_output=True)
    return out.read_text()


def test_kernels_build_for_gfx950_without_scratch_or_spills(isa):
    """the five kernels (the soft channel twice: 16-byte and 4-byte stores), each without scratch and without spills, and few enough
    vector registers for eight waves per SIMD (at most 64)"""
    meta = {n: m for n, m in kernel_meta(isa).items() if "lnsfaid_burst_" in n}
    kinds = {k: [n for n in meta if "lnsfaid_burst_%s_kernel" % k in n] for k in ("payload", "bsc", "soft", "count")}
    assert {k: len(v) for k, v in kinds.items()} == {"payload": 1, "bsc": 1, "soft": 2, "count": 1}, sorted(meta)
    for name, (vgpr, spill, scratch) in meta.items():
        print(name, vgpr, spill, scratch)
        assert spill == 0 and scratch == 0 and vgpr <= 64, (name, vgpr, spill, scratch)


def test_makefile_links_the_new_object():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^liblnsfaid\.so:.*\blnsfaid_burst_link\.o\b", mk, flags=re.M)
    assert re.search(r"^lnsfaid_burst_link\.o: lnsfaid_burst_link\.hip\b", mk, flags=re.M)
