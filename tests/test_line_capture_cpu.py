"""Line-format failure capture without a GPU (include/lnsfaid.h "line-format failure capture"): the host form - the
definition of what the device call returns - byte for byte against the numpy restatement (tests/line_capture_ref.py) on planted
batches, its agreement with the FEC status and the link's counters, paging, the error rules, the wrap of the codeword number, the
stand-alone sanitizer program and the driver's argument handling."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_capture_ref as lc
from test_line_cpu import _header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
NEW_SYMBOLS = {"lnsfaid_line_capture_words": 3, "lnsfaid_line_capture_device": 14, "lnsfaid_line_capture_host": 14}
FMTS = [lc.HARD, lc.LLR4]
FMT_IDS = ["hard", "llr4"]
# every kind of planted decision, the clean one in front, in the middle and at the end
KINDS = ["clean", "payload", "parity", "clean", "tail", "other", "alarm", "payload", "clean"]

_batches = {}


@pytest.fixture(scope="module")
def circ50(abi, lib, code50):
    return abi.code_parity_inverse(code50.code, lib)


def _batch(abi, lib, code50, circ50, fmt, kinds=KINDS, seed=7):
    """(line, bits, sent) of a planted batch, built once and never changed"""
    key = (fmt, tuple(kinds), seed)
    if key not in _batches:
        b = lc.planted(abi, lib, code50.code, circ50, kinds, fmt, seed)
        for a in b:
            a.setflags(write=False)
        _batches[key] = b
    return _batches[key]


def _same(got, want):
    found, rec, sec = got
    w_found, w_rec, w_pay = want
    assert found == w_found and len(rec) == len(w_rec)
    assert rec.tobytes() == w_rec.tobytes(), (rec.tolist(), w_rec.tolist())
    pay = np.concatenate([sec[k] for k in ("line", "bits", "error", "syndrome")], axis=1)
    assert pay.shape == w_pay.shape and pay.tobytes() == w_pay.tobytes()


def test_words_per_record(abi, lib, code50):
    assert abi.line_capture_words(code50.code, lc.HARD, lib) == lc.words(code50.code, lc.HARD) == 1740
    assert abi.line_capture_words(code50.code, lc.LLR4, lib) == lc.words(code50.code, lc.LLR4) == 3360
    assert abi.line_failure_dtype() == lc.RECORD and lc.RECORD.itemsize == 32


def test_the_planted_kinds_are_what_they_claim(abi, lib, code50, circ50):
    line, bits, sent = _batch(abi, lib, code50, circ50, lc.HARD)
    _, rec, _ = lc.capture(code50.code, line, lc.HARD, bits, sent, len(KINDS), select=3)
    by_index = {int(r["index"]): r for r in rec}
    assert sorted(by_index) == [i for i, k in enumerate(KINDS) if k != "clean"]
    for i, kind in enumerate(KINDS):
        if kind == "clean":
            continue
        r = by_index[i]
        assert (r["unsatisfied"] > 0) == (kind != "other"), kind
        assert (r["wrong_payload"] > 0) == (kind in ("payload", "other")), kind
        assert (r["wrong_parity"] > 0) == (kind in ("parity", "tail", "other", "alarm")), kind
        assert r["flags"] == {"payload": 3, "parity": 1, "tail": 1, "other": 2, "alarm": 1}[kind]


@pytest.mark.parametrize("with_line", [True, False], ids=["line", "noline"])
@pytest.mark.parametrize("select,with_sent", [(1, True), (2, True), (3, True), (1, False)], ids=["unc", "wrong", "both", "unc_nosent"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_host_form_equals_the_numpy_form(abi, lib, code50, circ50, fmt, select, with_sent, with_line):
    line, bits, sent = _batch(abi, lib, code50, circ50, fmt)
    n = len(KINDS)
    args = (line if with_line else None, fmt, bits, sent if with_sent else None, n)
    got = abi.line_capture_host(code50.code, *args, first_codeword=5, select=select, capacity=n, lib=lib)
    want = lc.capture(code50.code, *args, first=5, select=select, capacity=n)
    _same(got, want)
    found, rec, sec = got
    assert found == {1: 5, 2: 3, 3: 6}[select] and (rec["flags"] & select).all()
    if not with_line:
        assert not sec["line"].any() and not rec["channel_errors"].any()
    if not with_sent:
        assert not sec["error"].any() and not rec["wrong_payload"].any() and not rec["wrong_parity"].any() and not rec["channel_errors"].any()
    elif with_line:
        assert rec["channel_errors"].any()
    for r, e, s in zip(rec, sec["error"], sec["syndrome"]):
        assert len(abi.line_capture_positions(e)) == r["wrong_payload"] + r["wrong_parity"]
        assert len(abi.line_capture_positions(s)) == r["unsatisfied"]


def test_a_code_that_is_not_quasi_cyclic(abi, lib):
    """the host form reads pos_vn, deg and deg_rows row by row: 64 rows of degree 3 and 32 of degree 5 over 128 variable nodes"""
    rng = np.random.default_rng(3)
    pos = np.concatenate([rng.integers(0, 128, 64 * 3), rng.integers(0, 128, 32 * 5)]).astype(np.uint16)
    deg, deg_rows = (C.c_int32 * 2)(3, 5), (C.c_int32 * 2)(64, 32)
    code = abi.Code()
    code.n_var, code.n_check, code.puncture_tail, code.n_edges, code.z, code.nb_degres = 128, 96, 32, pos.size, 32, 2
    code.deg, code.deg_rows = C.cast(deg, C.POINTER(C.c_int32)), C.cast(deg_rows, C.POINTER(C.c_int32))
    code.pos_vn = pos.ctypes.data_as(C.POINTER(C.c_uint16))
    n = 12
    bits = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    bits[3] = 0
    sent = bits.copy()
    sent[5, 0] ^= 1
    sent[7, 3] ^= 0x80000000
    for fmt in FMTS:
        line = rng.integers(0, 256, (n, 96 // 2 if fmt == lc.LLR4 else 96 // 8), dtype=np.uint8)
        line = line if fmt == lc.LLR4 else line.view(np.uint32)
        for select in (1, 2, 3):
            _same(abi.line_capture_host(code, line, fmt, bits, sent, n, 0, select, 0, n, lib), lc.capture(code, line, fmt, bits, sent, n, 0, select, 0, n))
    found, rec, _ = abi.line_capture_host(code, None, lc.HARD, bits, sent, n, 0, 2, 0, n, lib)
    assert found == 1 and rec["index"].tolist() == [5] and rec["wrong_payload"].tolist() == [1]  # bit 127 of codeword 7 is parity


def test_syndrome_equals_the_fec_status_and_wrong_payload_the_counters(abi, lib, code50, circ50):
    kinds = [lc.KINDS[i % len(lc.KINDS)] for i in range(32)]
    line, bits, sent = _batch(abi, lib, code50, circ50, lc.HARD, kinds, 11)
    code = code50.code
    K = code50.K
    found, rec, sec = abi.line_capture_host(code, line, lc.HARD, bits, sent, 32, select=3, capacity=32, lib=lib)
    fec, _, _ = abi.fec_status_packed_host(code, None, bits, None, 1, lib=lib)
    pop = np.array([len(abi.line_capture_positions(s)) for s in sec["syndrome"]])
    assert np.array_equal(pop, fec["unsatisfied"][rec["index"]]) and np.array_equal(pop, rec["unsatisfied"])
    rest = np.setdiff1d(np.arange(32), rec["index"])
    assert not fec["unsatisfied"][rest].any() and found == 32 - len(rest) == sum(k != "clean" for k in kinds)
    errors, _, _ = abi.line_count_errors_host(code, bits[:, :K // 32], sent[:, :K // 32], None, 32, True, lib=lib)
    assert int(rec["wrong_payload"].sum()) == errors[2] and int((rec["wrong_payload"] > 0).sum()) == errors[1]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_paging(abi, lib, code50, circ50, fmt):
    """capacity 2 over 5 failures concatenates to the one-shot result; a skip beyond found stores 0; capacity 0 counts only"""
    line, bits, sent = _batch(abi, lib, code50, circ50, fmt)
    n = len(KINDS)
    host = lambda skip, cap: abi.line_capture_host(code50.code, line, fmt, bits, sent, n, 9, 1, skip, cap, lib)
    found, rec, sec = host(0, n)
    assert found == len(rec) == 5
    pages = [host(skip, 2) for skip in (0, 2, 4)]
    assert [p[0] for p in pages] == [5, 5, 5] and [len(p[1]) for p in pages] == [2, 2, 1]
    assert np.concatenate([p[1] for p in pages]).tobytes() == rec.tobytes()
    for name in sec:
        assert np.array_equal(np.concatenate([p[2][name] for p in pages]), sec[name])
    for skip in (5, 6, 2 ** 40):
        f, r, _ = host(skip, 2)
        assert f == 5 and len(r) == 0
    f, r, s = host(0, 0)
    assert f == 5 and len(r) == 0 and all(v.shape[0] == 0 for v in s.values())
    f, r, _ = host(1, 2 ** 40)  # a capacity beyond n_codewords
    assert f == 5 and r.tobytes() == rec[1:].tobytes()


def test_codeword_number_wraps(abi, lib, code50, circ50):
    line, bits, sent = _batch(abi, lib, code50, circ50, lc.HARD)
    n = len(KINDS)
    first = 2 ** 64 - 2
    _, rec, _ = abi.line_capture_host(code50.code, line, lc.HARD, bits, sent, n, first, 3, 0, n, lib)
    assert rec["index"].tolist() == [1, 2, 4, 5, 6, 7]
    assert rec["codeword"].tolist() == [(first + i) % 2 ** 64 for i in rec["index"].tolist()] == [2 ** 64 - 1, 0, 2, 3, 4, 5]
    _same((6, rec, abi.line_capture_host(code50.code, line, lc.HARD, bits, sent, n, first, 3, 0, n, lib)[2]),
          lc.capture(code50.code, line, lc.HARD, bits, sent, n, first, 3, 0, n))


def test_error_rules(abi, lib, code50, circ50):
    code = code50.code
    line, bits, sent = _batch(abi, lib, code50, circ50, lc.HARD)
    n = len(KINDS)
    W = lc.words(code, lc.HARD)
    rec = np.full(n * 8, 0x5A5A5A5A, np.uint32)
    pay = np.full(n * W, 0x5A5A5A5A, np.uint32)
    found, stored = C.c_uint64(77), C.c_uint64(78)
    pc = C.byref(code)
    host = lib.lnsfaid_line_capture_host
    # code, line, format, bits, sent, n, first, select, skip, capacity, records, payload, found, stored
    good = [pc, line.ctypes.data, lc.HARD, bits.ctypes.data, sent.ctypes.data, n, 0, 3, 0, n, rec.ctypes.data, pay.ctypes.data,
            C.byref(found), C.byref(stored)]

    def call(**change):
        names = ["code", "line", "format", "bits", "sent", "n", "first", "select", "skip", "capacity", "records", "payload", "found", "stored"]
        a = list(good)
        for k, v in change.items():
            a[names.index(k)] = v
        return host(*a)

    def untouched():
        return (rec == 0x5A5A5A5A).all() and (pay == 0x5A5A5A5A).all() and found.value == 77 and stored.value == 78

    assert call(code=None) == E_INVAL
    assert call(format=2) == E_INVAL and call(format=-1) == E_INVAL
    assert call(bits=None) == E_INVAL
    for select in (0, 4, -1, 7):
        assert call(select=select) == E_INVAL, select
    assert call(sent=None, select=2) == E_INVAL and call(sent=None, select=3) == E_INVAL  # WRONG needs a sent word
    assert call(records=None) == E_INVAL and call(payload=None) == E_INVAL
    assert call(found=None) == E_INVAL and call(stored=None) == E_INVAL
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16), ("n_var", code.n_var + 16)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert call(code=C.byref(broken)) == E_INVAL, field
        w = C.c_uint32(5)
        assert lib.lnsfaid_line_capture_words(C.byref(broken), lc.HARD, C.byref(w)) == E_INVAL and w.value == 5
    assert lib.lnsfaid_line_capture_words(pc, 2, C.byref(w)) == E_INVAL and lib.lnsfaid_line_capture_words(pc, lc.HARD, None) == E_INVAL
    assert lib.lnsfaid_line_capture_words(None, lc.HARD, C.byref(w)) == E_INVAL and w.value == 5
    assert untouched()
    # the device entry point refuses a NULL context before anything else
    assert lib.lnsfaid_line_capture_device(None, *good[1:]) == E_INVAL and untouched()
    # n_codewords 0: a no-op that sets both to 0, NULL buffers allowed
    assert call(n=0) == 0 and found.value == 0 and stored.value == 0 and (rec == 0x5A5A5A5A).all() and (pay == 0x5A5A5A5A).all()
    found.value, stored.value = 77, 78
    assert call(n=0, line=None, bits=None, sent=None, select=1, records=None, payload=None) == 0 and found.value == 0 and stored.value == 0
    # capacity 0 needs neither records nor payload; exactly `stored` records are written
    assert call(capacity=0, records=None, payload=None) == 0 and found.value == 6 and stored.value == 0
    assert call(capacity=2) == 0 and found.value == 6 and stored.value == 2
    assert (rec[2 * 8:] == 0x5A5A5A5A).all() and (pay[2 * W:] == 0x5A5A5A5A).all() and not (rec[:16] == 0x5A5A5A5A).all()


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
        elif t == "int32_t":
            assert a is C.c_int32
        elif t == "uint64_t*":
            assert a == C.POINTER(C.c_uint64)


def test_stand_alone_program_under_the_sanitizers():
    """host/line_capture_selftest.cpp: the host form on heap buffers of exactly the documented sizes at odd addresses, built with the
    Makefile's $(SANITIZE) flags and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "line_capture_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "line_capture_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "line_capture_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("args", [
    ["--ber", "0.01", "--codewords", "96", "--max-calls", "2", "--capture-file", "F.txt"],
    ["--ber", "0.01", "--codewords", "96", "--capture-failures", "x"],
    ["--ber", "0.01", "--codewords", "96", "--capture-failures", "0"],
    ["--ber", "0.01", "--codewords", "96", "--capture-failures"],
], ids=["file_without_capacity", "capacity_x", "capacity_0", "capacity_missing"])
def test_line_sim_bad_arguments(tmp_path, args):
    """the usage line and status 2, before anything touches a GPU or writes a file"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert r.stderr.startswith("usage: ") and "--capture-failures" in r.stderr and "--capture-file" in r.stderr and r.stderr.count("\n") == 1
    assert not os.listdir(str(tmp_path))
