"""Line-format failure capture on the GPU (include/lnsfaid.h "line-format failure capture", DESIGN.md §3.19, lnsfaid_line_capture.hip).
The definition is the host form (tested against numpy in test_line_capture_cpu.py); the device form must return its bytes.  Device
inputs lie between 64 guard words and must be unchanged after every call; `shift` words behind the front guard put their bases on 16,
8 or 4 bytes.  The host outputs lie between 64 guard words too, and nothing past `stored` records may be written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_capture_ref as lc
from test_gpu_line_link import GUARD, PATTERN, SHIFTS, _guarded, _inside

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
MAX_GROUPS = 3
# End to end: of the 96 codewords of this key from first_codeword 0 behind a BSC of p = 0.014, 22 fail on the CPU port (DecodeMethod 2,
# 10 iterations, magnitude 4: each codeword of lnsfaid_line_to_llr4 of the host-form line as a group of 32 copies; 23 115 flips in
# all).  All 22 are uncorrectable and wrong; the first are 3, 4, 10, 11, 14 with 570, 593, 61, 294, 298 unsatisfied rows.
KEY, P_FLIP, FAILURES = 0x5EED0F50C0DE2025, 0.014, 22
SIM_KEY, SIM_FAILURES = 20261019, 33  # the same prediction for the driver's key: 33 of 96, 23 284 flips
FMTS = [lc.HARD, lc.LLR4]
FMT_IDS = ["hard", "llr4"]

_batches = {}


@pytest.fixture(scope="module")
def circ50(abi, lib, code50):
    return abi.code_parity_inverse(code50.code, lib)


@pytest.fixture(scope="module")
def dec(abi, code50):
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, MAX_GROUPS)
    yield d
    d.close()


def _kinds(n, which):
    failing = lc.KINDS[1:]
    if which == "none":
        return ["clean"] * n
    if which == "all":
        return [failing[i % len(failing)] for i in range(n)]
    return [failing[i % len(failing)] if i in (0, 31, 32, n - 1) else "clean" for i in range(n)]  # "edges"


def _batch(abi, lib, code50, circ50, n, which, fmt):
    """(line, bits, sent), built once per key and never changed"""
    key = (n, which, fmt)
    if key not in _batches:
        b = lc.planted(abi, lib, code50.code, circ50, _kinds(n, which), fmt, 100 * n + fmt)
        for a in b:
            a.setflags(write=False)
        _batches[key] = b
    return _batches[key]


def _upload(torch, a, shift):
    """a host array (or None) in a guarded device buffer: (tensor, pointer, words)"""
    if a is None:
        return None, None, 0
    w = np.ascontiguousarray(a).view(np.int32).reshape(-1)
    t, p = _guarded(torch, w.size, shift)
    t[GUARD + shift:GUARD + shift + w.size] = torch.from_numpy(w.copy()).cuda()
    return t, p, w.size


def _capture(abi, lib, dec, ptrs, fmt, n, first, select, skip, capacity):
    """lnsfaid_line_capture_device into guarded host buffers of min(capacity, n) slots; checks the guards and that nothing past
    `stored` was written; returns (found, records, sections)"""
    code = dec.code50.code
    W = lc.words(code, fmt)
    slots = min(capacity, n)
    rec = np.full(GUARD + slots * 8 + GUARD, PATTERN, np.int32)
    pay = np.full(GUARD + slots * W + GUARD, PATTERN, np.int32)
    found, stored = C.c_uint64(12345), C.c_uint64(12345)
    rc = lib.lnsfaid_line_capture_device(dec.ctx, ptrs[0], fmt, ptrs[1], ptrs[2], n, first, select, skip, capacity,
                                         rec.ctypes.data + 4 * GUARD, pay.ctypes.data + 4 * GUARD, C.byref(found), C.byref(stored))
    assert rc == 0, (rc, lib.lnsfaid_last_hip_error())
    s = stored.value
    assert s <= slots
    assert (rec[:GUARD] == PATTERN).all() and (rec[GUARD + 8 * s:] == PATTERN).all(), "records: a word outside `stored` was written"
    assert (pay[:GUARD] == PATTERN).all() and (pay[GUARD + W * s:] == PATTERN).all(), "payload: a word outside `stored` was written"
    records = rec[GUARD:GUARD + 8 * s].copy().view(abi.line_failure_dtype())
    payload = pay[GUARD:GUARD + W * s].copy().view(np.uint32).reshape(s, W)
    return found.value, records, abi.line_capture_split(code, fmt, payload)


def _same(got, want):
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes(), (got[0], want[0], got[1].tolist(), want[1].tolist())
    for name in ("line", "bits", "error", "syndrome"):
        assert got[2][name].shape == want[2][name].shape and np.array_equal(got[2][name], want[2][name]), name


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("which", ["edges", "all", "none"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96])
def test_device_equals_host(abi, lib, code50, circ50, dec, n, which, fmt):
    import torch
    code = code50.code
    line, bits, sent = _batch(abi, lib, code50, circ50, n, which, fmt)
    first = 2 ** 64 - 17
    for align, shift in SHIFTS.items():
        ups = [_upload(torch, a, shift) for a in (line, bits, sent)]
        assert all(p % align == 0 and (align == 16 or p % (2 * align) != 0) for _, p, _ in ups)
        torch.cuda.synchronize()
        ptrs = [p for _, p, _ in ups]
        cases = [(ptrs, (line, bits, sent), 3), (ptrs, (line, bits, sent), 1), (ptrs, (line, bits, sent), 2),
                 ([ptrs[0], ptrs[1], None], (line, bits, None), 1), ([None, ptrs[1], ptrs[2]], (None, bits, sent), 3)]
        for dev, host, select in cases:
            got = _capture(abi, lib, dec, dev, fmt, n, first, select, 0, n)
            want = abi.line_capture_host(code, host[0], fmt, host[1], host[2], n, first, select, 0, n, lib)
            _same(got, want)
            if select == 3 and host[2] is not None:
                assert got[0] == {"edges": len({0, 31, 32, n - 1} & set(range(n))), "all": n, "none": 0}[which]
        for (t, _, w), a in zip(ups, (line, bits, sent)):  # a pure read of its inputs
            assert np.array_equal(_inside(t, w, shift), np.ascontiguousarray(a).view(np.uint32).reshape(-1)), align


@pytest.fixture(scope="module")
def carry(abi, code50):
    """n = 1027 on a context of 33 groups: the rank kernel's second chunk starts at codeword 1024.  The sent word is the all-zero
    codeword, the decisions are its flips; (bits with failures at 0, 1023, 1024 and 1026; bits with every codeword failing; sent)"""
    n, nw = 1027, code50.N // 32
    sent = np.zeros((n, nw), np.uint32)
    few = np.zeros((n, nw), np.uint32)
    for i, (w, b) in zip((0, 1023, 1024, 1026), ((0, 0), (455, 31), (456, 0), (551, 31))):  # payload, payload, parity, tail
        few[i, w] = np.uint32(1 << b)
    every = np.zeros((n, nw), np.uint32)
    every[np.arange(n), np.arange(n) % nw] = np.uint32(1) << (np.arange(n) % 32).astype(np.uint32)
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, 33)
    yield d, few, every, sent
    d.close()


def test_rank_carry_across_chunks(abi, lib, code50, carry):
    import torch
    dec33, few, every, sent = carry
    code = code50.code
    n = 1027
    d_sent = _upload(torch, sent, 0)
    d_few = _upload(torch, few, 0)
    d_every = _upload(torch, every, 0)
    torch.cuda.synchronize()
    got = _capture(abi, lib, dec33, [None, d_few[1], d_sent[1]], lc.HARD, n, 5, 3, 0, 16)
    _same(got, abi.line_capture_host(code, None, lc.HARD, few, sent, n, 5, 3, 0, 16, lib))
    assert got[0] == 4 and got[1]["index"].tolist() == [0, 1023, 1024, 1026] and got[1]["flags"].tolist() == [3, 3, 1, 1]
    got = _capture(abi, lib, dec33, [None, d_every[1], d_sent[1]], lc.HARD, n, 5, 3, 1020, 8)
    _same(got, abi.line_capture_host(code, None, lc.HARD, every, sent, n, 5, 3, 1020, 8, lib))
    assert got[0] == 1027 and got[1]["index"].tolist() == list(range(1020, 1027))
    got = _capture(abi, lib, dec33, [None, d_every[1], d_sent[1]], lc.HARD, n, 5, 2, 1022, 3)  # across the chunk boundary
    assert got[1]["index"].tolist() == [i for i in range(n) if i % 552 < 456][1022:1025]
    # more codewords than the context holds
    f, s = C.c_uint64(7), C.c_uint64(7)
    assert lib.lnsfaid_line_capture_device(dec33.ctx, None, lc.HARD, d_every[1], d_sent[1], 33 * 32 + 1, 0, 1, 0, 0, None, None, C.byref(f),
                                           C.byref(s)) == E_INVAL and f.value == s.value == 7


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_paging_on_the_device(abi, lib, code50, circ50, dec, fmt):
    """pages of 7 concatenate to the one-shot host result; a skip beyond found stores nothing; capacity 0 counts only"""
    import torch
    n = 33
    line, bits, sent = _batch(abi, lib, code50, circ50, n, "all", fmt)
    ups = [_upload(torch, a, 0) for a in (line, bits, sent)]
    ptrs = [p for _, p, _ in ups]
    torch.cuda.synchronize()
    want = abi.line_capture_host(code50.code, line, fmt, bits, sent, n, 0, 3, 0, n, lib)
    assert want[0] == n
    pages = [_capture(abi, lib, dec, ptrs, fmt, n, 0, 3, skip, 7) for skip in range(0, n, 7)]
    assert [p[0] for p in pages] == [n] * 5 and [len(p[1]) for p in pages] == [7, 7, 7, 7, 5]
    _same((n, np.concatenate([p[1] for p in pages]), {k: np.concatenate([p[2][k] for p in pages]) for k in want[2]}), want)
    for skip in (n, n + 1, 2 ** 40):
        f, r, _ = _capture(abi, lib, dec, ptrs, fmt, n, 0, 3, skip, 7)
        assert f == n and len(r) == 0
    f, r, _ = _capture(abi, lib, dec, ptrs, fmt, n, 0, 3, 0, 0)
    assert f == n and len(r) == 0
    _same(dec.line_capture_device(ptrs[0], fmt, ptrs[1], ptrs[2], n, 0, 3, 30, 2 ** 40), abi.line_capture_host(code50.code, line, fmt, bits, sent, n, 0, 3, 30, n, lib))


def test_refusals(abi, lib, code50, circ50, dec):
    import torch
    n = 33
    fmt = lc.HARD
    line, bits, sent = _batch(abi, lib, code50, circ50, n, "all", fmt)
    ups = [_upload(torch, a, 0) for a in (line, bits, sent)]
    p_line, p_bits, p_sent = [p for _, p, _ in ups]
    torch.cuda.synchronize()
    W = lc.words(code50.code, fmt)
    rec = np.full(n * 8, PATTERN, np.int32)
    pay = np.full(n * W, PATTERN, np.int32)
    found, stored = C.c_uint64(77), C.c_uint64(78)
    names = ["line", "format", "bits", "sent", "n", "first", "select", "skip", "capacity", "records", "payload", "found", "stored"]
    good = [p_line, fmt, p_bits, p_sent, n, 0, 3, 0, n, rec.ctypes.data, pay.ctypes.data, C.byref(found), C.byref(stored)]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[names.index(k)] = v
        return lib.lnsfaid_line_capture_device(dec.ctx, *a)

    assert call(n=32 * MAX_GROUPS + 1) == E_INVAL
    assert call(format=2) == E_INVAL and call(bits=None) == E_INVAL
    assert call(select=0) == E_INVAL and call(select=4) == E_INVAL
    assert call(sent=None, select=2) == E_INVAL and call(sent=None, select=3) == E_INVAL
    assert call(records=None) == E_INVAL and call(payload=None) == E_INVAL and call(found=None) == E_INVAL and call(stored=None) == E_INVAL
    for off in (1, 2, 3):
        assert call(line=p_line + off) == E_INVAL and call(bits=p_bits + off) == E_INVAL and call(sent=p_sent + off) == E_INVAL
    assert (rec == PATTERN).all() and (pay == PATTERN).all() and found.value == 77 and stored.value == 78
    assert call(n=0) == 0 and found.value == 0 and stored.value == 0 and (rec == PATTERN).all() and (pay == PATTERN).all()
    # and the same context works once the arguments are right
    assert call(capacity=2) == 0 and found.value == n and stored.value == 2 and (rec[16:] == PATTERN).all() and (pay[2 * W:] == PATTERN).all()


def test_end_to_end_with_the_real_decoder(abi, lib, code50, dec):
    """payload -> encode_line (with bits) -> BSC -> decode_line (HARD, magnitude 4, with bits and stats) -> capture, select 3"""
    import torch
    code = code50.code
    n = 96
    N, K, L = lc.dims(code)
    threshold = abi.line_bsc_threshold(P_FLIP, lib)
    d_pay, p_pay = _guarded(torch, n * K // 32)
    d_line, p_line = _guarded(torch, n * L // 32)
    d_sent, p_sent = _guarded(torch, n * N // 32)
    d_back, p_back = _guarded(torch, n * K // 32)
    d_bits, p_bits = _guarded(torch, n * N // 32)
    d_st, p_st = _guarded(torch, n * 4)
    torch.cuda.synchronize()
    dec.line_payload_random_device(KEY, 0, n, p_pay)
    dec.encode_line_device(p_pay, n, p_line, p_sent)
    dec.line_bsc_device(p_line, n, KEY, 0, threshold, p_line)
    dec.decode_line_device(p_line, abi.LINE_HARD, n, p_back, p_bits, p_st, 4)
    found, rec, sec = dec.line_capture_device(p_line, abi.LINE_HARD, p_bits, p_sent, n, 0, 3, 0, n)
    stats = _inside(d_st, n * 4).view(abi.line_stats_dtype())
    back, pay = _inside(d_back, n * K // 32).reshape(n, -1), _inside(d_pay, n * K // 32).reshape(n, -1)
    print("found", found, "indices", rec["index"].tolist(), "unsatisfied", rec["unsatisfied"].tolist())
    assert found == len(rec) == FAILURES
    idx = rec["index"].astype(np.int64)
    assert np.array_equal(rec["unsatisfied"], stats["unsatisfied"][idx].astype(np.uint32))
    assert idx.tolist() == np.flatnonzero((stats["unsatisfied"] > 0) | (back != pay).any(axis=1)).tolist()
    assert np.array_equal(rec["codeword"], idx.astype(np.uint64))
    # one record replayed on the host from (key, codeword) alone
    r = len(rec) // 2
    cw = int(rec["codeword"][r])
    payload = abi.line_payload_random_host(code, KEY, cw, 1, lib)
    line, word = abi.encode_line_host(code, payload, 1, True, lib)
    rx, flips, _ = abi.line_bsc_host(code, line, 1, KEY, cw, threshold, lib=lib)
    assert np.array_equal(sec["line"][r], rx[0]) and np.array_equal(sec["bits"][r] ^ sec["error"][r], word[0])
    assert rec["channel_errors"][r] == flips[0]
    assert len(abi.line_capture_positions(sec["error"][r])) == rec["wrong_payload"][r] + rec["wrong_parity"][r]
    assert len(abi.line_capture_positions(sec["syndrome"][r])) == rec["unsatisfied"][r]
    # and the whole result is the host form's on what came back
    _same((found, rec, sec), abi.line_capture_host(code, _inside(d_line, n * L // 32), abi.LINE_HARD, _inside(d_bits, n * N // 32),
                                                   _inside(d_sent, n * N // 32), n, 0, 3, 0, n, lib))


def _result_rows(path):
    """the rows of LineResult.txt without their last column, the wall-clock seconds of the run"""
    return [l.split()[:-1] for l in open(path) if l.strip() and not l.startswith("#")]


def test_line_sim_capture(tmp_path):
    """the driver with --capture-failures 4: one row per failure, paged four at a time; LineResult.txt is that of the run without the
    option (every column but the last, the seconds the run took)"""
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    args = ["--ber", str(P_FLIP), "--codewords", "96", "--max-calls", "1", "--min-errors", "1000", "--key", str(SIM_KEY)]
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    for d, extra in ((with_dir, ["--capture-failures", "4"]), (without_dir, [])):
        d.mkdir()
        r = subprocess.run(["timeout", "-k", "10", "120", exe] + args + extra, capture_output=True, text=True, cwd=str(d))
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert sorted(os.listdir(str(without_dir))) == ["LineResult.txt"] and sorted(os.listdir(str(with_dir))) == ["LineFailures.txt", "LineResult.txt"]
    rows = _result_rows(str(with_dir / "LineResult.txt"))
    assert rows == _result_rows(str(without_dir / "LineResult.txt")) and len(rows) == 1
    comments = lambda p: [l for l in open(p) if l.startswith("#")]
    assert comments(str(with_dir / "LineResult.txt")) == comments(str(without_dir / "LineResult.txt"))
    vs = [int(x) for x in rows[0][15:19]]
    failures = [l.rstrip("\n") for l in open(str(with_dir / "LineFailures.txt")) if not l.startswith("#")]
    assert len(failures) == vs[1] + vs[3] == SIM_FAILURES
    last = -1
    for l in failures:
        head, positions, unsat_rows = [part.split() for part in l.split(" ;")]
        x, codeword, index, flags, unsatisfied, wrong_payload, wrong_parity, channel_errors = head
        assert float(x) == P_FLIP and int(codeword) == int(index) > last and int(flags) in (1, 2, 3)
        last = int(index)
        assert len(positions) == int(wrong_payload) + int(wrong_parity) and len(unsat_rows) == int(unsatisfied)
        assert positions == sorted(positions, key=int) and unsat_rows == sorted(unsat_rows, key=int)
        assert int(channel_errors) > 0


def test_line_sim_capture_file_needs_capture_failures(tmp_path):
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run([exe, "--ber", "0.014", "--codewords", "96", "--max-calls", "1", "--min-errors", "1000", "--capture-file", "F.txt"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stderr.startswith("usage: ") and not os.listdir(str(tmp_path))
