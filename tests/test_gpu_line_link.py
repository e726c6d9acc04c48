"""Line-format link on the GPU (include/lnsfaid.h "line-format link", DESIGN.md §3.16, lnsfaid_line_link.hip).  The definition is the
host forms (tested against numpy in test_line_link_cpu.py); the device forms must return their bytes.  Every device output lies
between 64 guard words in front and 64 behind, which must keep their pattern after every call; `shift` words between the front guard
and the output put its base on 16, 8 or 4 bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_link_ref as ll

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32
MAX_GROUPS = 3
# All 96 codewords of this key from first_codeword 0 at p = 0.005 decode on the CPU port (DecodeMethod 2, 10 iterations, magnitude 4:
# each codeword of lnsfaid_line_to_llr4 of the host-form line as a group of 32 copies): 65 .. 110 flips per codeword, 8 360 in all,
# at most 4 iterations and no bit flipping.
KEY = 0x5EED0F50C0DE2025
SIM_KEY = 20261019  # the same check: 96 of 96, 8 226 flips
SHIFTS = {16: 0, 8: 2, 4: 1}  # base alignment in bytes -> words behind the front guard (torch's allocations start on 256 bytes)


def _words(code):
    return (code.n_var - code.n_check) // 32, (code.n_var - code.puncture_tail) // 32


def _guarded(torch, n_words, shift=0):
    t = torch.full((GUARD + shift + n_words + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 4 * (GUARD + shift)


def _inside(t, n_words, shift=0):
    """the words between the guards, after checking both guards"""
    h = t.cpu().numpy()
    assert (h[:GUARD + shift] == PATTERN).all() and (h[GUARD + shift + n_words:] == PATTERN).all(), "a guard word was overwritten"
    return h[GUARD + shift:GUARD + shift + n_words].view(np.uint32)


def _device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda()


@pytest.fixture(scope="module")
def dec(abi, code50):
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, MAX_GROUPS)
    yield d
    d.close()


@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96])
def test_payload_device_equals_host(abi, lib, code50, dec, n, first):
    import torch
    kw, _ = _words(code50.code)
    want = abi.line_payload_random_host(code50.code, KEY, first, n, lib)
    for align, shift in SHIFTS.items():
        extra = 2  # room for two more codewords: nothing past codeword n - 1 is written
        t, p = _guarded(torch, (n + extra) * kw, shift)
        assert p % align == 0 and (align == 16 or p % (2 * align) != 0)
        torch.cuda.synchronize()
        dec.line_payload_random_device(KEY, first, n, p)
        got = _inside(t, (n + extra) * kw, shift).reshape(n + extra, kw)
        assert np.array_equal(got[:n], want), align
        assert (got[n:].view(np.int32) == PATTERN).all(), align


@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96])
def test_bsc_device_equals_host(abi, lib, code50, dec, n, first):
    import torch
    _, lw = _words(code50.code)
    line = np.random.default_rng(n).integers(0, 2 ** 32, size=(n, lw), dtype=np.uint64).astype(np.uint32)
    for p_flip in (0.0, 0.005, 0.5):
        threshold = abi.line_bsc_threshold(p_flip, lib)
        want, want_flips, want_total = abi.line_bsc_host(code50.code, line, n, KEY, first, threshold, lib=lib)
        assert (p_flip > 0) == bool(want_total) and (p_flip > 0 or np.array_equal(want, line))
        for align, shift in SHIFTS.items():
            extra = 2
            d_in, p_in = _guarded(torch, n * lw, shift)
            d_in[GUARD + shift:GUARD + shift + n * lw] = _device(torch, line)
            d_out, p_out = _guarded(torch, (n + extra) * lw, shift)
            d_fl, p_fl = _guarded(torch, n + extra)
            torch.cuda.synchronize()
            total = dec.line_bsc_device(p_in, n, KEY, first, threshold, p_out, p_fl, total=1000)
            out = _inside(d_out, (n + extra) * lw, shift).reshape(n + extra, lw)
            flips = _inside(d_fl, n + extra)
            assert np.array_equal(out[:n], want), (p_flip, align)
            assert (out[n:].view(np.int32) == PATTERN).all() and (flips[n:].view(np.int32) == PATTERN).all(), (p_flip, align)
            assert np.array_equal(flips[:n], want_flips) and total == 1000 + want_total, (p_flip, align)
            assert np.array_equal(_inside(d_in, n * lw, shift).reshape(n, lw), line)  # a pure read of its input
            # in place, without the optional outputs
            assert lib.lnsfaid_line_bsc_device(dec.ctx, p_in, n, KEY, first, threshold, p_in, None, None) == 0
            assert np.array_equal(_inside(d_in, n * lw, shift).reshape(n, lw), want), (p_flip, align, "in place")


@pytest.mark.parametrize("n", [1, 41, 96])
def test_counters_device_equal_host(abi, lib, code50, dec, n):
    import torch
    K = code50.K
    kw, _ = _words(code50.code)
    got, sent, stats = ll.planted(n, K, 1000 + n, abi.line_stats_dtype())
    host = abi.line_count_errors_host
    for align, shift in SHIFTS.items():
        d_got, p_got = _guarded(torch, n * kw, shift)
        d_got[GUARD + shift:GUARD + shift + n * kw] = _device(torch, got)
        d_sent, p_sent = _guarded(torch, n * kw, shift)
        d_sent[GUARD + shift:GUARD + shift + n * kw] = _device(torch, sent)
        d_st = _device(torch, stats.view(np.int32))
        torch.cuda.synchronize()
        assert dec.line_count_errors_device(p_got, p_sent, d_st.data_ptr(), n, True, True, True) == host(code50.code, got, sent, stats, n, True, True, True, lib)
        start = ([5, 6, 7, 8], [1, 0, 2, 0], [9, 9, 9, 9])  # added to
        assert dec.line_count_errors_device(p_got, p_sent, d_st.data_ptr(), n, *start) == host(code50.code, got, sent, stats, n, *start, lib=lib)
        assert dec.line_count_errors_device(p_got, p_sent, None, n, True) == host(code50.code, got, sent, None, n, True, lib=lib)
        assert dec.line_count_errors_device(p_got, None, d_st.data_ptr(), n, True, True, True) == host(code50.code, got, None, stats, n, True, True, True, lib)
        assert dec.line_count_errors_device(p_got, p_sent, d_st.data_ptr(), n, None, None, True) == host(code50.code, got, sent, stats, n, None, None, True, lib)
        for t in (d_got, d_sent):  # pure reads
            _inside(t, n * kw, shift)


def _chain(abi, dec, n, key, first, threshold):
    """payload -> encode_line -> BSC in place -> decode_line (HARD, magnitude 4) on device buffers; returns what came back"""
    import torch
    kw, lw = _words(dec.code50.code)
    d_pay, p_pay = _guarded(torch, n * kw)
    d_line, p_line = _guarded(torch, n * lw)
    d_back, p_back = _guarded(torch, n * kw)
    d_st, p_st = _guarded(torch, n * 4)
    d_fl, p_fl = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.line_payload_random_device(key, first, n, p_pay)
    dec.encode_line_device(p_pay, n, p_line)
    total = dec.line_bsc_device(p_line, n, key, first, threshold, p_line, p_fl)
    dec.decode_line_device(p_line, abi.LINE_HARD, n, p_back, None, p_st, 4)
    counters = dec.line_count_errors_device(p_back, p_pay, p_st, n, True, True, True)
    r = {"payload": _inside(d_pay, n * kw).reshape(n, kw), "back": _inside(d_back, n * kw).reshape(n, kw),
         "stats": _inside(d_st, n * 4).view(abi.line_stats_dtype()), "flips": _inside(d_fl, n), "total": total, "counters": counters}
    _inside(d_line, n * lw)
    return r


def test_round_trip_below_the_correction_limit(abi, lib, code50, dec):
    """p = 0.005 at n = 96: everything decodes, and the decoder corrected exactly the positions the channel inverted.  No tolerance."""
    n = 96
    r = _chain(abi, dec, n, KEY, 0, abi.line_bsc_threshold(0.005, lib))
    errors, fec, vs = r["counters"]
    flips = r["flips"]
    assert np.array_equal(r["payload"], abi.line_payload_random_host(code50.code, KEY, 0, n, lib))
    assert int(flips.sum()) == r["total"] == 8360
    assert errors == [96, 0, 0, 0]
    assert fec == [96, 0, int((flips > 0).sum()), int(flips.sum())]
    assert vs == [96, 0, 0, 0]
    assert np.array_equal(r["stats"]["corrected"], flips.astype(np.int32))
    assert not r["stats"]["unsatisfied"].any() and np.array_equal(r["back"], r["payload"])


def test_round_trip_above_the_correction_limit(abi, lib, code50, dec):
    """p = 0.03, well above what the code corrects: error frames, and all twelve counters equal the host form on what came back"""
    n = 96
    r = _chain(abi, dec, n, KEY, 96, abi.line_bsc_threshold(0.03, lib))
    errors, fec, vs = r["counters"]
    assert errors[1] > 0
    assert (errors, fec, vs) == abi.line_count_errors_host(code50.code, r["back"], r["payload"], r["stats"], n, True, True, True, lib)
    assert errors[0] == fec[0] == vs[0] == n and vs[1] == errors[1]


def test_refusals(abi, lib, code50, dec):
    import torch
    n = 96
    kw, lw = _words(code50.code)
    d_pay, p_pay = _guarded(torch, (n + 1) * kw + 4)
    d_line, p_line = _guarded(torch, (n + 1) * lw + 4)
    d_fl, p_fl = _guarded(torch, n + 4)
    d_st = torch.zeros((n + 1) * 4 + 4, dtype=torch.int32, device="cuda")
    p_st = d_st.data_ptr()
    torch.cuda.synchronize()
    total = C.c_uint64(77)
    cnt = [(C.c_uint64 * 4)(1, 2, 3, 4) for _ in range(3)]
    payload, bsc, count = lib.lnsfaid_line_payload_random_device, lib.lnsfaid_line_bsc_device, lib.lnsfaid_line_count_errors_device

    def untouched():
        for t in (d_pay, d_line, d_fl):
            assert (t.cpu().numpy() == PATTERN).all()
        assert total.value == 77 and all(list(c) == [1, 2, 3, 4] for c in cnt)

    # more than 32 * max_groups codewords
    assert payload(dec.ctx, KEY, 0, 97, p_pay) == E_INVAL
    assert bsc(dec.ctx, p_line, 97, KEY, 0, 5, p_line, p_fl, C.byref(total)) == E_INVAL
    assert count(dec.ctx, p_pay, None, p_st, 97, *cnt) == E_INVAL
    # NULL required buffers
    assert payload(dec.ctx, KEY, 0, n, None) == E_INVAL
    assert bsc(dec.ctx, None, n, KEY, 0, 5, p_line, p_fl, C.byref(total)) == E_INVAL
    assert bsc(dec.ctx, p_line, n, KEY, 0, 5, None, p_fl, C.byref(total)) == E_INVAL
    assert count(dec.ctx, None, p_pay, p_st, n, *cnt) == E_INVAL
    # fec or vs_sent without stats
    assert count(dec.ctx, p_pay, None, None, n, cnt[0], cnt[1], None) == E_INVAL
    assert count(dec.ctx, p_pay, None, None, n, cnt[0], None, cnt[2]) == E_INVAL
    # a misaligned device pointer, each of them
    for off in (1, 2, 3):
        assert payload(dec.ctx, KEY, 0, n, p_pay + off) == E_INVAL
        assert bsc(dec.ctx, p_line + off, n, KEY, 0, 5, p_line, p_fl, C.byref(total)) == E_INVAL
        assert bsc(dec.ctx, p_line, n, KEY, 0, 5, p_line + off, p_fl, C.byref(total)) == E_INVAL
        assert bsc(dec.ctx, p_line, n, KEY, 0, 5, p_line, p_fl + off, C.byref(total)) == E_INVAL
        assert count(dec.ctx, p_pay + off, None, p_st, n, *cnt) == E_INVAL
        assert count(dec.ctx, p_pay, p_pay + off, p_st, n, *cnt) == E_INVAL
        assert count(dec.ctx, p_pay, None, p_st + off, n, *cnt) == E_INVAL
    # n_codewords 0: returns 0 and touches nothing, with buffers or without
    assert payload(dec.ctx, KEY, 0, 0, p_pay) == 0 and payload(dec.ctx, KEY, 0, 0, None) == 0
    assert bsc(dec.ctx, p_line, 0, KEY, 0, 5, p_line, p_fl, C.byref(total)) == 0 and bsc(dec.ctx, None, 0, KEY, 0, 5, None, None, None) == 0
    assert count(dec.ctx, p_pay, None, p_st, 0, *cnt) == 0 and count(dec.ctx, None, None, None, 0, *cnt) == 0
    untouched()
    # and the same context works once the arguments are right, also at a 4-byte offset: the accumulators start from zero
    assert payload(dec.ctx, KEY, 5, 1, p_pay + 4) == 0
    want = abi.line_payload_random_host(code50.code, KEY, 5, 1, lib)
    assert np.array_equal(_inside(d_pay, (n + 1) * kw + 4)[1:1 + kw], want[0])
    assert count(dec.ctx, p_pay + 4, None, p_st, 1, *cnt) == 0
    bits = int(np.unpackbits(want.view(np.uint8)).sum())
    assert [list(c) for c in cnt] == [[2, 3, 3 + bits, 4], [2, 2, 3, 4], [2, 3, 4, 4]]
    assert bsc(dec.ctx, p_pay + 4, 1, KEY, 5, 0, p_pay + 4, None, C.byref(total)) == 0 and total.value == 77


def _sim_rows(path):
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    return [{"threshold": int(r[1]), "codewords": int(r[2]), "flips": int(r[3]), "errors": [int(x) for x in r[5:9]],
             "fec": [int(x) for x in r[11:15]], "vs": [int(x) for x in r[15:19]]} for r in rows]


def test_line_sim_equals_the_same_chain_through_pyabi(abi, lib, code50, dec, tmp_path):
    """the driver's LineResult.txt against the same calls with the same key and first_codeword sequence: two points of two calls of
    96 codewords, first_codeword 0, 96, 192, 288"""
    n, calls = 96, 2
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, "--ber", "0.005,0.03", "--codewords", str(n), "--max-calls", str(calls),
                        "--min-errors", "1000", "--key", str(SIM_KEY)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = _sim_rows(str(tmp_path / "LineResult.txt"))
    assert len(rows) == 2 and [l for l in r.stdout.splitlines() if not l.startswith("#")] == \
        [l.rstrip("\n") for l in open(str(tmp_path / "LineResult.txt")) if not l.startswith("#")]
    first = 0
    for row, p in zip(rows, (0.005, 0.03)):
        threshold = abi.line_bsc_threshold(p, lib)
        errors, fec, vs, flips = [0] * 4, [0] * 4, [0] * 4, 0
        for _ in range(calls):
            c = _chain(abi, dec, n, SIM_KEY, first, threshold)
            errors, fec, vs = ([a + b for a, b in zip(acc, new)] for acc, new in zip((errors, fec, vs), c["counters"]))
            flips += c["total"]
            first += n
        assert row == {"threshold": threshold, "codewords": calls * n, "flips": flips, "errors": errors, "fec": fec, "vs": vs}, p
    assert rows[0]["errors"][0] == rows[1]["errors"][0] == calls * n and rows[1]["errors"][1] > 0
