"""Burst-format link on the GPU (include/lnsfaid.h "burst-format link", DESIGN.md §3.22, lnsfaid_burst_link.hip).  The definition is the
host forms (tested against numpy in test_burst_link_cpu.py); the device forms must return their bytes.  Every device output lies
between 64 guard words in front and 64 behind, which must keep their pattern after every call, and is compared word for word, so
every word inside has been written; `shift` words between the front guard and the buffer put its base 0, 4 or 8 bytes off a 16-byte
boundary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import burst_link_ref as bl
import burst_ref as br
import line_soft_ref as ls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32
MAX_GROUPS = 3
TAIL, HEAD = br.TAIL, br.HEAD
HARD, LLR4 = br.HARD, br.LLR4
# The 65 codewords of this key from first_codeword 0 in the "cycle" batch decode on the CPU port under oracle/ (lnsfaid_cpu_decode,
# DecodeMethod 2, 10 iterations, on lnsfaid_burst_to_llr4 of the host forms' output: payload -> lnsfaid_encode_burst_host -> channel):
# every one of the 65 whole mother codewords comes back, for TAIL and for HEAD.
#   BSC at lnsfaid_line_bsc_threshold(0.005), HARD at magnitude 4: 11 .. 123 flips per codeword (TAIL, 4 455 in all; HEAD 12 .. 125,
#     4 448), 3, 4 and 3 iterations per group, no bit-flipping iteration;
#   soft channel at Eb/N0 4.2 dB, scale 13 / sqrt 2, LLR4: 44 .. 398 flips (TAIL, 17 742 in all; HEAD 45 .. 398, 17 840), 4 iterations
#     per group, no bit-flipping iteration.
KEY = 0xB0257F0E5EED2026
# The driver's run: 128 codewords of this key as bursts of 4, the last shortened by 288 and 14 560 in turn, at p = 0.005 and magnitude 4:
# the same check returns 128 of 128 mother codewords (TAIL; 6 .. 109 flips per codeword, 10 126 in all), and 128 of 128 for the same
# codewords unshortened (62 .. 116 flips, 11 382 in all).
SIM_KEY = 20261020
SHIFTS = (0, 1, 2)  # words behind the front guard: 0, 4 and 8 bytes off a 16-byte boundary (torch's allocations start on 256 bytes)
BATCHES = [("cycle", 1), ("cycle", 33), ("burst", 33), ("cycle", 65), ("burst", 65)]
BATCH_IDS = ["one", "cycle33", "burst33", "cycle65", "burst65"]
WHERE = pytest.mark.parametrize("where", [TAIL, HEAD], ids=["tail", "head"])
BATCH = pytest.mark.parametrize("name,n", BATCHES, ids=BATCH_IDS)


def _dims(code50):
    N, K = code50.N, code50.K
    return N, K, N - code50.code.puncture_tail


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


def _filled(torch, a, shift=0):
    """a guarded device copy of the words of `a`"""
    words = np.ascontiguousarray(a).view(np.uint32).reshape(-1)
    t, p = _guarded(torch, words.size, shift)
    t[GUARD + shift:GUARD + shift + words.size] = _device(torch, words)
    return t, p


def _line(n, L, s, seed):
    bits, _ = br.burst_words(n, 0, L, s)
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=bits // 32, dtype=np.uint64).astype(np.uint32)


def _table(abi, lib, code50, db=4.2):
    N, K, L = _dims(code50)
    return abi.line_awgn_table(ls.ebn0_sigma(db, K, L), ls.DEFAULT_SCALE, lib)


@pytest.fixture(scope="module")
def dec(abi, code50):
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, MAX_GROUPS)
    yield d
    d.close()


# ---- device form = host form, byte for byte ----
@WHERE
@BATCH
def test_payload_device_equals_host(abi, lib, code50, dec, name, n, where):
    import torch
    s = br.batch(name, n)
    for first in (0, 2 ** 64 - 3):
        want = abi.burst_payload_random_host(code50.code, KEY, first, s, where, n, lib)
        for shift in SHIFTS:
            t, p = _guarded(torch, want.size, shift)
            assert p % 16 == 4 * shift
            torch.cuda.synchronize()
            dec.burst_payload_random_device(KEY, first, s, where, n, p)
            assert np.array_equal(_inside(t, want.size, shift), want), (first, shift)


@WHERE
@BATCH
def test_bsc_device_equals_host(abi, lib, code50, dec, name, n, where):
    import torch
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    line = _line(n, L, s, 100 + n)
    for p_flip in (0.005, 0.5):
        threshold = abi.line_bsc_threshold(p_flip, lib)
        want, want_flips, want_total = abi.burst_bsc_host(code50.code, line, s, where, n, KEY, 9, threshold, lib=lib)
        for shift in SHIFTS:
            d_in, p_in = _filled(torch, line, shift)
            d_out, p_out = _guarded(torch, line.size, shift)
            d_fl, p_fl = _guarded(torch, n)
            torch.cuda.synchronize()
            total = dec.burst_bsc_device(p_in, s, where, n, KEY, 9, threshold, p_out, p_fl, total=1000)
            assert np.array_equal(_inside(d_out, line.size, shift), want), (p_flip, shift)
            assert np.array_equal(_inside(d_fl, n), want_flips) and total == 1000 + want_total, (p_flip, shift)
            assert np.array_equal(_inside(d_in, line.size, shift), line)  # a pure read of its input
            # in place equals out of place, without the optional outputs
            assert lib.lnsfaid_burst_bsc_device(dec.ctx, p_in, s.ctypes.data, where, n, KEY, 9, threshold, p_in, None, None) == 0
            assert np.array_equal(_inside(d_in, line.size, shift), want), (p_flip, shift, "in place")


@WHERE
@BATCH
def test_soft_device_equals_host(abi, lib, code50, dec, name, n, where):
    import torch
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    line = _line(n, L, s, 200 + n)
    table = _table(abi, lib, code50)
    want, want_flips, want_total = abi.burst_soft_host(code50.code, line, s, where, n, KEY, 5, table, lib=lib)
    for shift in SHIFTS:
        d_in, p_in = _filled(torch, line, shift)
        d_out, p_out = _guarded(torch, 4 * line.size, shift)
        d_fl, p_fl = _guarded(torch, n)
        torch.cuda.synchronize()
        total = dec.burst_soft_device(p_in, s, where, n, KEY, 5, table, p_out, p_fl, total=7)
        assert _inside(d_out, 4 * line.size, shift).tobytes() == want.tobytes(), shift
        assert np.array_equal(_inside(d_fl, n), want_flips) and total == 7 + want_total, shift
        assert np.array_equal(_inside(d_in, line.size, shift), line)
        # without the optional outputs: the same bytes, nothing else touched
        d_out2, p_out2 = _guarded(torch, 4 * line.size, shift)
        torch.cuda.synchronize()
        assert lib.lnsfaid_burst_soft_device(dec.ctx, p_in, s.ctypes.data, where, n, KEY, 5, table.ctypes.data, p_out2, None, None) == 0
        assert _inside(d_out2, 4 * line.size, shift).tobytes() == want.tobytes(), shift
        assert np.array_equal(_inside(d_fl, n), want_flips)


@BATCH
def test_counters_device_equal_host(abi, lib, code50, dec, name, n):
    import torch
    N, K, L = _dims(code50)
    s = br.batch(name, n)
    got, sent, stats, ones = bl.planted(s, K, 300 + n, abi.line_stats_dtype())
    host = abi.burst_count_errors_host
    code = code50.code
    for shift in SHIFTS:
        d_got, p_got = _filled(torch, got, shift)
        d_sent, p_sent = _filled(torch, sent, shift)
        d_st, p_st = _filled(torch, stats, shift)
        d_on, p_on = _filled(torch, ones, shift)
        torch.cuda.synchronize()
        dev = dec.burst_count_errors_device
        assert dev(p_got, p_sent, p_st, p_on, s, n, True, True, True) == host(code, got, sent, stats, ones, s, n, True, True, True, lib)
        start = ([5, 6, 7, 8], [1, 0, 2, 0], [9, 9, 9, 9])  # added to
        assert dev(p_got, p_sent, p_st, p_on, s, n, *start) == host(code, got, sent, stats, ones, s, n, *start, lib=lib)
        assert dev(p_got, p_sent, p_st, None, s, n, True, True, True) == host(code, got, sent, stats, None, s, n, True, True, True, lib)
        assert dev(p_got, None, p_st, p_on, s, n, True, True, True) == host(code, got, None, stats, ones, s, n, True, True, True, lib)
        assert dev(p_got, p_sent, None, None, s, n, True) == host(code, got, sent, None, None, s, n, True, lib=lib)
        assert dev(p_got, p_sent, p_st, p_on, s, n, None, None, True) == host(code, got, sent, stats, ones, s, n, None, None, True, lib)
        for t, a in ((d_got, got), (d_sent, sent), (d_st, stats), (d_on, ones)):  # pure reads
            assert _inside(t, a.view(np.uint32).size, shift).tobytes() == a.tobytes()


# ---- no shortening: the line calls on the device ----
@WHERE
def test_no_shortening_is_the_line_device_calls(abi, lib, code50, dec, where):
    import torch
    N, K, L = _dims(code50)
    n = 65
    kw, lw = K // 32, L // 32
    line = _line(n, L, np.zeros(n, np.uint32), 5)
    threshold = abi.line_bsc_threshold(0.02, lib)
    table = _table(abi, lib, code50)
    got, sent, stats, _ = bl.planted(np.zeros(n, np.uint32), K, 6, abi.line_stats_dtype())
    d_in, p_in = _filled(torch, line)
    d_got, p_got = _filled(torch, got)
    d_sent, p_sent = _filled(torch, sent)
    d_st, p_st = _filled(torch, stats)
    d_zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    bufs = {k: _guarded(torch, w) for k, w in (("pay", n * kw), ("bsc", n * lw), ("soft", 4 * n * lw), ("fl", n), ("sfl", n))}
    torch.cuda.synchronize()
    dec.line_payload_random_device(KEY, 40, n, bufs["pay"][1])
    t_bsc = dec.line_bsc_device(p_in, n, KEY, 40, threshold, bufs["bsc"][1], bufs["fl"][1])
    t_soft = dec.line_soft_device(p_in, n, KEY, 40, table, bufs["soft"][1], bufs["sfl"][1])
    cnt = dec.line_count_errors_device(p_got, p_sent, p_st, n, True, True, True)
    want = {k: _inside(t, t.numel() - 2 * GUARD).copy() for k, (t, _) in bufs.items()}
    for s in (None, np.zeros(n, np.uint32)):
        mine = {k: _guarded(torch, want[k].size) for k in bufs}
        torch.cuda.synchronize()
        dec.burst_payload_random_device(KEY, 40, s, where, n, mine["pay"][1])
        assert dec.burst_bsc_device(p_in, s, where, n, KEY, 40, threshold, mine["bsc"][1], mine["fl"][1]) == t_bsc
        assert dec.burst_soft_device(p_in, s, where, n, KEY, 40, table, mine["soft"][1], mine["sfl"][1]) == t_soft
        for k, (t, _) in mine.items():
            assert np.array_equal(_inside(t, want[k].size), want[k]), k
        assert dec.burst_count_errors_device(p_got, p_sent, p_st, None, s, n, True, True, True) == cnt
        assert dec.burst_count_errors_device(p_got, p_sent, p_st, d_zero.data_ptr(), s, n, True, True, True) == cnt


# ---- one call of 65 equals calls of 20 + 45 ----
@WHERE
def test_split_20_45(abi, lib, code50, dec, where):
    import torch
    N, K, L = _dims(code50)
    n, cut, first = 65, 20, 2 ** 64 - 7  # the codeword number wraps inside the second call
    second = (first + cut) % 2 ** 64
    s = br.batch("cycle", n)
    line = _line(n, L, s, 8)
    threshold = abi.line_bsc_threshold(0.01, lib)
    table = _table(abi, lib, code50)
    lcut = br.burst_words(cut, K, L, s[:cut])[0] // 32
    pcut = br.burst_words(cut, K, L, s[:cut])[1] // 32
    pwords = br.burst_words(n, K, L, s)[1] // 32
    got, sent, stats, ones = bl.planted(s, K, 9, abi.line_stats_dtype())
    d_in, p_in = _filled(torch, line)
    d_got, p_got = _filled(torch, got)
    d_sent, p_sent = _filled(torch, sent)
    d_st, p_st = _filled(torch, stats)
    d_on, p_on = _filled(torch, ones)
    one = {k: _guarded(torch, w) for k, w in (("pay", pwords), ("bsc", line.size), ("soft", 4 * line.size), ("fl", n), ("sfl", n))}
    two = {k: _guarded(torch, t.numel() - 2 * GUARD) for k, (t, _) in one.items()}
    torch.cuda.synchronize()
    dec.burst_payload_random_device(KEY, first, s, where, n, one["pay"][1])
    t_bsc = dec.burst_bsc_device(p_in, s, where, n, KEY, first, threshold, one["bsc"][1], one["fl"][1])
    t_soft = dec.burst_soft_device(p_in, s, where, n, KEY, first, table, one["soft"][1], one["sfl"][1])
    cnt = dec.burst_count_errors_device(p_got, p_sent, p_st, p_on, s, n, True, True, True)
    assert cnt == abi.burst_count_errors_host(code50.code, got, sent, stats, ones, s, n, True, True, True, lib)
    a, b = (s[:cut], cut, first, 0, 0, 0), (s[cut:], n - cut, second, pcut, lcut, cut)
    tb, ts, c = 0, 0, (True, True, True)
    for sh, m, f, po, lo, co in (a, b):
        dec.burst_payload_random_device(KEY, f, sh, where, m, two["pay"][1] + 4 * po)
        tb = dec.burst_bsc_device(p_in + 4 * lo, sh, where, m, KEY, f, threshold, two["bsc"][1] + 4 * lo, two["fl"][1] + 4 * co, total=tb)
        ts = dec.burst_soft_device(p_in + 4 * lo, sh, where, m, KEY, f, table, two["soft"][1] + 16 * lo, two["sfl"][1] + 4 * co, total=ts)
        c = dec.burst_count_errors_device(p_got + 4 * po, p_sent + 4 * po, p_st + 16 * co, p_on + 4 * co, sh, m, *c)
    assert (tb, ts, c) == (t_bsc, t_soft, cnt)
    for k in one:
        words = one[k][0].numel() - 2 * GUARD
        assert np.array_equal(_inside(two[k][0], words), _inside(one[k][0], words)), k
    assert np.array_equal(_inside(one["pay"][0], pwords), abi.burst_payload_random_host(code50.code, KEY, first, s, where, n, lib))


# ---- the rules ----
def test_refusals(abi, lib, code50, dec):
    """every refusal leaves the device outputs and the ADDED-to words untouched; the same context then serves a good call"""
    import torch
    N, K, L = _dims(code50)
    n = 33
    s = br.batch("cycle", n)
    ps = s.ctypes.data
    kw, lw = K // 32, L // 32
    d_pay, p_pay = _guarded(torch, n * kw + 4)
    d_line, p_line = _guarded(torch, n * lw + 4)
    d_llr4, p_llr4 = _guarded(torch, 4 * n * lw + 4)
    d_fl, p_fl = _guarded(torch, n + 4)
    d_st = torch.zeros(n * 4 + 4, dtype=torch.int32, device="cuda")
    d_on = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    p_st, p_on = d_st.data_ptr(), d_on.data_ptr()
    torch.cuda.synchronize()
    table = _table(abi, lib, code50)
    ptab = table.ctypes.data
    total = C.c_uint64(77)
    tb = C.byref(total)
    cnt = [(C.c_uint64 * 4)(1, 2, 3, 4) for _ in range(3)]
    pay, bsc, soft, count = (lib.lnsfaid_burst_payload_random_device, lib.lnsfaid_burst_bsc_device, lib.lnsfaid_burst_soft_device,
                             lib.lnsfaid_burst_count_errors_device)
    ctx = dec.ctx

    def all_refuse(shortened, where, m):
        assert pay(ctx, KEY, 0, shortened, where, m, p_pay) == E_INVAL
        assert bsc(ctx, p_line, shortened, where, m, KEY, 0, 5, p_line, p_fl, tb) == E_INVAL
        assert soft(ctx, p_line, shortened, where, m, KEY, 0, ptab, p_llr4, p_fl, tb) == E_INVAL

    # more than 32 * max_groups codewords
    all_refuse(None, TAIL, 97)
    assert count(ctx, p_pay, None, p_st, p_on, None, 97, *cnt) == E_INVAL
    # a bad `shortened` entry, a bad `where`
    for bad in (31, 33, K, K + 32, 2 ** 32 - 32):
        b = s.copy()
        b[n - 1] = bad
        all_refuse(b.ctypes.data, TAIL, n)
        all_refuse(b.ctypes.data, HEAD, n)
        assert count(ctx, p_pay, None, p_st, p_on, b.ctypes.data, n, *cnt) == E_INVAL
    for where in (2, -1):
        all_refuse(ps, where, n)
        all_refuse(None, where, 0)
    # NULL required buffers
    assert pay(ctx, KEY, 0, ps, TAIL, n, None) == E_INVAL
    assert bsc(ctx, None, ps, TAIL, n, KEY, 0, 5, p_line, p_fl, tb) == E_INVAL
    assert bsc(ctx, p_line, ps, TAIL, n, KEY, 0, 5, None, p_fl, tb) == E_INVAL
    assert soft(ctx, None, ps, TAIL, n, KEY, 0, ptab, p_llr4, p_fl, tb) == E_INVAL
    assert soft(ctx, p_line, ps, TAIL, n, KEY, 0, ptab, None, p_fl, tb) == E_INVAL
    assert soft(ctx, p_line, ps, TAIL, n, KEY, 0, None, p_llr4, p_fl, tb) == E_INVAL
    assert count(ctx, None, p_pay, p_st, p_on, ps, n, *cnt) == E_INVAL
    # fec or vs_sent without stats
    assert count(ctx, p_pay, None, None, p_on, ps, n, cnt[0], cnt[1], None) == E_INVAL
    assert count(ctx, p_pay, None, None, p_on, ps, n, cnt[0], None, cnt[2]) == E_INVAL
    # a table that decreases; overlapping ranges of the soft channel
    down = table.copy()
    down[9] = down[8] - 1
    assert soft(ctx, p_line, ps, TAIL, n, KEY, 0, down.ctypes.data, p_llr4, p_fl, tb) == E_INVAL
    lwords = br.burst_words(n, K, L, s)[0] // 32
    assert soft(ctx, p_llr4, ps, TAIL, n, KEY, 0, ptab, p_llr4, p_fl, tb) == E_INVAL
    assert soft(ctx, p_llr4 + 16 * lwords - 4, ps, TAIL, n, KEY, 0, ptab, p_llr4, p_fl, tb) == E_INVAL
    assert soft(ctx, p_llr4 + 4 * lwords - 4, ps, TAIL, n, KEY, 0, ptab, p_llr4 + 4 * lwords, p_fl, tb) == E_INVAL
    # a misaligned device pointer, each of them
    for off in (1, 2, 3):
        assert pay(ctx, KEY, 0, ps, TAIL, n, p_pay + off) == E_INVAL
        assert bsc(ctx, p_line + off, ps, TAIL, n, KEY, 0, 5, p_line, p_fl, tb) == E_INVAL
        assert bsc(ctx, p_line, ps, TAIL, n, KEY, 0, 5, p_line + off, p_fl, tb) == E_INVAL
        assert bsc(ctx, p_line, ps, TAIL, n, KEY, 0, 5, p_line, p_fl + off, tb) == E_INVAL
        assert soft(ctx, p_line + off, ps, TAIL, n, KEY, 0, ptab, p_llr4, p_fl, tb) == E_INVAL
        assert soft(ctx, p_line, ps, TAIL, n, KEY, 0, ptab, p_llr4 + off, p_fl, tb) == E_INVAL
        assert soft(ctx, p_line, ps, TAIL, n, KEY, 0, ptab, p_llr4, p_fl + off, tb) == E_INVAL
        assert count(ctx, p_pay + off, None, p_st, p_on, ps, n, *cnt) == E_INVAL
        assert count(ctx, p_pay, p_pay + off, p_st, p_on, ps, n, *cnt) == E_INVAL
        assert count(ctx, p_pay, None, p_st + off, p_on, ps, n, *cnt) == E_INVAL
        assert count(ctx, p_pay, None, p_st, p_on + off, ps, n, *cnt) == E_INVAL
    # n_codewords 0: returns 0 and touches nothing, with buffers or without
    assert pay(ctx, KEY, 0, ps, TAIL, 0, p_pay) == 0 and pay(ctx, KEY, 0, None, HEAD, 0, None) == 0
    assert bsc(ctx, p_line, ps, TAIL, 0, KEY, 0, 5, p_line, p_fl, tb) == 0 and bsc(ctx, None, None, TAIL, 0, KEY, 0, 5, None, None, None) == 0
    assert soft(ctx, p_line, ps, TAIL, 0, KEY, 0, ptab, p_llr4, p_fl, tb) == 0 and soft(ctx, None, None, HEAD, 0, KEY, 0, None, None, None, None) == 0
    assert count(ctx, p_pay, None, p_st, p_on, ps, 0, *cnt) == 0 and count(ctx, None, None, None, None, None, 0, *cnt) == 0
    for t in (d_pay, d_line, d_llr4, d_fl):
        assert (t.cpu().numpy() == PATTERN).all()
    assert total.value == 77 and all(list(c) == [1, 2, 3, 4] for c in cnt)
    # and the same context serves a good call, also at a 4-byte offset: the accumulators start from zero
    one = np.array([288], np.uint32)
    assert pay(ctx, KEY, 5, one.ctypes.data, HEAD, 1, p_pay + 4) == 0
    want = abi.burst_payload_random_host(code50.code, KEY, 5, one, HEAD, 1, lib)
    assert np.array_equal(_inside(d_pay, n * kw + 4)[1:1 + want.size], want)
    assert count(ctx, p_pay + 4, None, p_st, p_on, one.ctypes.data, 1, *cnt) == 0
    bits = int(np.unpackbits(want.view(np.uint8)).sum())
    assert [list(c) for c in cnt] == [[2, 3, 3 + bits, 4], [2, 2, 3, 4], [2, 3, 4, 4]]
    assert bsc(ctx, p_pay + 4, one.ctypes.data, HEAD, 1, KEY, 5, 0, p_pay + 4, None, tb) == 0 and total.value == 77


# ---- round trip with nothing on the host ----
def _chain(abi, lib, dec, s, where, key, first, channel, x):
    """burst_payload_random_device -> encode_burst_device -> channel -> decode_burst_device -> burst_count_errors_device on device
    buffers; channel "bsc" (x the threshold, in place, HARD at magnitude 4) or "soft" (x the table, LLR4).  Returns what came back."""
    import torch
    code50 = dec.code50
    N, K, L = _dims(code50)
    n = len(s)
    line_bits, payload_bits = br.burst_words(n, K, L, s)
    lwords, pwords = line_bits // 32, payload_bits // 32
    d_pay, p_pay = _guarded(torch, pwords)
    d_line, p_line = _guarded(torch, lwords)
    d_llr4, p_llr4 = _guarded(torch, 4 * lwords if channel == "soft" else 1)
    d_back, p_back = _guarded(torch, pwords)
    d_st, p_st = _guarded(torch, n * 4)
    d_on, p_on = _guarded(torch, n)
    d_fl, p_fl = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.burst_payload_random_device(key, first, s, where, n, p_pay)
    dec.encode_burst_device(p_pay, s, where, n, p_line)
    if channel == "bsc":
        total = dec.burst_bsc_device(p_line, s, where, n, key, first, x, p_line, p_fl)
        dec.decode_burst_device(p_line, HARD, s, where, n, p_back, None, p_st, p_on, 4)
    else:
        total = dec.burst_soft_device(p_line, s, where, n, key, first, x, p_llr4, p_fl)
        dec.decode_burst_device(p_llr4, LLR4, s, where, n, p_back, None, p_st, p_on)
    counters = dec.burst_count_errors_device(p_back, p_pay, p_st, p_on, s, n, True, True, True)
    r = {"payload": _inside(d_pay, pwords), "back": _inside(d_back, pwords), "stats": _inside(d_st, n * 4).view(abi.line_stats_dtype()),
         "ones": _inside(d_on, n), "flips": _inside(d_fl, n), "total": total, "counters": counters}
    _inside(d_line, lwords)
    _inside(d_llr4, 4 * lwords if channel == "soft" else 1)
    return r


@WHERE
@pytest.mark.parametrize("channel", ["bsc", "soft"])
def test_round_trip(abi, lib, code50, dec, channel, where):
    """n = 65, "cycle", DecodeMethod 2, 10 iterations; the BSC at lnsfaid_line_bsc_threshold(0.005) in place and HARD at magnitude 4,
    the soft channel on lnsfaid_line_awgn_table at Eb/N0 4.2 dB (scale 13 / sqrt 2) and LLR4.  Everything decodes, and the decoder
    corrected exactly the positions the channel inverted, codeword for codeword.  No tolerance.  That needs the decoder itself to
    succeed on the batch.  Confirmed for KEY on the CPU port under oracle/ (lnsfaid_cpu_decode on lnsfaid_burst_to_llr4 of the host
    forms' output, 65 codewords in three groups): all 65 whole mother codewords come back, for both channels and both `where` - BSC
    11 .. 123 flips per codeword (TAIL; HEAD 12 .. 125) in 3, 4 and 3 iterations, soft channel 44 .. 398 (HEAD 45 .. 398) in 4, 4 and
    4, no bit-flipping iteration anywhere (the comment at KEY has the totals)."""
    n = 65
    s = br.batch("cycle", n)
    code = code50.code
    x = abi.line_bsc_threshold(0.005, lib) if channel == "bsc" else _table(abi, lib, code50, 4.2)
    r = _chain(abi, lib, dec, s, where, KEY, 0, channel, x)
    errors, fec, vs = r["counters"]
    flips = r["flips"]
    assert np.array_equal(r["payload"], abi.burst_payload_random_host(code, KEY, 0, s, where, n, lib))
    line, _ = abi.encode_burst_host(code, r["payload"], s, where, n, False, lib)
    host = (abi.burst_bsc_host if channel == "bsc" else abi.burst_soft_host)(code, line, s, where, n, KEY, 0, x, lib=lib)
    assert np.array_equal(flips, host[1]) and r["total"] == host[2] == int(flips.sum()) and flips.min() > 0
    assert errors == [65, 0, 0, 0]
    assert vs == [65, 0, 0, 0]
    assert fec[1] == 0
    assert np.array_equal(r["stats"]["corrected"], flips.astype(np.int32))
    assert fec[3] == r["total"]
    assert not r["ones"].any()
    assert fec == [65, 0, 65, r["total"]] and not r["stats"]["unsatisfied"].any() and np.array_equal(r["back"], r["payload"])


# ---- the driver ----
def _sim_rows(path):
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    return [{"threshold": int(r[1]), "codewords": int(r[2]), "flips": int(r[3]), "ber_in": float(r[4]), "errors": [int(x) for x in r[5:9]],
             "ber_out": float(r[10]), "fec": [int(x) for x in r[11:15]], "vs": [int(x) for x in r[15:19]], "columns": len(r),
             "sent_bits": int(r[20]), "payload_bits": int(r[21]), "short_ones": int(r[22])} for r in rows]


def _sim(tmp_path, name, args):
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    cwd = tmp_path / name
    cwd.mkdir()
    r = subprocess.run(["timeout", "-k", "10", "120", exe] + args, capture_output=True, text=True, cwd=str(cwd))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    text = open(str(cwd / "LineResult.txt")).read()
    assert [l for l in r.stdout.splitlines() if not l.startswith("#")] == [l for l in text.splitlines() if not l.startswith("#")]
    return text, str(cwd / "LineResult.txt")


def test_line_sim_burst_mode(abi, lib, code50, dec, tmp_path):
    """--burst-length 4 --shorten 288,14560 at p = 0.005: the row against the host forms over the same 128 global codewords (payload,
    lnsfaid_encode_burst_host, lnsfaid_burst_bsc_host: threshold, flips and both denominators) and against the same chain through
    pyabi with lnsfaid_burst_count_errors_host on what came back (the twelve counters); 4 calls of 32 give the same totals"""
    N, K, L = _dims(code50)
    code = code50.code
    common = ["--burst-length", "4", "--shorten", "288,14560", "--ber", "0.005", "--min-errors", "1", "--key", str(SIM_KEY)]
    _, path = _sim(tmp_path, "two", common + ["--codewords", "64", "--max-calls", "2"])
    rows = _sim_rows(path)
    assert len(rows) == 1 and rows[0]["columns"] == 23
    row = rows[0]
    threshold = abi.line_bsc_threshold(0.005, lib)
    s = bl.sim_shortened(0, 128, 4, [288, 14560])
    assert [int(v) for v in s[:8]] == [0, 0, 0, 288, 0, 0, 0, 14560]
    line_bits, payload_bits = br.burst_words(128, K, L, s)
    payload = abi.burst_payload_random_host(code, SIM_KEY, 0, s, TAIL, 128, lib)
    line, _ = abi.encode_burst_host(code, payload, s, TAIL, 128, False, lib)
    _, flips, total = abi.burst_bsc_host(code, line, s, TAIL, 128, SIM_KEY, 0, threshold, lib=lib)
    errors, fec, vs, ones = [0] * 4, [0] * 4, [0] * 4, 0
    for first in (0, 64):
        sh = bl.sim_shortened(first, 64, 4, [288, 14560])
        assert np.array_equal(sh, s[first:first + 64])
        c = _chain(abi, lib, dec, sh, TAIL, SIM_KEY, first, "bsc", threshold)
        assert np.array_equal(c["flips"], flips[first:first + 64])
        errors, fec, vs = abi.burst_count_errors_host(code, c["back"], c["payload"], c["stats"], c["ones"], sh, 64, errors, fec, vs, lib)
        ones += int((c["ones"] > 0).sum())
    want = {"threshold": threshold, "codewords": 128, "flips": total, "errors": errors, "fec": fec, "vs": vs, "sent_bits": line_bits,
            "payload_bits": payload_bits, "short_ones": ones}
    assert {k: row[k] for k in want} == want
    assert errors == [128, 0, 0, 0] and fec[1] == 0 and ones == 0
    assert row["ber_in"] == pytest.approx(total / line_bits, rel=1e-6) and row["ber_out"] == 0.0
    _, path4 = _sim(tmp_path, "four", common + ["--codewords", "32", "--max-calls", "4"])
    row4, = _sim_rows(path4)
    assert row4 == row


def test_line_sim_burst_mode_soft_head(abi, lib, code50, dec, tmp_path):
    """--ebn0 4.2 --where head: one call of 64 codewords; the row (22 columns and the three appended) against the same chain through
    pyabi and the host form of the soft channel"""
    N, K, L = _dims(code50)
    code = code50.code
    _, path = _sim(tmp_path, "soft", ["--burst-length", "4", "--shorten", "288,14560", "--where", "head", "--ebn0", "4.2", "--codewords", "64",
                                      "--max-calls", "1", "--min-errors", "1", "--key", str(SIM_KEY)])
    r, = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    assert len(r) == 25
    table = _table(abi, lib, code50, 4.2)
    s = bl.sim_shortened(0, 64, 4, [288, 14560])
    line_bits, payload_bits = br.burst_words(64, K, L, s)
    c = _chain(abi, lib, dec, s, HEAD, SIM_KEY, 0, "soft", table)
    line, _ = abi.encode_burst_host(code, c["payload"], s, HEAD, 64, False, lib)
    _, flips, total = abi.burst_soft_host(code, line, s, HEAD, 64, SIM_KEY, 0, table, lib=lib)
    assert np.array_equal(c["flips"], flips) and c["total"] == total
    errors, fec, vs = c["counters"]
    assert [int(x) for x in r[1:4]] == [int(table[7]), 64, total]
    assert [int(x) for x in r[5:9]] == errors and [int(x) for x in r[11:15]] == fec and [int(x) for x in r[15:19]] == vs
    assert [int(x) for x in r[22:25]] == [line_bits, payload_bits, int((c["ones"] > 0).sum())]
    assert float(r[4]) == pytest.approx(total / line_bits, rel=1e-6) and float(r[10]) == pytest.approx(errors[2] / payload_bits, rel=1e-6)


def test_line_sim_without_burst_length_is_unchanged(abi, lib, code50, dec, tmp_path):
    """without --burst-length the header and every row are those of the line calls: 20 columns, the counters of the same chain
    through pyabi, byte for byte apart from the seconds column"""
    text, path = _sim(tmp_path, "line", ["--ber", "0.005", "--codewords", "64", "--max-calls", "2", "--min-errors", "1", "--key", str(SIM_KEY)])
    lines = text.splitlines()
    assert lines[0] == "# lnsfaid_line_sim: DecodeMethod 2, 10 iterations, magnitude 4, key %d, 64 codewords per call" % SIM_KEY
    assert lines[1] == ("# p threshold codewords flipped_bits ber_in TestFrame ErrorFrame ErrorBits LT3ErrBitFrame FER ber_out "
                        "TotalCodewords UncorrectableCodewords CorrectedCodewords CorrectedBits "
                        "vsTestFrame vsErrorFrame UndetectedErrorFrame FalseAlarmFrame seconds")
    assert len(lines) == 3
    N, K, L = _dims(code50)
    threshold = abi.line_bsc_threshold(0.005, lib)
    line, _ = abi.encode_line_host(code50.code, abi.line_payload_random_host(code50.code, SIM_KEY, 0, 128, lib), 128, False, lib)
    _, flips, total = abi.line_bsc_host(code50.code, line, 128, SIM_KEY, 0, threshold, lib=lib)
    want = "0.005 %d 128 %d %.6e 128 0 0 0 %.6e %.6e 128 0 %d %d 128 0 0 0 " % (threshold, total, total / (128.0 * L), 0.0, 0.0,
                                                                              int((flips > 0).sum()), total)
    assert lines[2].startswith(want) and len(lines[2].split()) == 20, (lines[2], want)
