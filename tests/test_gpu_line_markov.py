"""Line-format error-propagation channel on the GPU (include/lnsfaid.h "line-format error-propagation channel", DESIGN.md §3.20,
lnsfaid_line_markov.hip).  The definition is the host form (tested against numpy in test_line_markov_cpu.py); the device form must
return its bytes.  Every device output lies between 64 guard words in front and 64 behind, which must keep their pattern after every
call; `shift` words between the front guard and the output put its base on 16, 8 or 4 bytes.

The kernel resolves the chain of a codeword in parallel: inside a word with one add, across the 64 words of a pass with one add on two
ballot masks, and from pass to pass with one carried bit that is re-seeded at each codeword.  The smallest shapes at which that can go
wrong are two, and both are here:
  - { 0, 0xFFFFFFFF, 2^31 } at n = 96: every codeword is all or nothing, so the carry has to pass through every word and every pass
    of the codewords that start inverted, and must not reach the codeword after them;
  - the long-run set { 2^32 / 500, floor(0.99 * 2^32), 0 } (mean run 100): runs that begin anywhere and cross word, 128-position and
    pass edges (a multiple of 2 048 positions).  The test asserts on the reference output that at least three runs cross a pass edge
    and at least one crosses a multiple of 128 that is no pass edge."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import line_markov_ref as lm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32
MAX_GROUPS = 3
# All 96 codewords of this key from first_codeword 0 behind the chain of (p, a) = (0.005, 0.5) decode on the CPU port (DecodeMethod 2,
# 10 iterations, magnitude 4: each codeword of lnsfaid_line_to_llr4 of the host-form line as a group of 32 copies): 52 .. 140 flips per
# codeword, 8 576 in all in 4 269 runs, at most 5 iterations and no bit flipping.  0.005 is the largest of 0.005, 0.003 and 0.002, and
# all three decode (5 057 and 3 320 flips).
KEY = 0x5EED0F50C0DE2025
ROUND_TRIP_P = 0.005
SIM_KEY = 20261019
SHIFTS = {16: 0, 8: 2, 4: 1}  # base alignment in bytes -> words behind the front guard (torch's allocations start on 256 bytes)
SETS = {"copy": [0, 0, 0], "helper": lm.thresholds(0.01, 0.5), "long": [2 ** 32 // 500, int(math.floor(0.99 * 2 ** 32)), 0],
        "all": [0, 0xFFFFFFFF, 2 ** 31]}


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
@pytest.mark.parametrize("n", [1, 2, 33, 96])
def test_markov_device_equals_host(abi, lib, code50, dec, n, first):
    import torch
    _, lw = _words(code50.code)
    L = 32 * lw
    line = np.random.default_rng(n).integers(0, 2 ** 32, size=(n, lw), dtype=np.uint64).astype(np.uint32)
    extra = 2  # room for two more codewords: nothing past codeword n - 1 is written
    for name, t in SETS.items():
        want, want_flips, want_runs, want_total, want_total_runs = abi.line_markov_host(code50.code, line, n, KEY, first, t, lib=lib)
        if name == "copy":
            assert np.array_equal(want, line) and want_total == 0
        if name == "all" and n == 96:  # codewords that start inverted and codewords that do not, the first kind followed by the second
            hit = want_flips > 0
            assert np.array_equal(want_flips[hit], np.full(int(hit.sum()), L)) and (hit[:-1] & ~hit[1:]).any() and (~hit[:-1] & hit[1:]).any()
        if name == "long" and n >= 33:
            e = lm.error_bits(KEY, first, n, L, t)
            assert np.array_equal(np.packbits(e, axis=1, bitorder="little").view(np.uint32).reshape(n, lw), want ^ line)
            assert lm.runs_crossing(e, 2048) >= 3 and lm.runs_crossing(e, 128, 2048) >= 1
        tt = np.array(t, np.uint32)
        for align, shift in SHIFTS.items():
            d_in, p_in = _guarded(torch, n * lw, shift)
            d_in[GUARD + shift:GUARD + shift + n * lw] = _device(torch, line)
            d_out, p_out = _guarded(torch, (n + extra) * lw, shift)
            d_fl, p_fl = _guarded(torch, n + extra)
            d_rn, p_rn = _guarded(torch, n + extra)
            assert p_in % align == 0 and p_out % align == 0 and (align == 16 or p_in % (2 * align) != 0)
            torch.cuda.synchronize()
            total, total_runs = dec.line_markov_device(p_in, n, KEY, first, t, p_out, p_fl, p_rn, total=1000, total_runs=500)
            out = _inside(d_out, (n + extra) * lw, shift).reshape(n + extra, lw)
            flips, runs = _inside(d_fl, n + extra), _inside(d_rn, n + extra)
            assert np.array_equal(out[:n], want), (name, align)
            assert (out[n:].view(np.int32) == PATTERN).all() and (flips[n:].view(np.int32) == PATTERN).all(), (name, align)
            assert (runs[n:].view(np.int32) == PATTERN).all(), (name, align)
            assert np.array_equal(flips[:n], want_flips) and np.array_equal(runs[:n], want_runs), (name, align)
            assert (total, total_runs) == (1000 + want_total, 500 + want_total_runs), (name, align)
            assert np.array_equal(_inside(d_in, n * lw, shift).reshape(n, lw), line)  # a pure read of its input
            # each optional output NULL in turn: the others as before, the dropped one untouched
            for drop in range(4):
                d_out.fill_(PATTERN), d_fl.fill_(PATTERN), d_rn.fill_(PATTERN)
                tf, tr = C.c_uint64(7), C.c_uint64(9)
                opt = [p_fl, p_rn, C.byref(tf), C.byref(tr)]
                opt[drop] = None
                assert lib.lnsfaid_line_markov_device(dec.ctx, p_in, n, KEY, first, tt.ctypes.data, p_out, *opt) == 0
                assert np.array_equal(_inside(d_out, (n + extra) * lw, shift).reshape(n + extra, lw)[:n], want), (name, align, drop)
                flips, runs = _inside(d_fl, n + extra), _inside(d_rn, n + extra)
                assert (flips.view(np.int32) == PATTERN).all() if drop == 0 else np.array_equal(flips[:n], want_flips), (name, align, drop)
                assert (runs.view(np.int32) == PATTERN).all() if drop == 1 else np.array_equal(runs[:n], want_runs), (name, align, drop)
                assert tf.value == 7 + (0 if drop == 2 else want_total) and tr.value == 9 + (0 if drop == 3 else want_total_runs)
            # in place, without the optional outputs
            assert lib.lnsfaid_line_markov_device(dec.ctx, p_in, n, KEY, first, tt.ctypes.data, p_in, None, None, None, None) == 0
            assert np.array_equal(_inside(d_in, n * lw, shift).reshape(n, lw), want), (name, align, "in place")


@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("n", [1, 2, 33, 96])
def test_equal_thresholds_are_the_bsc_kernels_output(abi, lib, code50, dec, n, first):
    """the degenerate set against lnsfaid_line_bsc_device's own output: line, flips and total, whatever t_start is"""
    import torch
    _, lw = _words(code50.code)
    line = np.random.default_rng(100 + n).integers(0, 2 ** 32, size=(n, lw), dtype=np.uint64).astype(np.uint32)
    threshold = abi.line_bsc_threshold(0.01, lib)
    for (align, shift), t_start in zip(SHIFTS.items(), (0, 12345, 0xFFFFFFFF)):
        d_in, p_in = _guarded(torch, n * lw, shift)
        d_in[GUARD + shift:GUARD + shift + n * lw] = _device(torch, line)
        d_bsc, p_bsc = _guarded(torch, n * lw, shift)
        d_out, p_out = _guarded(torch, n * lw, shift)
        d_fb, p_fb = _guarded(torch, n)
        d_fl, p_fl = _guarded(torch, n)
        torch.cuda.synchronize()
        bsc_total = dec.line_bsc_device(p_in, n, KEY, first, threshold, p_bsc, p_fb, total=3)
        total, _ = dec.line_markov_device(p_in, n, KEY, first, [threshold, threshold, t_start], p_out, p_fl, None, total=3)
        assert np.array_equal(_inside(d_out, n * lw, shift), _inside(d_bsc, n * lw, shift)), (align, t_start)
        assert np.array_equal(_inside(d_fl, n), _inside(d_fb, n)) and total == bsc_total > 3, (align, t_start)


def _chain(abi, dec, n, key, first, t):
    """payload -> encode_line -> the channel in place (t three thresholds; an int t is the BSC with that threshold) -> decode_line
    (HARD, magnitude 4) -> counters, on device buffers; returns what came back"""
    import torch
    kw, lw = _words(dec.code50.code)
    d_pay, p_pay = _guarded(torch, n * kw)
    d_line, p_line = _guarded(torch, n * lw)
    d_back, p_back = _guarded(torch, n * kw)
    d_st, p_st = _guarded(torch, n * 4)
    d_fl, p_fl = _guarded(torch, n)
    d_rn, p_rn = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.line_payload_random_device(key, first, n, p_pay)
    dec.encode_line_device(p_pay, n, p_line)
    if isinstance(t, int):
        total, total_runs = dec.line_bsc_device(p_line, n, key, first, t, p_line, p_fl), 0
    else:
        total, total_runs = dec.line_markov_device(p_line, n, key, first, t, p_line, p_fl, p_rn)
    dec.decode_line_device(p_line, abi.LINE_HARD, n, p_back, None, p_st, 4)
    counters = dec.line_count_errors_device(p_back, p_pay, p_st, n, True, True, True)
    r = {"payload": _inside(d_pay, n * kw).reshape(n, kw), "back": _inside(d_back, n * kw).reshape(n, kw),
         "stats": _inside(d_st, n * 4).view(abi.line_stats_dtype()), "flips": _inside(d_fl, n), "runs": _inside(d_rn, n), "total": total,
         "total_runs": total_runs, "counters": counters}
    _inside(d_line, n * lw)
    return r


def test_round_trip_below_the_correction_limit(abi, lib, code50, dec):
    """(p, a) = (0.005, 0.5) at n = 96: everything decodes, and the decoder corrected exactly the positions the channel inverted.  No
    tolerance."""
    n = 96
    r = _chain(abi, dec, n, KEY, 0, abi.line_markov_thresholds(ROUND_TRIP_P, 0.5, lib))
    errors, fec, vs = r["counters"]
    flips = r["flips"]
    assert np.array_equal(r["payload"], abi.line_payload_random_host(code50.code, KEY, 0, n, lib))
    assert int(flips.sum()) == r["total"] == 8576 and int(r["runs"].sum()) == r["total_runs"] == 4269
    assert errors == [96, 0, 0, 0]
    assert np.array_equal(r["stats"]["corrected"], flips.astype(np.int32))
    assert fec == [96, 0, int((flips > 0).sum()), r["total"]] and fec[3] == r["total"]
    assert vs == [96, 0, 0, 0]
    assert not r["stats"]["unsatisfied"].any() and np.array_equal(r["back"], r["payload"])


def test_round_trip_above_the_correction_limit(abi, lib, code50, dec):
    """(p, a) = (0.03, 0.5), well above what the code corrects: error frames, and all twelve counters equal the host form on what came
    back"""
    n = 96
    r = _chain(abi, dec, n, KEY, 96, abi.line_markov_thresholds(0.03, 0.5, lib))
    errors, fec, vs = r["counters"]
    assert errors[1] > 0
    assert (errors, fec, vs) == abi.line_count_errors_host(code50.code, r["back"], r["payload"], r["stats"], n, True, True, True, lib)
    assert errors[0] == fec[0] == vs[0] == n and vs[1] == errors[1]


def test_refusals(abi, lib, code50, dec):
    import torch
    n = 96
    _, lw = _words(code50.code)
    d_line, p_line = _guarded(torch, (n + 1) * lw + 4)
    d_fl, p_fl = _guarded(torch, n + 4)
    d_rn, p_rn = _guarded(torch, n + 4)
    torch.cuda.synchronize()
    total, total_runs = C.c_uint64(77), C.c_uint64(55)
    tot = (C.byref(total), C.byref(total_runs))
    t = np.array(SETS["helper"], np.uint32)
    down = np.array([t[1] + 1, t[1], t[2]], np.uint32)
    pt = t.ctypes.data
    markov = lib.lnsfaid_line_markov_device

    def untouched():
        for buf in (d_line, d_fl, d_rn):
            assert (buf.cpu().numpy() == PATTERN).all()
        assert total.value == 77 and total_runs.value == 55

    assert markov(dec.ctx, p_line, 97, KEY, 0, pt, p_line, p_fl, p_rn, *tot) == E_INVAL          # more than 32 * max_groups codewords
    assert markov(dec.ctx, None, n, KEY, 0, pt, p_line, p_fl, p_rn, *tot) == E_INVAL             # NULL required buffers
    assert markov(dec.ctx, p_line, n, KEY, 0, pt, None, p_fl, p_rn, *tot) == E_INVAL
    assert markov(dec.ctx, p_line, n, KEY, 0, None, p_line, p_fl, p_rn, *tot) == E_INVAL         # NULL t
    assert markov(dec.ctx, p_line, n, KEY, 0, down.ctypes.data, p_line, p_fl, p_rn, *tot) == E_INVAL  # t_idle > t_after
    for off in (1, 2, 3):                                                                        # a misaligned device pointer, each of them
        assert markov(dec.ctx, p_line + off, n, KEY, 0, pt, p_line, p_fl, p_rn, *tot) == E_INVAL
        assert markov(dec.ctx, p_line, n, KEY, 0, pt, p_line + off, p_fl, p_rn, *tot) == E_INVAL
        assert markov(dec.ctx, p_line, n, KEY, 0, pt, p_line, p_fl + off, p_rn, *tot) == E_INVAL
        assert markov(dec.ctx, p_line, n, KEY, 0, pt, p_line, p_fl, p_rn + off, *tot) == E_INVAL
    # n_codewords 0: returns 0 and touches nothing, with buffers or without
    assert markov(dec.ctx, p_line, 0, KEY, 0, pt, p_line, p_fl, p_rn, *tot) == 0
    assert markov(dec.ctx, None, 0, KEY, 0, None, None, None, None, None, None) == 0
    untouched()
    # and the same context works once the arguments are right, also at a 4-byte offset: the accumulators start from zero
    assert markov(dec.ctx, p_line + 4, 1, KEY, 5, pt, p_line + 4, p_fl + 4, p_rn + 4, *tot) == 0
    start = np.full((1, lw), PATTERN, np.uint32)
    want, want_flips, want_runs, want_total, want_total_runs = abi.line_markov_host(code50.code, start, 1, KEY, 5, t, lib=lib)
    inside = _inside(d_line, (n + 1) * lw + 4)
    assert np.array_equal(inside[1:1 + lw], want[0]) and inside[0] == PATTERN and (inside[1 + lw:] == PATTERN).all()
    assert _inside(d_fl, n + 4)[1] == want_flips[0] and _inside(d_rn, n + 4)[1] == want_runs[0]
    assert total.value == 77 + want_total and total_runs.value == 55 + want_total_runs


def _sim_rows(path):
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    out = []
    for r in rows:
        row = {"threshold": int(r[1]), "codewords": int(r[2]), "flips": int(r[3]), "errors": [int(x) for x in r[5:9]],
               "fec": [int(x) for x in r[11:15]], "vs": [int(x) for x in r[15:19]], "columns": len(r)}
        if len(r) > 20:
            row.update({"propagation": float(r[20]), "t_idle": int(r[21]), "t_after": int(r[22]), "runs": int(r[23]), "mean_run": r[24]})
        out.append(row)
    return out


def _sim(tmp_path, args):
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run(["timeout", "-k", "10", "120", exe] + args, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    path = str(tmp_path / "LineResult.txt")
    assert [l for l in r.stdout.splitlines() if not l.startswith("#")] == [l.rstrip("\n") for l in open(path) if not l.startswith("#")]
    return _sim_rows(path), open(path).read()


def test_line_sim_equals_the_same_chain_through_pyabi(abi, lib, code50, dec, tmp_path):
    """the driver's LineResult.txt with --propagation 0.5 against the same calls with the same key and first_codeword sequence: two
    points of two calls of 96 codewords, first_codeword 0, 96, 192, 288, the appended columns included; and one run without the
    option against the same chain with the BSC"""
    n, calls = 96, 2
    common = ["--codewords", str(n), "--max-calls", str(calls), "--min-errors", "1000", "--key", str(SIM_KEY)]
    rows, text = _sim(tmp_path, ["--ber", "%g,0.03" % ROUND_TRIP_P, "--propagation", "0.5"] + common)
    assert len(rows) == 2 and text.splitlines()[1].endswith(" seconds propagation t_idle t_after runs mean_run")
    first = 0
    for row, p in zip(rows, (ROUND_TRIP_P, 0.03)):
        t = abi.line_markov_thresholds(p, 0.5, lib)
        errors, fec, vs, flips, runs = [0] * 4, [0] * 4, [0] * 4, 0, 0
        for _ in range(calls):
            c = _chain(abi, dec, n, SIM_KEY, first, t)
            errors, fec, vs = ([a + b for a, b in zip(acc, new)] for acc, new in zip((errors, fec, vs), c["counters"]))
            flips += c["total"]
            runs += c["total_runs"]
            first += n
        assert row == {"threshold": int(t[2]), "codewords": calls * n, "flips": flips, "errors": errors, "fec": fec, "vs": vs, "columns": 25,
                       "propagation": 0.5, "t_idle": int(t[0]), "t_after": int(t[1]), "runs": runs, "mean_run": "%.6f" % (flips / runs)}, p
        assert int(t[2]) == abi.line_bsc_threshold(p, lib)  # column 1 stays the threshold of the marginal BER
    assert rows[0]["errors"][0] == rows[1]["errors"][0] == calls * n and rows[1]["errors"][1] > 0
    # without the option: the BSC chain and the columns of before
    rows, text = _sim(tmp_path, ["--ber", "%g" % ROUND_TRIP_P] + common)
    assert len(rows) == 1 and "propagation" not in text and text.splitlines()[1].endswith(" seconds")
    threshold = abi.line_bsc_threshold(ROUND_TRIP_P, lib)
    errors, fec, vs, flips = [0] * 4, [0] * 4, [0] * 4, 0
    for call in range(calls):
        c = _chain(abi, dec, n, SIM_KEY, call * n, threshold)
        errors, fec, vs = ([a + b for a, b in zip(acc, new)] for acc, new in zip((errors, fec, vs), c["counters"]))
        flips += c["total"]
    assert rows[0] == {"threshold": threshold, "codewords": calls * n, "flips": flips, "errors": errors, "fec": fec, "vs": vs, "columns": 20}
