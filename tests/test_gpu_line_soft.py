"""Line-format soft channel on the GPU (include/lnsfaid.h "line-format soft channel", DESIGN.md §3.17, lnsfaid_line_soft.hip).  The
definition is the host form (tested against numpy in test_line_soft_cpu.py); the device form must return its bytes.  Every device
output lies between 64 guard words in front and 64 behind, which must keep their pattern after every call; `shift` words between the
front guard and the buffer put its base on 16, 8 or 4 bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_soft_ref as ls
from test_gpu_line_link import GUARD, PATTERN, SHIFTS, _device, _guarded, _inside, _words
from test_line_soft_cpu import tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "host")
E_INVAL = -1
MAX_GROUPS = 3
# All 96 codewords of this key from first_codeword 0 at Eb/N0 4.2 dB (default scale) decode on the CPU port (DecodeMethod 2, 10
# iterations: each codeword of lnsfaid_line_to_llr4 of the host-form output as a group of 32 copies): 298 .. 384 flips per codeword,
# 33 011 in all, at most 4 iterations (3.44 on average).
KEY = 0x5EED0F50C0DE2025
SIM_KEY = 20261019  # the same check at 4.2 dB: 96 of 96, 33 372 flips, at most 5 iterations
FLIPS_4_2 = 33011


@pytest.fixture(scope="module")
def dec(abi, code50):
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, MAX_GROUPS)
    yield d
    d.close()


def _table(abi, lib, code50, db):
    code = code50.code
    return abi.line_awgn_table(ls.ebn0_sigma(db, code.n_var - code.n_check, code.n_var - code.puncture_tail), ls.DEFAULT_SCALE, lib)


@pytest.fixture(scope="module")
def host_outputs(abi, lib, code50):
    """the host form on 96 random codewords per (first, table), computed once: a call on the first n of them gives the first n rows"""
    _, lw = _words(code50.code)
    line = np.random.default_rng(96).integers(0, 2 ** 32, size=(96, lw), dtype=np.uint64).astype(np.uint32)
    want = {(first, name): abi.line_soft_host(code50.code, line, 96, KEY, first, table, lib=lib)
            for first in (0, 2 ** 32 + 5) for name, table in tables().items()}
    return line, want


@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96])
def test_soft_device_equals_host(abi, lib, code50, dec, host_outputs, n, first):
    import torch
    _, lw = _words(code50.code)
    ow = 4 * lw  # output words per codeword
    all_lines, want_all = host_outputs
    line = all_lines[:n]
    for name, table in tables().items():
        want, want_flips, _ = want_all[(first, name)]
        want, want_flips = want[:n], want_flips[:n]
        want_total = int(want_flips.sum())
        assert (name in ("awgn", "middle", "ones")) == bool(want_total)
        for align, shift in SHIFTS.items():
            extra = 2  # room for two more codewords: nothing past codeword n - 1 is written
            d_in, p_in = _guarded(torch, n * lw, shift)
            d_in[GUARD + shift:GUARD + shift + n * lw] = _device(torch, line)
            d_out, p_out = _guarded(torch, (n + extra) * ow, shift)
            d_fl, p_fl = _guarded(torch, n + extra)
            assert p_out % align == 0 and p_in % align == 0 and (align == 16 or p_out % (2 * align) != 0)
            torch.cuda.synchronize()
            total = dec.line_soft_device(p_in, n, KEY, first, table, p_out, p_fl, total=1000)
            out = _inside(d_out, (n + extra) * ow, shift).reshape(n + extra, ow)
            flips = _inside(d_fl, n + extra)
            assert out[:n].tobytes() == want.tobytes(), (name, align)
            assert (out[n:].view(np.int32) == PATTERN).all() and (flips[n:].view(np.int32) == PATTERN).all(), (name, align)
            assert np.array_equal(flips[:n], want_flips) and total == 1000 + want_total, (name, align)
            assert np.array_equal(_inside(d_in, n * lw, shift).reshape(n, lw), line)  # a pure read of its input
    # without the optional outputs
    d_in, p_in = _guarded(torch, n * lw)
    d_in[GUARD:GUARD + n * lw] = _device(torch, line)
    d_out, p_out = _guarded(torch, n * ow)
    torch.cuda.synchronize()
    table = np.array(tables()["awgn"], np.uint32)
    assert lib.lnsfaid_line_soft_device(dec.ctx, p_in, n, KEY, first, table.ctypes.data, p_out, None, None) == 0
    assert _inside(d_out, n * ow).tobytes() == want_all[(first, "awgn")][0][:n].tobytes()


def _chain(abi, dec, n, key, first, table):
    """payload -> encode_line -> soft channel -> decode_line (LLR4) -> counters on device buffers; returns what came back"""
    import torch
    kw, lw = _words(dec.code50.code)
    d_pay, p_pay = _guarded(torch, n * kw)
    d_line, p_line = _guarded(torch, n * lw)
    d_llr, p_llr = _guarded(torch, n * 4 * lw)
    d_back, p_back = _guarded(torch, n * kw)
    d_st, p_st = _guarded(torch, n * 4)
    d_fl, p_fl = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.line_payload_random_device(key, first, n, p_pay)
    dec.encode_line_device(p_pay, n, p_line)
    total = dec.line_soft_device(p_line, n, key, first, table, p_llr, p_fl)
    dec.decode_line_device(p_llr, abi.LINE_LLR4, n, p_back, None, p_st)
    counters = dec.line_count_errors_device(p_back, p_pay, p_st, n, True, True, True)
    r = {"payload": _inside(d_pay, n * kw).reshape(n, kw), "back": _inside(d_back, n * kw).reshape(n, kw),
         "stats": _inside(d_st, n * 4).view(abi.line_stats_dtype()), "flips": _inside(d_fl, n), "total": total, "counters": counters}
    _inside(d_line, n * lw)
    _inside(d_llr, n * 4 * lw)
    return r


def test_round_trip_below_the_limit(abi, lib, code50, dec):
    """4.2 dB at n = 96: everything decodes, and the decoder corrected exactly the positions at which the channel's own decision was
    wrong.  No tolerance."""
    n = 96
    r = _chain(abi, dec, n, KEY, 0, _table(abi, lib, code50, 4.2))
    errors, fec, vs = r["counters"]
    flips = r["flips"]
    assert np.array_equal(r["payload"], abi.line_payload_random_host(code50.code, KEY, 0, n, lib))
    assert int(flips.sum()) == r["total"] == FLIPS_4_2
    assert errors == [96, 0, 0, 0]
    assert fec == [96, 0, int((flips > 0).sum()), int(flips.sum())]
    assert vs == [96, 0, 0, 0]
    assert np.array_equal(r["stats"]["corrected"], flips.astype(np.int32))
    assert not r["stats"]["unsatisfied"].any() and np.array_equal(r["back"], r["payload"])


def test_round_trip_above_the_limit(abi, lib, code50, dec):
    """1.0 dB, far below what the code corrects: error frames, and all twelve counters equal the host form on what came back"""
    n = 96
    r = _chain(abi, dec, n, KEY, 96, _table(abi, lib, code50, 1.0))
    errors, fec, vs = r["counters"]
    assert errors[1] > 0
    assert (errors, fec, vs) == abi.line_count_errors_host(code50.code, r["back"], r["payload"], r["stats"], n, True, True, True, lib)
    assert errors[0] == fec[0] == vs[0] == n and vs[1] == errors[1]


def test_refusals(abi, lib, code50, dec):
    import torch
    n = 96
    _, lw = _words(code50.code)
    d_line, p_line = _guarded(torch, (n + 1) * lw + 4)
    d_out, p_out = _guarded(torch, (n + 1) * 4 * lw + 4)
    d_fl, p_fl = _guarded(torch, n + 4)
    torch.cuda.synchronize()
    total = C.c_uint64(77)
    table = np.array(tables()["awgn"], np.uint32)
    down = table.copy()
    down[3] = down[2] - 1
    soft = lib.lnsfaid_line_soft_device
    t, dn = table.ctypes.data, down.ctypes.data

    def untouched():
        for buf in (d_line, d_out, d_fl):
            assert (buf.cpu().numpy() == PATTERN).all()
        assert total.value == 77

    assert soft(None, p_line, n, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_line, 97, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL      # more than 32 * max_groups codewords
    assert soft(dec.ctx, None, n, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_line, n, KEY, 0, t, None, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_line, n, KEY, 0, None, p_out, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_line, n, KEY, 0, dn, p_out, p_fl, C.byref(total)) == E_INVAL       # a table that decreases
    for off in (1, 2, 3):                                                                      # a misaligned device pointer, each of them
        assert soft(dec.ctx, p_line + off, n, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL
        assert soft(dec.ctx, p_line, n, KEY, 0, t, p_out + off, p_fl, C.byref(total)) == E_INVAL
        assert soft(dec.ctx, p_line, n, KEY, 0, t, p_out, p_fl + off, C.byref(total)) == E_INVAL
    # overlapping byte ranges: in place, the input at the last word of the output, the output at the last word of the input
    assert soft(dec.ctx, p_out, n, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_out + 4 * (n * 4 * lw - 1), n, KEY, 0, t, p_out, p_fl, C.byref(total)) == E_INVAL
    assert soft(dec.ctx, p_line, n, KEY, 0, t, p_line + 4 * (n * lw - 1), p_fl, C.byref(total)) == E_INVAL
    # n_codewords 0: returns 0 and touches nothing, with buffers or without
    assert soft(dec.ctx, p_line, 0, KEY, 0, t, p_out, p_fl, C.byref(total)) == 0
    assert soft(dec.ctx, None, 0, KEY, 0, None, None, None, None) == 0
    untouched()
    # and the same context works once the arguments are right, also at a 4-byte offset: the accumulator starts from zero
    line = np.full((1, lw), PATTERN, np.int32).view(np.uint32)
    want, want_flips, want_total = abi.line_soft_host(code50.code, line, 1, KEY, 5, table, lib=lib)
    assert soft(dec.ctx, p_line + 4, 1, KEY, 5, t, p_out + 4, p_fl + 4, C.byref(total)) == 0
    assert total.value == 77 + want_total
    out = _inside(d_out, (n + 1) * 4 * lw + 4)
    assert out[1:1 + 4 * lw].tobytes() == want.tobytes() and (out[1 + 4 * lw:].view(np.int32) == PATTERN).all() and out.view(np.int32)[0] == PATTERN
    fl = _inside(d_fl, n + 4)
    assert fl[1] == want_flips[0] and (np.delete(fl, 1).view(np.int32) == PATTERN).all()


def _sim_rows(path):
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    assert all(len(r) == 22 for r in rows)
    return [{"ebn0": float(r[0]), "table7": int(r[1]), "codewords": int(r[2]), "flips": int(r[3]), "errors": [int(x) for x in r[5:9]],
             "fec": [int(x) for x in r[11:15]], "vs": [int(x) for x in r[15:19]], "sigma": float(r[20]), "scale": float(r[21])} for r in rows]


def test_line_sim_equals_the_same_chain_through_pyabi(abi, lib, code50, dec, tmp_path):
    """the driver's LineResult.txt against the same calls with the same key and first_codeword sequence: two points of two calls of
    96 codewords, first_codeword 0, 96, 192, 288"""
    n, calls = 96, 2
    exe = os.path.join(HOST, "lnsfaid_line_sim")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, "--ebn0", "4.2,1.0", "--codewords", str(n), "--max-calls", str(calls),
                        "--min-errors", "1000", "--key", str(SIM_KEY)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    text = open(str(tmp_path / "LineResult.txt")).read().splitlines()
    assert "soft" in text[0] and text[1].split()[1:3] == ["ebn0_db", "table7"] and text[1].split()[-2:] == ["sigma", "scale"]
    rows = _sim_rows(str(tmp_path / "LineResult.txt"))
    assert len(rows) == 2 and [l for l in r.stdout.splitlines() if not l.startswith("#")] == [l for l in text if not l.startswith("#")]
    first = 0
    for row, db in zip(rows, (4.2, 1.0)):
        table = _table(abi, lib, code50, db)
        errors, fec, vs, flips = [0] * 4, [0] * 4, [0] * 4, 0
        for _ in range(calls):
            c = _chain(abi, dec, n, SIM_KEY, first, table)
            errors, fec, vs = ([a + b for a, b in zip(acc, new)] for acc, new in zip((errors, fec, vs), c["counters"]))
            flips += c["total"]
            first += n
        got = {k: row[k] for k in ("ebn0", "table7", "codewords", "flips", "errors", "fec", "vs")}
        assert got == {"ebn0": db, "table7": int(table[7]), "codewords": calls * n, "flips": flips, "errors": errors, "fec": fec, "vs": vs}, db
        assert abs(row["sigma"] - ls.ebn0_sigma(db, code50.K, code50.N - code50.code.puncture_tail)) < 1e-8 and abs(row["scale"] - ls.DEFAULT_SCALE) < 1e-8
    assert rows[0]["errors"][0] == rows[1]["errors"][0] == calls * n and rows[1]["errors"][1] > 0
