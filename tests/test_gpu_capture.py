"""Error-frame capture on the GPU (include/lnsfaid.h "error-frame capture"): lnsfaid_capture_errors_device
(lnsfaid_capture.hip) against the host function of the same library, which tests/test_capture_cpu.py holds against the numpy
restatement; on real decoder output behind the device front-end; and `lnsfaid_sim --device-collect` against the host front-end's
dumps."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import capture_ref as cr
import encoder_ref as er
import oracle_abi as oa
from test_gpu_prefec import _on_device

pytestmark = pytest.mark.gpu

E_INVAL = -1
N_GROUPS = 3
EXE = os.path.join(oa.PKG_DIR, "host", "lnsfaid_sim")


def _host(lib, code50, fix, dec, sent, n_groups):
    ptr = [a.ctypes.data if a is not None else None for a in (fix, dec, sent)]
    return lambda skip, cap, r, p, f, s, o: lib.lnsfaid_capture_errors_host(code50.N, code50.M, ptr[0], ptr[1], ptr[2], n_groups, skip, cap,
                                                                            r, p, f, s, o)


def _device(lib, dec, ptr, n_groups):
    return lambda skip, cap, r, p, f, s, o: lib.lnsfaid_capture_errors_device(dec.ctx, ptr[0], ptr[1], ptr[2], n_groups, skip, cap, r, p, f, s, o)


def _same(host, device, n_var, skip, cap, slots, out=(3, 5, 7, 1 << 40)):
    """one call of each with guard bytes: return code, found, stored, every byte of both output buffers (the slots that were not
    written included) and the counters are equal.  Returns (found, stored, records, payload) of the device call."""
    h = cr.guarded_call(lambda r, p, f, s, o: host(skip, cap, r, p, f, s, o), n_var, slots, out)
    d = cr.guarded_call(lambda r, p, f, s, o: device(skip, cap, r, p, f, s, o), n_var, slots, out)
    assert h[0] == d[0] == 0, (h[0], d[0])
    assert d[1:3] == h[1:3], (d[1:3], h[1:3], skip, cap)
    assert d[3].tobytes() == h[3].tobytes() and d[4].tobytes() == h[4].tobytes(), (skip, cap)
    assert d[5] == h[5] and d[6] and h[6], (d[5], h[5])
    return d[1], d[2], d[3][:d[2]].copy(), d[4][:d[2]].copy()


@pytest.mark.parametrize("case", sorted(cr.CASES))
def test_device_equals_host(abi, lib, code50, case):
    import torch
    N, M = code50.N, code50.M
    fix, dec, sent = cr.batch(N, M, N_GROUPS, 100 + sorted(cr.CASES).index(case), *cr.CASES[case])
    host = _host(lib, code50, fix, dec, sent, N_GROUPS)
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, N_GROUPS)
    copies = [[_on_device(a, shift, torch.int8) for shift in (0, 1, 3)] for a in (fix, dec, sent)]
    n_found = len(cr.CASES[case][0]) + len(cr.CASES[case][2])
    for sf in range(3):
        for sd in range(3):
            for ss in range(3):
                device = _device(lib, d, [copies[0][sf][1], copies[1][sd][1], copies[2][ss][1]], N_GROUPS)
                found, stored, rec, pay = _same(host, device, N, 0, 96, 96)
                assert found == n_found == stored and rec["codeword"].tolist() == sorted(cr.CASES[case][0] + cr.CASES[case][2])
                _same(host, device, N, max(found - 3, 0), 2, 2)
    # the capacities and skips of the CPU test, and paging, on aligned inputs
    device = _device(lib, d, [copies[0][0][1], copies[1][0][1], copies[2][0][1]], N_GROUPS)
    _same(host, device, N, 0, 0, 0)
    for cap in (1, n_found + 3):
        for skip in sorted({0, max(n_found - 1, 0), n_found, n_found + 5}):
            _same(host, device, N, skip, cap, cap)
    _same(host, device, N, 1 << 40, 1 << 40, 96)  # numbers that do not fit 32 bits
    recs, skip = [], 0
    while True:
        _, stored, r2, _ = _same(host, device, N, skip, 2, 2)
        recs.append(r2)
        skip += stored
        if stored == 0 or skip >= n_found:
            break
    assert np.concatenate(recs)["codeword"].tolist() == rec["codeword"].tolist()
    # NULL inputs: the all-zero codeword, an empty LLR section
    for no_fix, no_sent in ((True, False), (False, True), (True, True)):
        h = _host(lib, code50, None if no_fix else fix, dec, None if no_sent else sent, N_GROUPS)
        dv = _device(lib, d, [None if no_fix else copies[0][1][1], copies[1][0][1], None if no_sent else copies[2][2][1]], N_GROUPS)
        _same(h, dv, N, 0, 96, 96)
    # out = NULL
    r = cr.guarded_call(lambda r, p, f, s, o: device(0, 96, r, p, f, s, None), N, 96)
    assert r[0] == 0 and r[1] == r[2] == n_found and r[6]
    d.close()


def test_one_larger_batch(abi, lib, code50):
    """70 groups: the rank kernel takes three chunks of 1024 codewords, with error frames on both sides of 1023 / 1024 and
    2047 / 2048 and of every power of two below; one-shot, paged with capacity 7, and twice for identical bytes"""
    import torch
    n_groups, N, M = 70, code50.N, code50.M
    rng = np.random.default_rng(70)
    planted = {0, 31, 32, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 2239} | set(np.nonzero(rng.random(32 * n_groups) < 0.05)[0].tolist())
    fix, dec, sent = cr.batch(N, M, n_groups, 71, sorted(planted))
    host = _host(lib, code50, fix, dec, sent, n_groups)
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    d_fix, d_dec, d_sent = (torch.from_numpy(a).cuda() for a in (fix, dec, sent))
    torch.cuda.synchronize()
    device = _device(lib, d, [d_fix.data_ptr(), d_dec.data_ptr(), d_sent.data_ptr()], n_groups)
    n_found = len(planted)
    found, stored, rec, pay = _same(host, device, N, 0, n_found + 9, n_found + 9)
    assert found == stored == n_found and rec["codeword"].tolist() == sorted(planted)
    # paged: the first pages against the host function, all of them against the one-shot result
    recs, pays, skip = [], [], 0
    while skip < n_found:
        if skip < 21:
            _, stored, r2, p2 = _same(host, device, N, skip, 7, 7)
        else:
            rc, f2, stored, r2, p2, _, intact = cr.guarded_call(lambda r, p, f, s, o: device(skip, 7, r, p, f, s, o), N, 7)
            assert rc == 0 and f2 == n_found and intact
            r2, p2 = r2[:stored].copy(), p2[:stored].copy()
        assert stored == min(7, n_found - skip)
        recs.append(r2)
        pays.append(p2)
        skip += stored
    assert np.concatenate(recs).tobytes() == rec.tobytes() and np.concatenate(pays).tobytes() == pay.tobytes()
    # determinism: the same call again gives the same bytes
    again = cr.guarded_call(lambda r, p, f, s, o: device(0, n_found + 9, r, p, f, s, o), N, n_found + 9, (0, 0, 0, 0))
    assert again[0] == 0 and again[1] == again[2] == n_found
    assert again[3][:n_found].tobytes() == rec.tobytes() and again[4][:n_found].tobytes() == pay.tobytes()
    d.close()


def test_limits(abi, lib, code50):
    import torch
    n_groups, N = 2, code50.N
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    buf = torch.zeros(3 * 32 * N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    fn = lib.lnsfaid_capture_errors_device
    rec = np.full(64, 0x5A5A5A5A, dtype=np.uint32).view(cr.RECORD)
    pay = np.full(16 * 3 * N, 0x5A, dtype=np.int8)
    found, stored = C.c_uint64(77), C.c_uint64(88)
    out = (C.c_uint64 * 4)(1, 2, 3, 4)
    f, s = C.byref(found), C.byref(stored)
    assert fn(d.ctx, p, p, p, n_groups + 1, 0, 16, rec.ctypes.data, pay.ctypes.data, f, s, out) == E_INVAL  # above max_groups
    assert fn(None, p, p, p, n_groups, 0, 16, rec.ctypes.data, pay.ctypes.data, f, s, out) == E_INVAL
    assert fn(d.ctx, p, None, p, n_groups, 0, 16, rec.ctypes.data, pay.ctypes.data, f, s, out) == E_INVAL
    assert fn(d.ctx, p, p, p, n_groups, 0, 16, rec.ctypes.data, pay.ctypes.data, None, s, out) == E_INVAL
    assert fn(d.ctx, p, p, p, n_groups, 0, 16, rec.ctypes.data, pay.ctypes.data, f, None, out) == E_INVAL
    assert fn(d.ctx, p, p, p, n_groups, 0, 16, None, pay.ctypes.data, f, s, out) == E_INVAL
    assert fn(d.ctx, p, p, p, n_groups, 0, 16, rec.ctypes.data, None, f, s, out) == E_INVAL
    assert (found.value, stored.value, list(out)) == (77, 88, [1, 2, 3, 4])  # a refused call touches nothing
    assert (rec.view(np.uint32) == 0x5A5A5A5A).all() and (pay == 0x5A).all()
    # n_groups 0: a no-op that sets found = stored = 0
    assert fn(d.ctx, None, None, None, 0, 0, 16, None, None, f, s, out) == 0
    assert (found.value, stored.value, list(out)) == (0, 0, [1, 2, 3, 4])
    # all-zero decisions against the all-zero codeword: counted, nothing found, nothing written
    found.value, stored.value = 77, 88
    assert fn(d.ctx, None, p, None, n_groups, 0, 16, rec.ctypes.data, pay.ctypes.data, f, s, out) == 0
    assert (found.value, stored.value, list(out)) == (0, 0, [65, 2, 3, 4])
    assert (rec.view(np.uint32) == 0x5A5A5A5A).all() and (pay == 0x5A).all()
    assert d.frontend_sent_bits() is None and lib.lnsfaid_frontend_sent_bits(None, None) == E_INVAL
    d.close()


def test_real_decoder_output(abi, lib, code50):
    """DecodeMethod 2 behind the device front-end at 3.5 dB QPSK (FER 0.12 in the README: 128 frames have errors with near
    certainty): frontend_random_frames -> frontend_device -> decode_device -> capture, the caller never synchronises"""
    import torch
    n, N, M, K = 4, code50.N, code50.M, code50.K
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    d.random_frames([0xC0FFEE + 31 * s for s in range(n)])
    seeds, draws = (C.c_uint32 * n)(*[101 + 2 * s for s in range(n)]), (C.c_uint64 * n)(*([0] * n))
    d_clean, d_fix, d_dec = (torch.empty(n * 32 * N, dtype=torch.int8, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    # the sent frames, copied back: without noise the sign of every LLR is its bit
    assert lib.lnsfaid_frontend_device(d.ctx, seeds, draws, n, 2, 0.0, 13.0, None, d_clean.data_ptr()) == 0
    sigma = oa.load().lnsfaid_frontend_sigma(3.5, 2, oa.ReferenceChannel.RATE)
    assert lib.lnsfaid_frontend_device(d.ctx, seeds, draws, n, 2, sigma, 13.0, None, d_fix.data_ptr()) == 0
    d.decode_device(d_fix.data_ptr(), n, d_dec.data_ptr())
    sent_ptr = d.frontend_sent_bits()
    assert sent_ptr
    found, rec, pay, cnt = d.capture_errors_device(d_fix.data_ptr(), d_dec.data_ptr(), sent_ptr, n, capacity=128, counters=True)
    d_in = C.c_void_p()
    assert lib.lnsfaid_frontend_input_bits(d.ctx, C.byref(d_in)) == 0 and d_in.value
    want_cnt = d.count_errors_device(d_dec.data_ptr(), d_in.value, n)
    print("found %d, counters %s" % (found, cnt))
    assert found > 0 and cnt == want_cnt and found == cnt[1]
    sent = (d_clean.cpu().numpy() > 0).astype(np.int8)
    fix, dec = d_fix.cpu().numpy(), d_dec.cpu().numpy()
    w_found, w_rec, w_pay, w_cnt = cr.capture(N, M, fix, dec, sent, n, 0, 128)
    assert found == w_found and rec.tobytes() == w_rec.tobytes() and pay.tobytes() == w_pay.tobytes() and cnt == w_cnt
    assert int(rec["info_errors"].sum()) == cnt[2]
    assert not er.syndromes(er.parity_matrix(code50), pay[:, 2]).any()  # every captured sent frame is a codeword
    assert np.array_equal(pay[:, 0], cr.frames_of(fix, n, N, M)[rec["codeword"]])
    d.close()


# ---- lnsfaid_sim --device-collect ------------------------------------------------------------------------------------------
DUMPS = ("errorindex.txt", "errorfloat.txt", "errordecode.txt")


def _driver(tmp, extra, eb_n0=3.55):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    prof = open(os.path.join(oa.PKG_DIR, "host", "Profile.txt")).read()
    prof = prof.replace("StartSNR: 3.3", "StartSNR: %g" % eb_n0).replace("EndSNR: 3.85", "EndSNR: %g" % (eb_n0 + 0.05))
    assert "DecodeMethod: 2" in prof
    (tmp / "Profile.txt").write_text(prof)
    res = subprocess.run([EXE, "--streams", "2", "--gpus", "1", "--max-rounds", "1"] + extra, cwd=tmp, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr
    return {name: (tmp / name).read_text() for name in DUMPS}, res


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    return _driver(tmp_path_factory.mktemp("collect_host"), ["--collect"])[0]


@pytest.fixture(scope="module")
def run_b(tmp_path_factory):
    return _driver(tmp_path_factory.mktemp("collect_device"), ["--device-frontend", "--collect", "--device-collect"])[0]


def _lines(text, prefix):
    return [l for l in text.splitlines() if l.startswith(prefix)]


def _values(line, prefix):
    return line[len(prefix):line.rindex("]")].split()


def test_driver_device_collect_equals_host_collect(code50, run_a, run_b):
    assert len(_lines(run_a["errorindex.txt"], "ErrorFrame:")) >= 1
    assert run_b["errorindex.txt"] == run_a["errorindex.txt"]
    assert run_b["errordecode.txt"] == run_a["errordecode.txt"]
    assert _lines(run_b["errorfloat.txt"], "ErrorChar=") == _lines(run_a["errorfloat.txt"], "ErrorChar=")
    fa, fb = _lines(run_a["errorfloat.txt"], "ErrorFloat="), _lines(run_b["errorfloat.txt"], "ErrorFloat=")
    assert len(fa) == len(fb) == len(_lines(run_a["errorindex.txt"], "ErrorFrame:"))
    if fa == fb:  # the same text: nothing to parse
        assert all(len(_values(l, "ErrorFloat=[")) == code50.N for l in fa[:2])
        print("ErrorFloat: %d lines, identical text" % len(fa))
        return
    a = np.array([np.array(_values(l, "ErrorFloat=["), dtype=np.float64) for l in fa])
    b = np.array([np.array(_values(l, "ErrorFloat=["), dtype=np.float64) for l in fb])
    assert a.shape == b.shape and a.shape[1] == code50.N
    rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-300)
    print("ErrorFloat: %d values, largest relative difference %.3g" % (a.size, rel.max()))
    assert (rel <= 2e-5).all()


def test_driver_paging_changes_nothing(run_b, tmp_path):
    run_c, _ = _driver(tmp_path, ["--device-frontend", "--collect", "--device-collect", "--collect-capacity", "3"])
    assert len(_lines(run_c["errorindex.txt"], "ErrorFrame:")) >= 1
    assert run_c == run_b


def test_driver_device_collect_with_device_encoder(code50, tmp_path):
    """--device-encode: the dump is the only place the sent bits reach the host"""
    run_d, _ = _driver(tmp_path, ["--device-frontend", "--device-encode", "--collect", "--device-collect"])
    K = code50.K
    ob = np.array([[int(x) for x in _values(l, "outputbits=[")] for l in _lines(run_d["errordecode.txt"], "outputbits=[")], dtype=np.int8)
    ib = np.array([[int(x) for x in _values(l, "inputbits=[")] for l in _lines(run_d["errordecode.txt"], "inputbits=[")], dtype=np.int8)
    db = np.array([[int(x) for x in _values(l, "Decodedbits=[")] for l in _lines(run_d["errordecode.txt"], "Decodedbits=[")], dtype=np.int8)
    num = [int(l.split(":")[1]) for l in _lines(run_d["errorindex.txt"], "ErrorBit Num:")]
    assert len(num) >= 1 and ob.shape == db.shape == (len(num), code50.N) and ib.shape == (len(num), K)
    assert ob.any() and not er.syndromes(er.parity_matrix(code50), ob).any()
    assert np.array_equal(ib, ob[:, :K])
    assert (db[:, :K] != ib).sum(axis=1).tolist() == num


def test_driver_flags(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    res = subprocess.run([EXE, "--device-collect"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr
    res = subprocess.run([EXE, "--collect", "--device-collect"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr
    # --collect-capacity belongs to --device-collect
    res = subprocess.run([EXE, "--device-frontend", "--collect", "--collect-capacity", "3"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr
    res = subprocess.run([EXE, "--device-frontend", "--device-collect", "--collect-capacity", "0"], cwd=tmp_path, capture_output=True,
                         text=True, timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr


def test_driver_without_the_flag_writes_no_dumps(tmp_path):
    dumps, res = _driver(tmp_path, ["--device-frontend", "--collect"])
    assert "no error dumps" in res.stderr
    assert len(dumps["errorindex.txt"].splitlines()) == 1
