"""FEC status on the GPU (include/lnsfaid.h "FEC status"): lnsfaid_fec_status_device and
lnsfaid_fec_status_packed_device (lnsfaid_fecstatus.hip) against the host forms of the same library, which
tests/test_fec_status_cpu.py holds against the numpy restatement; on real decoder output against the decoder's own per-codeword
syndrome count; and `lnsfaid_sim --fec-status`.  Exact integer equalities throughout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import capture_ref as cr
import fec_status_ref as fr
import oracle_abi as oa
from test_gpu_prefec import _on_device

pytestmark = pytest.mark.gpu

E_INVAL = -1
EXE = os.path.join(oa.PKG_DIR, "host", "lnsfaid_sim")
START = ([3, 5, 7, 1 << 40], [1, 2, 3, 4])  # what out and vs_sent hold before a call: both are added to


def _bytes_on_device(arr, shift):
    """a copy of arr's bytes on the device, `shift` bytes after a 16-byte boundary: (tensor to keep alive, pointer)"""
    import torch
    return _on_device(np.ascontiguousarray(arr).view(np.uint8).reshape(-1), shift, torch.uint8)


def _same(a, b):
    assert (a[0] is None) == (b[0] is None)
    if a[0] is not None:
        bad = np.nonzero(a[0] != b[0])[0]
        assert bad.size == 0, (bad[:8], a[0][bad[:8]], b[0][bad[:8]])
    assert a[1:] == b[1:], (a[1:], b[1:])


@pytest.fixture(scope="module")
def batch5(code50):
    """5 groups: random decisions, clean frames, single wrong bits (the host form's results are computed once per test from it)"""
    return fr.random_batch(code50.code, 55, 5)


@pytest.fixture(scope="module")
def dec5(abi, code50):
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, 5)
    yield d
    d.close()


@pytest.mark.parametrize("n_groups", [1, 3, 5])
def test_group_counts(abi, lib, code50, batch5, dec5, n_groups):
    """odd workgroup counts and the last workgroup of a batch, int8 and packed"""
    N = code50.N
    fix, dec, sent = (a[:n_groups * 32 * N] for a in batch5)
    want = abi.fec_status_host(code50.code, fix, dec, sent, n_groups, out=START[0], vs_sent=START[1], lib=lib)
    keep = [_bytes_on_device(a, 0) for a in (fix, dec, sent)]
    got = dec5.fec_status_device(keep[0][1], keep[1][1], keep[2][1], n_groups, out=START[0], vs_sent=START[1])
    _same(got, want)
    assert want[1][0] == START[0][0] + 32 * n_groups and want[0]["unsatisfied"].any() and (want[0]["unsatisfied"] == 0).any()
    dec01 = (dec != 0).astype(np.int8)
    want = abi.fec_status_host(code50.code, fix, dec01, sent, n_groups, out=START[0], vs_sent=START[1], lib=lib)
    keep = [_bytes_on_device(a, 0) for a in (abi.pack_llr4(fix, lib), fr.pack_decisions(dec01), sent)]
    got = dec5.fec_status_packed_device(keep[0][1], keep[1][1], keep[2][1], n_groups, out=START[0], vs_sent=START[1])
    _same(got, want)


def test_planted_pairs_25_groups(abi, lib, code50):
    """the largest shape: 789 codewords with two flipped neighbours of one check each (rows 0, 37 and 255 of every layer: every
    circulant's rotation at both ends of the 256-bit block), then random decisions, in one call of 200 workgroups"""
    n = 25
    fix, dec, sent = fr.pair_batch(code50.code, 25, n)
    want = abi.fec_status_host(code50.code, fix, dec, sent, n, out=START[0], vs_sent=START[1], lib=lib)
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    keep = [_bytes_on_device(a, 0) for a in (fix, dec, sent)]
    _same(d.fec_status_device(keep[0][1], keep[1][1], keep[2][1], n, out=START[0], vs_sent=START[1]), want)
    keep = [_bytes_on_device(a, 0) for a in (abi.pack_llr4(fix, lib), fr.pack_decisions(dec), sent)]
    _same(d.fec_status_packed_device(keep[0][1], keep[1][1], keep[2][1], n, out=START[0], vs_sent=START[1]), want)
    assert (want[0]["unsatisfied"][:789] <= 24).all() and (want[0]["unsatisfied"][:789] >= 2).all()
    d.close()


@pytest.mark.parametrize("shifts", [(1, 1, 1), (4, 4, 4), (0, 1, 4), (4, 0, 1), (1, 4, 0)], ids=lambda s: "%d%d%d" % s)
def test_alignment(abi, lib, code50, batch5, dec5, shifts):
    """every input pointer 0, 1 or 4 bytes into its buffer: more alignment only widens the loads"""
    n, N = 3, code50.N
    fix, dec, sent = (a[:n * 32 * N] for a in batch5)
    dec01 = (dec != 0).astype(np.int8)
    want = abi.fec_status_host(code50.code, fix, dec01, sent, n, out=START[0], vs_sent=START[1], lib=lib)
    keep = [_bytes_on_device(a, s) for a, s in zip((fix, dec01, sent), shifts)]
    _same(dec5.fec_status_device(keep[0][1], keep[1][1], keep[2][1], n, out=START[0], vs_sent=START[1]), want)
    keep = [_bytes_on_device(a, s) for a, s in zip((abi.pack_llr4(fix, lib), fr.pack_decisions(dec01), sent), shifts)]
    _same(dec5.fec_status_packed_device(keep[0][1], keep[1][1], keep[2][1], n, out=START[0], vs_sent=START[1]), want)


def test_optional_arguments(abi, lib, code50, batch5, dec5):
    n, N = 3, code50.N
    fix, dec, sent = (a[:n * 32 * N] for a in batch5)
    code = code50.code
    p = [_bytes_on_device(a, 0) for a in (fix, dec, sent)]
    p_fix, p_dec, p_sent = (x[1] for x in p)
    # d_fixInput NULL: corrected 0 everywhere
    got = dec5.fec_status_device(None, p_dec, p_sent, n, vs_sent=True)
    _same(got, abi.fec_status_host(code, None, dec, sent, n, vs_sent=True, lib=lib))
    assert not got[0]["corrected"].any()
    # d_records NULL; vs_sent NULL
    _same(dec5.fec_status_device(p_fix, p_dec, p_sent, n, records=False, vs_sent=True),
          abi.fec_status_host(code, fix, dec, sent, n, records=False, vs_sent=True, lib=lib))
    _same(dec5.fec_status_device(p_fix, p_dec, p_sent, n), abi.fec_status_host(code, fix, dec, sent, n, lib=lib))
    # sent NULL with vs_sent: the all-zero codeword
    got = dec5.fec_status_device(p_fix, p_dec, None, n, vs_sent=True)
    _same(got, abi.fec_status_host(code, fix, dec, None, n, vs_sent=True, lib=lib))
    assert got[2][1] > abi.fec_status_host(code, fix, dec, sent, n, vs_sent=True, lib=lib)[2][1]
    # no output at all; n_groups 0
    assert lib.lnsfaid_fec_status_device(dec5.ctx, p_fix, p_dec, p_sent, n, None, None, None) == 0
    out = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert lib.lnsfaid_fec_status_device(dec5.ctx, None, None, None, 0, None, out, out) == 0 and list(out) == [1, 2, 3, 4]
    assert lib.lnsfaid_fec_status_packed_device(dec5.ctx, None, None, None, 0, None, out, out) == 0 and list(out) == [1, 2, 3, 4]


def test_limits(abi, lib, code50, dec5):
    import torch
    buf = torch.zeros(32 * code50.N + 64, dtype=torch.int8, device="cuda")
    rec = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    out, vs = (C.c_uint64 * 4)(1, 2, 3, 4), (C.c_uint64 * 4)(5, 6, 7, 8)
    for fn in (lib.lnsfaid_fec_status_device, lib.lnsfaid_fec_status_packed_device):
        assert fn(None, p, p, p, 1, rec.data_ptr(), out, vs) == E_INVAL
        assert fn(dec5.ctx, p, None, p, 1, rec.data_ptr(), out, vs) == E_INVAL
        assert fn(dec5.ctx, p, p, p, 6, rec.data_ptr(), out, vs) == E_INVAL  # above max_groups
    torch.cuda.synchronize()
    assert list(out) == [1, 2, 3, 4] and list(vs) == [5, 6, 7, 8] and (rec.cpu().numpy() == 0x5A5A5A5A).all()


def test_guard_bytes_and_pure_read(abi, lib, code50, batch5, dec5):
    """nothing is written outside the n_groups * 32 records, and no input byte changes"""
    import torch
    n, N = 3, code50.N
    fix, dec, sent = (a[:n * 32 * N] for a in batch5)
    want = abi.fec_status_host(code50.code, fix, dec, sent, n, vs_sent=True, lib=lib)
    for packed in (False, True):
        src = (abi.pack_llr4(fix, lib), fr.pack_decisions(dec), sent) if packed else (fix, dec, sent)
        if packed:
            want = abi.fec_status_host(code50.code, fix, (dec != 0).astype(np.int8), sent, n, vs_sent=True, lib=lib)
        keep = [_bytes_on_device(a, 0) for a in src]
        rec = torch.full((16 + 2 * 32 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fn = dec5.fec_status_packed_device if packed else dec5.fec_status_device
        got = fn(keep[0][1], keep[1][1], keep[2][1], n, vs_sent=True, d_records_ptr=rec.data_ptr() + 64)
        assert got[0] is None and got[1:] == want[1:]
        r = rec.cpu().numpy().view(np.uint32)
        assert (r[:16] == 0x5A5A5A5A).all() and (r[-16:] == 0x5A5A5A5A).all()
        assert r[16:-16].view(fr.RECORD).tobytes() == want[0].tobytes()
        for (t, _), a in zip(keep, src):
            assert t.cpu().numpy()[:a.nbytes].tobytes() == np.ascontiguousarray(a).tobytes()


def test_against_the_decoders_own_count(abi, lib, code50):
    """per-codeword rule: the status call's unsatisfied equals cw_stats.unsatisfied codeword for codeword, on the 3.55 dB golden group
    (one trapped frame) and on a 3.3 dB group behind the device front-end (mostly failing frames); the caller never synchronises
    between the calls.  Group rule: the status call equals the host form on the buffers copied back."""
    import torch
    N, M = code50.N, code50.M
    n = 2
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    z, gold_fix, gold_dec = fr.golden_group("m2_3p55dB_cw_g0", N)
    d_fix = torch.empty(n * 32 * N, dtype=torch.int8, device="cuda")
    d_fix[:32 * N] = torch.from_numpy(gold_fix)
    d_dec = torch.empty(n * 32 * N, dtype=torch.int8, device="cuda")
    d_cw = torch.zeros((n * 32, 3), dtype=torch.int32, device="cuda")
    d_rec = torch.zeros(n * 32 * 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # group 1: the all-zero codeword through the device front-end at 3.3 dB
    seeds, draws = (C.c_uint32 * 1)(101), (C.c_uint64 * 1)(0)
    sigma = oa.load().lnsfaid_frontend_sigma(3.3, 2, oa.ReferenceChannel.RATE)
    assert lib.lnsfaid_frontend_device(d.ctx, seeds, draws, 1, 2, sigma, 13.0, None, d_fix.data_ptr() + 32 * N) == 0
    d.decode_codewords_device(d_fix.data_ptr(), n, d_dec.data_ptr(), d_cw.data_ptr())
    _, out, _ = d.fec_status_device(d_fix.data_ptr(), d_dec.data_ptr(), None, n, d_records_ptr=d_rec.data_ptr())
    rec = d_rec.cpu().numpy().view(np.uint32).view(fr.RECORD)
    cw = d_cw.cpu().numpy()
    print("unsatisfied, 3.55 dB golden group:", rec["unsatisfied"][:32].tolist())
    print("unsatisfied, 3.3 dB group:", rec["unsatisfied"][32:].tolist())
    assert rec["unsatisfied"].tolist() == cw[:, 2].tolist()
    assert (rec["unsatisfied"][32:] > 0).sum() >= 4 and out[0] == 64 and out[1] == int((cw[:, 2] > 0).sum())
    # the group rule (the default): decode_device, then the status of its output against the host form
    d.decode_device(d_fix.data_ptr(), n, d_dec.data_ptr())
    sent = np.concatenate([cr.layout_of(np.tile(fr.golden_codeword(N), (32, 1)), 1, N, M), np.zeros(32 * N, dtype=np.int8)])
    p_sent = _bytes_on_device(sent, 0)
    got = d.fec_status_device(d_fix.data_ptr(), d_dec.data_ptr(), p_sent[1], n, vs_sent=True)
    fix, dec = d_fix.cpu().numpy(), d_dec.cpu().numpy()
    assert np.array_equal(dec[:32 * N], gold_dec)
    want = abi.fec_status_host(code50.code, fix, dec, sent, n, vs_sent=True, lib=lib)
    _same(got, want)
    assert got[0]["unsatisfied"][:32].tolist() == [175 if m == 9 else 0 for m in range(32)]
    assert got[2][1] == d.count_errors_device(d_dec.data_ptr(), p_sent[1], 1)[1] + d.count_errors_device(d_dec.data_ptr() + 32 * N, None, 1)[1]
    d.close()


# ---- lnsfaid_sim --fec-status ----------------------------------------------------------------------------------------------
def _driver(tmp, extra, eb_n0=3.55):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    prof = open(os.path.join(oa.PKG_DIR, "host", "Profile.txt")).read()
    prof = prof.replace("StartSNR: 3.3", "StartSNR: %g" % eb_n0).replace("EndSNR: 3.85", "EndSNR: %g" % (eb_n0 + 0.05))
    assert "DecodeMethod: 2" in prof
    (tmp / "Profile.txt").write_text(prof)
    return subprocess.run([EXE, "--streams", "4", "--gpus", "1", "--max-rounds", "1"] + extra, cwd=tmp, capture_output=True, text=True,
                          timeout=600)


def test_driver_fec_status(tmp_path):
    res = _driver(tmp_path, ["--device-frontend", "--fec-status"])
    assert res.returncode == 0, res.stderr
    row = [int(x) for x in (tmp_path / "fecstatus.txt").read_text().splitlines()[-1].split()[1:]]
    result = (tmp_path / "Result.txt").read_text().splitlines()[-1].split()
    test_frame, error_frame = int(result[1]), int(result[2])
    print("fecstatus.txt:", row, "Result.txt:", test_frame, error_frame)
    assert len(row) == 8 and row[0] == row[4] == test_frame == 4 * 50 * 32 and row[5] == error_frame
    assert row[1] >= row[5] - row[6] and row[2] + row[1] <= row[0] and row[6] <= row[5]


def test_driver_without_the_flag(tmp_path):
    res = _driver(tmp_path, ["--device-frontend"])
    assert res.returncode == 0, res.stderr
    assert not (tmp_path / "fecstatus.txt").exists() and (tmp_path / "Result.txt").exists()
    res = subprocess.run([EXE, "--fec-status"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr and not (tmp_path / "fecstatus.txt").exists()
