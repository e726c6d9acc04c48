"""The pre-FEC error counters on the GPU (include/lnsfaid.h "pre-FEC error counters"):
lnsfaid_prefec_errors_device (lnsfaid_prefec.hip) against the host function of the same library, which tests/test_prefec_cpu.py
holds against the numpy restatement; the fused counting of the device front-end against its own output bytes, against the
double-precision chain and through every sent-bit source; and `lnsfaid_sim --prefec`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import demap_ref as dr
import oracle_abi as oa
import prefec_ref as pr
from test_gpu_demap import EB_N0, SCALE

pytestmark = pytest.mark.gpu

E_INVAL = -1
CASES = sorted(EB_N0)


def _rx(code50, mod, il, n_groups, seed):
    """(noisy constellation points of random bits with the threshold values planted, the sent bits in the encoder's layout)"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 2, (n_groups, 32, code50.N), dtype=np.int8)
    sigma = oa.load().lnsfaid_frontend_sigma(EB_N0[(mod, il)], mod, oa.ReferenceChannel.RATE)
    rx = pr.plant(dr.noisy_symbols(rng, frames, mod, il, sigma), n_groups, code50.N, code50.M, il, mod)
    return rx, pr.sent_of_frames(frames, code50.M)


def _on_device(arr, shift, dtype):
    """a copy of arr on the device that starts `shift` elements after a 16-byte boundary: (tensor to keep alive, pointer)"""
    import torch
    buf = torch.zeros(arr.size + 16, dtype=dtype, device="cuda")
    buf[shift:shift + arr.size] = torch.from_numpy(arr)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + shift * buf.element_size()


@pytest.mark.parametrize("mod,il", CASES, ids=["m%d_i%d" % k for k in CASES])
def test_device_equals_host(abi, lib, code50, mod, il):
    import torch
    n_groups, N, M = 3, code50.N, code50.M
    rx, sent = _rx(code50, mod, il, n_groups, 700 + 10 * mod + il)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    keep_rx, rx_ptr = _on_device(rx, 0, torch.float32)
    keep_sent, sent_ptr = _on_device(sent, 0, torch.int8)
    for scope in (pr.INFO, pr.CODEWORD):
        want = abi.prefec_errors_host(N, M, il, rx, n_groups, mod, sent, scope, lib)
        got = dec.prefec_errors_device(rx_ptr, n_groups, mod, sent_ptr, scope)
        print("mod %d I %d scope %d: device %s host %s" % (mod, il, scope, got, want))
        assert got == want and want[0] == 96 and want[1] == 96 and want[2] > 0
        assert dec.prefec_errors_device(rx_ptr, n_groups, mod, None, scope) == abi.prefec_errors_host(N, M, il, rx, n_groups, mod, None, scope, lib)
    # ADDED to what out holds, one group only
    one = abi.prefec_errors_host(N, M, il, rx[:dr.rx_floats(N, mod)], 1, mod, sent[:32 * N], pr.INFO, lib)
    assert dec.prefec_errors_device(rx_ptr, 1, mod, sent_ptr, pr.INFO, out=[5, 6, 7, 1 << 40]) == [5 + one[0], 6 + one[1], 7 + one[2], (1 << 40) + one[3]]
    dec.close()


@pytest.mark.parametrize("mod,il", [(1, 1), (2, 1), (4, 1), (6, 1), (8, 1), (2, 2), (4, 4)], ids=lambda v: str(v))
def test_alignment_selects_the_loads_not_the_counts(abi, lib, code50, mod, il):
    import torch
    n_groups, N, M = 2, code50.N, code50.M
    rx, sent = _rx(code50, mod, il, n_groups, 900 + 10 * mod + il)
    want = [abi.prefec_errors_host(N, M, il, rx, n_groups, mod, sent, scope, lib) for scope in (pr.INFO, pr.CODEWORD)]
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    for rx_shift in (0, 1, 2):  # floats: 0, 4 and 8 bytes
        keep_rx, rx_ptr = _on_device(rx, rx_shift, torch.float32)
        for sent_shift in (0, 1, 3):
            keep_sent, sent_ptr = _on_device(sent, sent_shift, torch.int8)
            got = [dec.prefec_errors_device(rx_ptr, n_groups, mod, sent_ptr, scope) for scope in (pr.INFO, pr.CODEWORD)]
            assert got == want, (rx_shift, sent_shift, got, want)
    dec.close()


def test_limits(abi, lib, code50):
    import torch
    n_groups, N = 2, code50.N
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    d_rx = torch.zeros(3 * 32 * N + 4, dtype=torch.float32, device="cuda")
    d_sent = torch.zeros(3 * 32 * N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    out = (C.c_uint64 * 4)(1, 2, 3, 4)
    fn, rxp, sp = lib.lnsfaid_prefec_errors_device, d_rx.data_ptr(), d_sent.data_ptr()
    assert fn(dec.ctx, rxp, n_groups + 1, 2, sp, pr.INFO, out) == E_INVAL  # above max_groups
    assert fn(dec.ctx, rxp + 2, n_groups, 2, sp, pr.INFO, out) == E_INVAL  # d_rx not 4-byte aligned
    for scope in (0, 3, -1):
        assert fn(dec.ctx, rxp, n_groups, 2, sp, scope, out) == E_INVAL
    for mod in (0, 3, 5, 7, 16):
        assert fn(dec.ctx, rxp, n_groups, mod, sp, pr.INFO, out) == E_INVAL
    assert fn(dec.ctx, None, n_groups, 2, sp, pr.INFO, out) == E_INVAL and fn(dec.ctx, rxp, n_groups, 2, sp, pr.INFO, None) == E_INVAL
    assert fn(None, rxp, n_groups, 2, sp, pr.INFO, out) == E_INVAL
    assert fn(dec.ctx, None, 0, 2, None, pr.INFO, None) == 0 and fn(dec.ctx, None, 0, 2, None, 0, None) == E_INVAL
    assert list(out) == [1, 2, 3, 4]  # a refused call adds nothing
    # all-zero levels decide 0 against all-zero sent bits; the interleaver is the context's
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, 3) == 0
    assert fn(dec.ctx, rxp, n_groups, 2, sp, pr.CODEWORD, out) == 0 and list(out) == [65, 2, 3, 4]
    assert lib.lnsfaid_frontend_set_prefec(dec.ctx, 3) == E_INVAL and lib.lnsfaid_frontend_set_prefec(None, 1) == E_INVAL
    assert lib.lnsfaid_frontend_prefec_counters(dec.ctx, None, 0) == E_INVAL
    dec.close()


def test_symbols_to_bits_with_both_counters_without_synchronisation(abi, lib, code50, encoder):
    """prefec_errors_device -> demap_packed_device -> decode_packed_device -> count_errors_packed_device on the context's stream,
    the caller never synchronises"""
    import torch
    n_groups, mod, il, K, N, M = 2, 4, 4, code50.K, code50.N, code50.M
    rng = np.random.default_rng(41)
    info = rng.integers(0, 2, (n_groups, 32, K), dtype=np.uint8)
    frames = np.stack([encoder.encode(i) for i in info]).astype(np.int8)
    sigma = oa.load().lnsfaid_frontend_sigma(8.6, mod, oa.ReferenceChannel.RATE)
    rx = dr.noisy_symbols(rng, frames, mod, il, sigma)
    sent = pr.sent_of_frames(frames, M)
    cfg = abi.default_cfg(2, 10)
    dec = abi.Decoder(code50, cfg, 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    d_rx, d_sent = torch.from_numpy(rx).cuda(), torch.from_numpy(sent).cuda()
    d_llr4 = torch.zeros(n_groups * 16 * N, dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros(n_groups * N, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((n_groups, 2), dtype=torch.int32, device="cuda")
    info8 = np.ascontiguousarray(info.reshape(-1).astype(np.int8))
    d_msg = torch.from_numpy(abi.pack_bits(info8, lib)).cuda()
    torch.cuda.synchronize()
    pre = dec.prefec_errors_device(d_rx.data_ptr(), n_groups, mod, d_sent.data_ptr(), pr.INFO)
    dec.demap_packed_device(d_rx.data_ptr(), n_groups, mod, SCALE[mod], d_llr4.data_ptr())
    dec.decode_packed_device(d_llr4.data_ptr(), n_groups, d_bits.data_ptr(), d_st.data_ptr())
    post = dec.count_errors_packed_device(d_bits.data_ptr(), d_msg.data_ptr(), n_groups)
    assert pre == abi.prefec_errors_host(N, M, il, rx, n_groups, mod, sent, pr.INFO, lib) and pre[2] > 0
    fix = abi.demap_host(N, M, il, rx, n_groups, mod, SCALE[mod], lib)
    ref, ref_stats = oa.decode_mt(code50, cfg, fix, n_groups, kind="avx2")
    assert np.array_equal(abi.unpack_bits(d_bits.cpu().numpy().view(np.uint32), lib), ref)
    assert post == oa.Oracle(code50, cfg).count_errors(ref, info8, n_groups)
    dec.close()


# ---- fused counting in the device front-end ---------------------------------------------------------------------------
SEEDS = [101, 103, 1019]
FRONTEND = [(2, 1, 13.0, 3.6), (4, 4, 12.5, 8.6), (8, 1, 40.0, 19.0)]  # Eb/N0 and scale of tests/test_gpu_frontend.py


def _frontend(lib, dec, code50, mod, eb_n0, scale, call=0, codeword=None, seeds=SEEDS):
    import torch
    n = len(seeds)
    d_fix = torch.empty(n * 32 * code50.N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    sigma = oa.load().lnsfaid_frontend_sigma(eb_n0, mod, oa.ReferenceChannel.RATE) if eb_n0 is not None else 0.0
    per_group = lib.lnsfaid_frontend_draws_per_group(dec.ctx, mod)
    cw = None if codeword is None else np.ascontiguousarray(codeword, dtype=np.int8).ctypes.data
    rc = lib.lnsfaid_frontend_device(dec.ctx, (C.c_uint32 * n)(*seeds), (C.c_uint64 * n)(*([call * per_group] * n)), n, mod, sigma, scale,
                                     cw, d_fix.data_ptr())
    assert rc == 0, lib.lnsfaid_last_hip_error()
    return d_fix.cpu().numpy()


def _within(lower, got, upper):
    return got[0] == lower[0] == upper[0] and all(lo <= g <= up for lo, g, up in zip(lower[1:], got[1:], upper[1:]))


@pytest.mark.parametrize("mod,il,scale,eb_n0", FRONTEND, ids=["qpsk", "16qam_il4", "256qam"])
def test_fused_counting(abi, lib, code50, mod, il, scale, eb_n0):
    n, N, M = len(SEEDS), code50.N, code50.M
    rng = np.random.default_rng(60 + mod)
    frames = rng.integers(0, 2, (n, 32, N), dtype=np.int8)
    sent = pr.sent_of_frames(frames, M)
    info = np.ascontiguousarray(frames[:, :, :code50.K]).reshape(-1)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    assert lib.lnsfaid_frontend_set_frames(dec.ctx, sent.ctypes.data, info.ctypes.data, n) == 0
    off = _frontend(lib, dec, code50, mod, eb_n0, scale)
    assert dec.frontend_prefec_counters() == [0, 0, 0, 0]  # never switched on
    for scope in (pr.INFO, pr.CODEWORD):
        dec.frontend_set_prefec(scope)
        assert lib.lnsfaid_frontend_set_exact(dec.ctx, 0) == 0
        on = _frontend(lib, dec, code50, mod, eb_n0, scale)
        fast = dec.frontend_prefec_counters()
        assert np.array_equal(on, off)  # (a) counting does not move a byte
        dec.frontend_set_prefec(scope)  # clears
        assert lib.lnsfaid_frontend_set_exact(dec.ctx, 1) == 0
        exact_bytes = _frontend(lib, dec, code50, mod, eb_n0, scale)
        exact = dec.frontend_prefec_counters()
        assert np.array_equal(exact_bytes, off) and fast == exact  # (b)
        lower, upper = pr.bounds_from_fix_input(on, n, N, M, il, mod, sent, scope)  # (c)
        print("mod %d scope %d: %s within %s .. %s" % (mod, scope, fast, lower, upper))
        assert _within(lower, fast, upper) and fast[0] == 32 * n and lower[2] > 0
    # (d) scale 1e6: a quantised value is zero only for |level| < 1e-6, so the bytes pin the counters
    assert lib.lnsfaid_frontend_set_exact(dec.ctx, 0) == 0
    host = np.concatenate([oa.ReferenceChannel(code50, s, 1e6, mod_type=mod, interleave=il).groups(eb_n0, 1, frames=f) for s, f in zip(SEEDS, frames)])
    assert int((host == 0).sum()) <= 16  # the condition of this part, from the host generator (no GPU in it)
    dec.frontend_set_prefec(pr.CODEWORD)
    big = _frontend(lib, dec, code50, mod, eb_n0, 1e6)
    got = dec.frontend_prefec_counters()
    lower, upper = pr.bounds_from_fix_input(big, n, N, M, il, mod, sent, pr.CODEWORD)
    print("mod %d scale 1e6: %s within %s .. %s" % (mod, got, lower, upper))
    assert _within(lower, got, upper) and upper[2] - lower[2] <= 16 and int((big == 0).sum()) <= 16
    dec.close()


def test_fused_counting_with_every_sent_bit_source(abi, lib, code50):
    """(e) codeword, NULL, set_frames and random_frames at scale 1e6, where the written bytes pin the counters to within the few
    zeros; (f) calls accumulate, reset clears, scope 0 stops the counting"""
    mod, il, eb_n0, scale, n, N, M = 2, 1, 3.6, 1e6, len(SEEDS), code50.N, code50.M
    cw = np.unpackbits(np.fromfile(os.path.join(oa.ROOT, "tests", "golden", "codeword_50gpon.bin"), dtype=np.uint8))[:N].astype(np.int8)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 2, (n, 32, N), dtype=np.int8)
    own = pr.sent_of_frames(frames, M)
    info = np.ascontiguousarray(frames[:, :, :code50.K]).reshape(-1)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    dec.random_frames([0xABCDEF + 31 * s for s in range(n)])
    drawn = (_frontend(lib, dec, code50, mod, None, 13.0) > 0).astype(np.int8)  # without noise the sign of fixInput is the sent bit
    assert 0.4 < drawn.mean() < 0.6

    def check(sent, codeword=None, scope=pr.INFO):
        dec.frontend_set_prefec(scope)
        fix = _frontend(lib, dec, code50, mod, eb_n0, scale, codeword=codeword)
        got = dec.frontend_prefec_counters()
        lower, upper = pr.bounds_from_fix_input(fix, n, N, M, il, mod, sent, scope)
        print("%s within %s .. %s" % (got, lower, upper))
        in_scope = upper[0] * (N - M if scope == pr.INFO else N)  # Q(1 / sigma) is 2.5 % at 3.6 dB
        assert _within(lower, got, upper) and upper[2] - lower[2] <= 16 and 0.02 * in_scope < got[2] < 0.03 * in_scope
        return got

    from_drawn = check(drawn)                                                  # random_frames
    assert check(np.tile(pr.sent_of_frames(np.tile(cw, (1, 32, 1)), M), n), codeword=cw) != from_drawn  # codeword, wins over the frames
    assert lib.lnsfaid_frontend_set_frames(dec.ctx, own.ctypes.data, info.ctypes.data, n) == 0
    one = check(own, scope=pr.CODEWORD)                                        # set_frames
    assert lib.lnsfaid_frontend_set_frames(dec.ctx, None, None, 0) == 0
    zero = check(None, scope=pr.CODEWORD)                                      # NULL: the all-zero codeword
    assert zero != one
    # (f) a second call with the next draws accumulates; reading does not clear unless asked to
    dec.frontend_set_prefec(pr.CODEWORD)
    _frontend(lib, dec, code50, mod, eb_n0, scale, call=0)
    _frontend(lib, dec, code50, mod, eb_n0, scale, call=1)
    both = dec.frontend_prefec_counters()
    assert both[0] == 2 * 32 * n and all(b > z for b, z in zip(both[2:], zero[2:])) and both[1] == 2 * zero[1]
    assert dec.frontend_prefec_counters(reset=True, out=[1, 1, 1, 1]) == [b + 1 for b in both]
    assert dec.frontend_prefec_counters() == [0, 0, 0, 0]
    _frontend(lib, dec, code50, mod, eb_n0, scale, call=0)
    assert dec.frontend_prefec_counters() == zero
    dec.frontend_set_prefec(0)  # clears and stops
    _frontend(lib, dec, code50, mod, eb_n0, scale, call=0)
    assert dec.frontend_prefec_counters() == [0, 0, 0, 0]
    dec.close()


# ---- the driver -------------------------------------------------------------------------------------------------------
def _run_sim(tmp_path, eb_n0, args):
    exe = os.path.join(oa.PKG_DIR, "host", "lnsfaid_sim")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    prof = open(os.path.join(oa.PKG_DIR, "host", "Profile.txt")).read()
    prof = prof.replace("StartSNR: 3.3", "StartSNR: %g" % eb_n0).replace("EndSNR: 3.85", "EndSNR: %g" % (eb_n0 + 0.05))
    (tmp_path / "Profile.txt").write_text(prof)
    res = subprocess.run([exe, "--gpus", "1", "--max-rounds", "1"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    demod = (tmp_path / "demod.txt").read_text().splitlines()
    assert demod[0].split() == ["Eb/N0", "ModFER", "ModBER", "ModSER"]
    line = [l for l in res.stdout.splitlines() if l.startswith("pre-FEC counters:")]
    counters = [int(x) for x in re.findall(r"\d+", line[-1])] if line else None
    row = [l for l in res.stdout.splitlines() if re.match(r"\s*%g\s" % eb_n0, l)][-1].split()
    return counters, [float(x) for x in demod[-1].split()[1:]], row


def _quotients(c, K, mod):
    return [c[1] / c[0], c[2] / (c[0] * K), c[3] / (c[0] * K / mod)]


def test_driver_prefec_with_the_device_frontend(abi, lib, code50, tmp_path):
    eb_n0, streams, K = 3.5, 2, code50.K
    counters, demod, row = _run_sim(tmp_path, eb_n0, ["--streams", str(streams), "--device-frontend", "--prefec"])
    print("driver: %s, demod.txt %s" % (counters, demod))
    assert counters[0] == 50 * 32 * streams == int(row[1]) and counters[1] == counters[0] and counters[2] > 0
    want = _quotients(counters, K, 2)
    assert all(d > 0 and abs(d - w) <= 1e-5 * w for d, w in zip(demod, want)), (demod, want)  # (six digits in the file)
    assert [float(x) for x in row[-3:]] == demod  # the same figures at the end of the console row
    # the same 50 calls of the same streams through pyabi
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, streams)
    dec.frontend_set_prefec(pr.INFO)
    for call in range(50):
        _frontend(lib, dec, code50, 2, eb_n0, 13.0, call=call, seeds=[101, 103])
    assert dec.frontend_prefec_counters() == counters
    dec.close()
    # without --prefec the row stays the reference's zeros, and nothing is appended to the console row
    (tmp_path / "demod.txt").unlink()
    counters0, demod0, row0 = _run_sim(tmp_path, eb_n0, ["--streams", str(streams), "--device-frontend"])
    assert counters0 is None and demod0 == [0.0, 0.0, 0.0] and len(row0) == len(row) - 3 and row0[:4] == row[:4]


def test_driver_prefec_with_the_host_frontend(abi, lib, code50, tmp_path):
    eb_n0, N, M = 3.5, code50.N, code50.M
    dump = tmp_path / "symbols.bin"
    counters, demod, row = _run_sim(tmp_path, eb_n0, ["--streams", "1", "--prefec", "--dump-symbols", str(dump)])
    rx = np.fromfile(dump, dtype=np.float32)
    assert rx.size == 50 * 32 * N
    want = abi.prefec_errors_host(N, M, 1, rx, 50, 2, None, pr.INFO, lib)  # FakeEncoder sends the all-zero codeword
    print("driver: %s, host function on its symbols: %s" % (counters, want))
    assert counters == want and want[2] > 0
    assert all(abs(d - w) <= 1e-5 * w for d, w in zip(demod, _quotients(counters, code50.K, 2)))
