"""GPU tests of the device encoder (lnsfaid_encode, lnsfaid_encode_device) and the device frame source
(lnsfaid_frontend_random_frames, lnsfaid_sim --device-encode) against the test encoder (tests/gf2_encoder.py), the numpy
restatement of the message generator (tests/encoder_ref.py) and the oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import encoder_ref as er
import gf2_encoder
import oracle_abi as oa

pytestmark = pytest.mark.gpu

E_CODE = -2
MAX_GROUPS = 96
EXE = os.path.join(oa.PKG_DIR, "host", "lnsfaid_sim")


def _encoded_groups(encoder, info):
    """info [n, 32, K] -> the encoder output layout of n groups, flat"""
    n, _, K = info.shape
    return gf2_encoder.to_group_layout(encoder.encode(info.reshape(n * 32, K)), K)


def _assert_codewords(H, out, n, K, M):
    for g in range(n):
        frames = er.frames_of_group(out[g * 32 * (K + M):(g + 1) * 32 * (K + M)], K, M)
        assert not er.syndromes(H, frames).any(), g


@pytest.fixture(scope="module")
def batch(code50, encoder):
    info = np.random.default_rng(2024).integers(0, 2, size=(MAX_GROUPS, 32, code50.K), dtype=np.int8)
    return info, _encoded_groups(encoder, info)


@pytest.fixture(scope="module")
def H50(code50):
    return er.parity_matrix(code50)


@pytest.mark.parametrize("n", [1, 3, 64, MAX_GROUPS])
def test_encode_host_and_device_pointers(abi, code50, batch, H50, n):
    import torch
    info_all, want_all = batch
    K, N, M = code50.K, code50.N, code50.M
    info = np.ascontiguousarray(info_all[:n].reshape(-1))
    want = want_all[:n * 32 * N]
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, MAX_GROUPS)
    out = d.encode(info, n)
    assert np.array_equal(out, want)
    for g in range(n):  # systematic: the information part is the input
        assert np.array_equal(out[g * 32 * N:g * 32 * N + 32 * K], info[g * 32 * K:(g + 1) * 32 * K])
    _assert_codewords(H50, out, min(n, 3), K, M)
    for off in (0, 1):  # device buffers at any byte offset
        d_in = torch.from_numpy(np.concatenate([np.zeros(off, np.int8), info])).cuda()
        d_out = torch.full((n * 32 * N + off,), 5, dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        d.encode_device(d_in.data_ptr() + off, n, d_out.data_ptr() + off)
        got = d_out.cpu().numpy()
        assert np.array_equal(got[off:], want), off
        assert (got[:off] == 5).all()
    assert d.lib.lnsfaid_encode(d.ctx, None, 0, None) == 0
    assert d.lib.lnsfaid_encode(d.ctx, info.ctypes.data, MAX_GROUPS + 1, out.ctypes.data) == -1
    assert d.lib.lnsfaid_encode_device(d.ctx, None, 1, None) == -1
    d.close()


def _frames_on_device(abi, lib, dec, n, N, torch):
    """the frames the device front-end sends (codeword = NULL) without noise: fixInput = +-7, the sign is the bit"""
    d_fix = torch.empty(n * 32 * N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.lnsfaid_frontend_device(dec.ctx, (C.c_uint32 * n)(*range(1, n + 1)), (C.c_uint64 * n)(*([0] * n)), n, 2, 0.0, 13.0,
                                     None, d_fix.data_ptr())
    assert rc == 0, lib.lnsfaid_last_hip_error()
    return d_fix


def _device_input_bits_equal(abi, lib, dec, code50, info, torch):
    """lnsfaid_frontend_input_bits against `info` [n, 32, K]: count_errors_device of a decodedBits buffer that carries info"""
    n, K, N = info.shape[0], code50.K, code50.N
    d_in = C.c_void_p()
    assert lib.lnsfaid_frontend_input_bits(dec.ctx, C.byref(d_in)) == 0 and d_in.value
    dec_bits = np.zeros((n, 32, N), dtype=np.int8)
    dec_bits[:, :, :K] = info
    d_dec = torch.from_numpy(dec_bits.reshape(-1)).cuda()
    torch.cuda.synchronize()
    same = dec.count_errors_device(d_dec.data_ptr(), d_in.value, n)
    dec_bits[n - 1, 31, K - 1] ^= 1  # one wrong bit is seen
    d_dec = torch.from_numpy(dec_bits.reshape(-1)).cuda()
    torch.cuda.synchronize()
    one = dec.count_errors_device(d_dec.data_ptr(), d_in.value, n)
    return same[1:3] == [0, 0] and one[1:3] == [1, 1]


@pytest.mark.parametrize("n", [2, 64])
def test_random_frames(abi, lib, code50, encoder, n):
    import torch
    K, N, M = code50.K, code50.N, code50.M
    keys = [0x1234_5678_9ABC + 977 * s for s in range(n)]
    info = er.messages(keys, K)
    want = _encoded_groups(encoder, info)
    cfg = abi.default_cfg(2, 10)
    dec = abi.Decoder(code50, cfg, 0, n)
    dec.random_frames(keys)
    assert _device_input_bits_equal(abi, lib, dec, code50, info, torch)
    sent = (_frames_on_device(abi, lib, dec, n, N, torch).cpu().numpy() > 0).astype(np.int8)
    assert np.array_equal(sent, want)
    # the same frames through lnsfaid_frontend_set_frames give the same channel output
    seeds, draws = (C.c_uint32 * n)(*[101 + 2 * s for s in range(n)]), (C.c_uint64 * n)(*([0] * n))
    sigma = oa.load().lnsfaid_frontend_sigma(3.6, 2, oa.ReferenceChannel.RATE)
    d_fix = torch.empty(n * 32 * N, dtype=torch.int8, device="cuda")
    d_fix2 = torch.empty_like(d_fix)
    torch.cuda.synchronize()
    assert lib.lnsfaid_frontend_device(dec.ctx, seeds, draws, n, 2, sigma, 13.0, None, d_fix.data_ptr()) == 0
    d_out = torch.empty(n * 32 * N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    dec.decode_device(d_fix.data_ptr(), n, d_out.data_ptr())
    d_in = C.c_void_p()
    assert lib.lnsfaid_frontend_input_bits(dec.ctx, C.byref(d_in)) == 0
    got = dec.count_errors_device(d_out.data_ptr(), d_in.value, n)
    fix = d_fix.cpu().numpy()
    ref, _ = oa.decode_mt(code50, cfg, fix, n)
    assert got == oa.Oracle(code50, cfg).count_errors(ref, np.ascontiguousarray(info.reshape(-1)), n)
    info_flat = np.ascontiguousarray(info.reshape(-1))
    assert lib.lnsfaid_frontend_set_frames(dec.ctx, want.ctypes.data, info_flat.ctypes.data, n) == 0  # host buffers override
    assert lib.lnsfaid_frontend_device(dec.ctx, seeds, draws, n, 2, sigma, 13.0, None, d_fix2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_fix, d_fix2)
    # random_frames again, then set_frames(NULL): back to the one-codeword mode (all-zero here)
    dec.random_frames(keys)
    assert lib.lnsfaid_frontend_set_frames(dec.ctx, None, None, 0) == 0
    assert lib.lnsfaid_frontend_input_bits(dec.ctx, C.byref(d_in)) == 0 and not d_in.value
    assert not (_frames_on_device(abi, lib, dec, n, N, torch).cpu().numpy() > 0).any()
    assert lib.lnsfaid_frontend_random_frames(dec.ctx, None, 0) == 0
    assert lib.lnsfaid_frontend_random_frames(dec.ctx, None, 1) == -1
    assert lib.lnsfaid_frontend_random_frames(dec.ctx, (C.c_uint64 * (n + 1))(), n + 1) == -1
    dec.close()


def test_random_frames_2048_streams(abi, lib, code50, encoder):
    """Every frame of 2048 streams has zero syndrome (on the GPU: 0/1 half-precision products are exact); 8 groups exactly."""
    import torch
    n, K, N, M = 2048, code50.K, code50.N, code50.M
    keys = [(s * 0x9E3779B97F4A7C15 + 12345) & er.MASK64 for s in range(n)]
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n)
    dec.random_frames(keys)
    fix = _frames_on_device(abi, lib, dec, n, N, torch).view(n, 32 * N)
    Ht = torch.from_numpy(er.parity_matrix(code50).T.copy()).to(device="cuda", dtype=torch.float16)
    for g0 in range(0, n, 256):
        x = fix[g0:g0 + 256]
        frames = torch.cat([x[:, :32 * K].reshape(-1, 32, K), x[:, 32 * K:].reshape(-1, 32, M)], dim=2).reshape(-1, N)
        s = (frames > 0).to(torch.float16) @ Ht
        assert int((s.to(torch.int32) & 1).sum().item()) == 0, g0
    sample = [0, 1, 2, 255, 1024, 1535, 2046, 2047]
    got = (fix[sample].cpu().numpy() > 0).astype(np.int8).reshape(-1)
    assert np.array_equal(got, _encoded_groups(encoder, er.messages([keys[g] for g in sample], K)))
    dec.close()


def test_derived_codes(abi, lib):
    import torch
    dc = er.derived_code(abi, lib, [67, 68], 2)
    assert list(dc.deg) == [23, 22, 21]
    H = er.parity_matrix(dc)
    assert er.gf2_rank(H[:, dc.K:]) == 3072
    enc = gf2_encoder.Encoder(dc)
    info = np.random.default_rng(5).integers(0, 2, size=(3, 32, dc.K), dtype=np.int8)
    d = abi.Decoder(dc, abi.default_cfg(2, 10), 0, 3)
    out = d.encode(np.ascontiguousarray(info.reshape(-1)), 3)
    assert np.array_equal(out, _encoded_groups(enc, info))
    _assert_codewords(H, out, 3, dc.K, dc.M)
    d.close()

    sc = er.derived_code(abi, lib, [68], 11)
    Hs = er.parity_matrix(sc)
    assert er.gf2_rank(Hs[:, sc.K:]) == 3071
    cfg = abi.default_cfg(2, 10)
    d = abi.Decoder(sc, cfg, 0, 3)
    info = np.zeros(3 * 32 * sc.K, dtype=np.int8)
    out = np.zeros(3 * 32 * sc.N, dtype=np.int8)
    d_in = torch.zeros(3 * 32 * sc.K, dtype=torch.int8, device="cuda")
    d_out = torch.zeros(3 * 32 * sc.N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    assert lib.lnsfaid_encode(d.ctx, info.ctypes.data, 3, out.ctypes.data) == E_CODE
    assert lib.lnsfaid_encode_device(d.ctx, d_in.data_ptr(), 3, d_out.data_ptr()) == E_CODE
    assert lib.lnsfaid_frontend_random_frames(d.ctx, (C.c_uint64 * 3)(1, 2, 3), 3) == E_CODE
    fix = oa.synth_llr(3, sc.N, 3.9, seed=31)
    ref, rst = oa.decode_mt(sc, cfg, fix, 3)
    got, st = d.decode(fix, 3)
    d.close()
    assert np.array_equal(got, ref) and np.array_equal(st, rst)


def _run_driver(tmp_path, eb_n0, method, mod_type, scale, interleave, extra):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    prof = open(os.path.join(oa.PKG_DIR, "host", "Profile.txt")).read()
    prof = prof.replace("StartSNR: 3.3", "StartSNR: %g" % eb_n0).replace("EndSNR: 3.85", "EndSNR: %g" % (eb_n0 + 0.05))
    prof = prof.replace("DecodeMethod: 2", "DecodeMethod: %d" % method).replace("modType: 2", "modType: %d" % mod_type)
    prof = prof.replace("scale: 13", "scale: %g" % scale).replace("InterleaveModType: 1", "InterleaveModType: %d" % interleave)
    (tmp_path / "Profile.txt").write_text(prof)
    res = subprocess.run([EXE, "--streams", "2", "--gpus", "1", "--max-rounds", "1"] + extra, cwd=tmp_path, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    row = [l for l in res.stdout.splitlines() if re.match(r"\s*%g\s" % eb_n0, l)][-1].split()
    return [int(row[1]), int(row[2]), int(row[3]), int(row[6])], res.stdout


@pytest.mark.parametrize("method,mod_type,scale,eb_n0,interleave", [(2, 2, 13.0, 3.55, 1), (5, 4, 12.5, 8.1, 4)],
                         ids=["qpsk_faid", "16qam_2b1c_il4"])
def test_host_driver_with_device_encoder(abi, code50, encoder, tmp_path, method, mod_type, scale, eb_n0, interleave):
    """lnsfaid_sim --device-frontend --device-encode: stream s's key is its generator state at the start of the run
    (IX | IY << 16 | IZ << 32, i.e. seed * (1 + 2^16 + 2^32) in round 1); the counters must be the oracle's on the frames
    rebuilt here from the keys."""
    got, out = _run_driver(tmp_path, eb_n0, method, mod_type, scale, interleave, ["--device-frontend", "--device-encode"])
    K = code50.K
    cfg = abi.default_cfg(method, 10)
    want = [0, 0, 0, 0]
    for seed in [101, 103]:
        info = er.messages([seed | seed << 16 | seed << 32], K)
        frames = encoder.encode(info[0])
        fix = oa.ReferenceChannel(code50, seed, scale, mod_type=mod_type, interleave=interleave).groups(eb_n0, 50, frames=frames)
        dec, _ = oa.decode_mt(code50, cfg, fix, 50, kind="avx2")
        c = oa.Oracle(code50, cfg).count_errors(dec, np.ascontiguousarray(np.tile(info.reshape(-1), 50)), 50)
        want = [w + x for w, x in zip(want, c)]
    assert got == want, (got, want, out)
    assert want[0] == 3200
    if method == 2:
        assert want[1] > 0  # the point has frame errors


def test_device_encode_needs_device_frontend(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(oa.PKG_DIR, "host")])
    res = subprocess.run([EXE, "--device-encode"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "usage" in res.stderr
