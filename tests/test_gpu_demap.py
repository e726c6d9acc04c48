"""The demapper for received symbols on the GPU (lnsfaid_demap_device / _packed_device, lnsfaid_demap.hip) against the host
functions of the same library, which tests/test_demap_cpu.py holds against the oracle: byte for byte, on every load / store
path, with guard regions around the outputs; then symbols -> bits through the packed calls with no synchronisation in between."""
import ctypes as C

import numpy as np
import pytest

import demap_ref as dr
import oracle_abi as oa

pytestmark = pytest.mark.gpu

E_INVAL = -1
GUARD, FILL = 64, 0x55
SCALE = {1: 13.0, 2: 13.0, 4: 12.5, 6: 12.5, 8: 40.0}
# Eb/N0 of tests/test_gpu_frontend.py for each order and interleaver
EB_N0 = {(1, 1): 3.6, (2, 1): 3.6, (4, 1): 8.1, (6, 1): 14.0, (8, 1): 19.0, (2, 2): 3.8, (4, 4): 8.6, (6, 3): 14.0, (8, 8): 19.0, (2, 23): 3.8}


def _rx(code50, mod, il, n_groups, seed):
    """noisy constellation points of random bits with the planted values of the CPU tests"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 2, (n_groups, 32, code50.N), dtype=np.int8)
    sigma = oa.load().lnsfaid_frontend_sigma(EB_N0[(mod, il)], mod, oa.ReferenceChannel.RATE)
    rx = dr.noisy_symbols(rng, frames, mod, il, sigma)
    return dr.plant(rx, n_groups, code50.N, code50.M, il, mod, SCALE[mod])


def _device_rx(rx, shift_floats=0):
    import torch
    buf = torch.zeros(rx.size + 4, dtype=torch.float32, device="cuda")
    buf[shift_floats:shift_floats + rx.size] = torch.from_numpy(rx)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * shift_floats


def _demap(dec, packed, rx_ptr, n_groups, mod, size, shift=0):
    """runs the device call into a guarded buffer filled with FILL; returns the output bytes (uint8)"""
    import torch
    buf = torch.full((GUARD + size + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + GUARD + shift
    (dec.demap_packed_device if packed else dec.demap_device)(rx_ptr, n_groups, mod, SCALE[mod], ptr)
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == FILL).all() and (host[GUARD + shift + size:] == FILL).all(), "wrote outside the output"
    return host[GUARD + shift:GUARD + shift + size]


@pytest.mark.parametrize("mod,il", sorted(EB_N0), ids=["m%d_i%d" % k for k in sorted(EB_N0)])
def test_device_equals_host(abi, lib, code50, mod, il):
    n_groups, N, M = 3, code50.N, code50.M
    rx = _rx(code50, mod, il, n_groups, 100 + 10 * mod + il)
    want = abi.demap_host(N, M, il, rx, n_groups, mod, SCALE[mod], lib)
    assert np.array_equal(want, dr.demap(rx, n_groups, N, M, il, mod, SCALE[mod]))  # (the restatement agrees at this size too)
    assert set(np.unique(want).tolist()) == set(range(-7, 8))
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    keep, rx_ptr = _device_rx(rx)
    got = _demap(dec, False, rx_ptr, n_groups, mod, want.size)
    assert np.array_equal(got.view(np.int8), want), np.nonzero(got.view(np.int8) != want)[0][:8]
    got4 = _demap(dec, True, rx_ptr, n_groups, mod, want.size // 2)
    assert np.array_equal(got4, abi.demap_packed_host(N, M, il, rx, n_groups, mod, SCALE[mod], lib))
    assert np.array_equal(got4, abi.pack_llr4(want, lib))
    dec.close()


@pytest.mark.parametrize("mod,il", [(2, 1), (4, 1), (2, 2)], ids=["qpsk", "16qam", "qpsk_il2"])
def test_alignment_selects_the_path_not_the_bytes(abi, lib, code50, mod, il):
    n_groups = 2
    rx = _rx(code50, mod, il, n_groups, 300 + mod + il)
    want = abi.demap_host(code50.N, code50.M, il, rx, n_groups, mod, SCALE[mod], lib)
    want4 = abi.pack_llr4(want, lib)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    for rx_shift in (0, 1, 2):  # floats: 0, 4 and 8 bytes
        keep, rx_ptr = _device_rx(rx, rx_shift)
        for out_shift in (0, 1, 4):
            got = _demap(dec, False, rx_ptr, n_groups, mod, want.size, out_shift)
            assert np.array_equal(got.view(np.int8), want), (rx_shift, out_shift)
        for out_shift in (0, 4):
            assert np.array_equal(_demap(dec, True, rx_ptr, n_groups, mod, want4.size, out_shift), want4), (rx_shift, out_shift)
    dec.close()


def test_symbols_to_bits_without_synchronisation(abi, lib, code50, encoder):
    """demap_packed_device -> decode_packed_device -> count_errors_packed_device on the context's stream; the AVX2 port decodes
    the host demapper's LLRs of the same symbols"""
    import torch
    n_groups, mod, il, K, N = 2, 4, 4, code50.K, code50.N
    rng = np.random.default_rng(41)
    info = rng.integers(0, 2, (n_groups, 32, K), dtype=np.uint8)
    frames = np.stack([encoder.encode(i) for i in info]).astype(np.int8)  # [n_groups, 32, N]
    sigma = oa.load().lnsfaid_frontend_sigma(8.6, mod, oa.ReferenceChannel.RATE)
    rx = dr.noisy_symbols(rng, frames, mod, il, sigma)
    cfg = abi.default_cfg(2, 10)
    dec = abi.Decoder(code50, cfg, 0, n_groups)
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
    d_rx = torch.from_numpy(rx).cuda()
    d_llr4 = torch.zeros(n_groups * 16 * N, dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros(n_groups * N, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((n_groups, 2), dtype=torch.int32, device="cuda")
    info8 = np.ascontiguousarray(info.reshape(-1).astype(np.int8))
    d_msg = torch.from_numpy(abi.pack_bits(info8, lib)).cuda()
    torch.cuda.synchronize()
    dec.demap_packed_device(d_rx.data_ptr(), n_groups, mod, SCALE[mod], d_llr4.data_ptr())
    dec.decode_packed_device(d_llr4.data_ptr(), n_groups, d_bits.data_ptr(), d_st.data_ptr())
    counters = dec.count_errors_packed_device(d_bits.data_ptr(), d_msg.data_ptr(), n_groups)
    fix = abi.demap_host(N, code50.M, il, rx, n_groups, mod, SCALE[mod], lib)
    assert np.array_equal(d_llr4.cpu().numpy(), abi.pack_llr4(fix, lib))
    assert fix.any() and (np.abs(fix) < 7).any()  # neither all zero nor all saturated
    ref, ref_stats = oa.decode_mt(code50, cfg, fix, n_groups, kind="avx2")
    assert np.array_equal(abi.unpack_bits(d_bits.cpu().numpy().view(np.uint32), lib), ref)
    assert np.array_equal(d_st.cpu().numpy(), ref_stats)
    assert counters == oa.Oracle(code50, cfg).count_errors(ref, info8, n_groups)
    dec.close()


def test_limits(abi, lib, code50):
    import torch
    n_groups, N, M = 2, code50.N, code50.M
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, n_groups)
    rx = _rx(code50, 2, 1, n_groups, 7)
    d_rx = torch.from_numpy(np.concatenate([rx, rx[:32 * N]])).cuda()  # room for a third group
    d_out = torch.full((3 * 32 * N + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rxp, outp = d_rx.data_ptr(), d_out.data_ptr()
    for fn in (lib.lnsfaid_demap_device, lib.lnsfaid_demap_packed_device):
        assert fn(dec.ctx, rxp, n_groups + 1, 2, 13.0, outp) == E_INVAL      # above max_groups
        assert fn(dec.ctx, rxp + 2, n_groups, 2, 13.0, outp) == E_INVAL      # d_rx not 4-byte aligned
        assert fn(dec.ctx, None, n_groups, 2, 13.0, outp) == E_INVAL and fn(dec.ctx, rxp, n_groups, 2, 13.0, None) == E_INVAL
        assert fn(dec.ctx, rxp, n_groups, 3, 13.0, outp) == E_INVAL
        assert fn(dec.ctx, None, 0, 2, 13.0, None) == 0
        assert fn(None, rxp, n_groups, 2, 13.0, outp) == E_INVAL
    assert lib.lnsfaid_demap_packed_device(dec.ctx, rxp, n_groups, 2, 13.0, outp + 2) == E_INVAL  # d_llr4 not 4-byte aligned
    torch.cuda.synchronize()
    assert int((d_out != FILL).sum().item()) == 0  # a refused call writes nothing
    # the interleaver of the context: 7 does not divide n_var and leaves the value alone; 3 applies to the demap calls
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, 7) != 0
    assert lib.lnsfaid_frontend_set_interleave(dec.ctx, 3) == 0
    dec.demap_device(rxp, n_groups, 2, 13.0, outp)
    got = d_out.cpu().numpy()[:n_groups * 32 * N].view(np.int8)
    assert np.array_equal(got, abi.demap_host(N, M, 3, rx, n_groups, 2, 13.0, lib))
    assert not np.array_equal(got, abi.demap_host(N, M, 1, rx, n_groups, 2, 13.0, lib))
    dec.close()
