"""Packed decode I/O on the GPU (lnsfaid_decode*_packed*, lnsfaid_count_errors_packed*, lnsfaid_kernel4p.hip): every case decodes
the same batch through the int8 path and the packed path; the unpacked packed decisions must equal the int8 decisions byte for
byte, and group stats, per-codeword stats and counters must be equal."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

CODEWORD = 1
E_INVAL = -1


def _unpack(abi, bits):
    return abi.unpack_bits(bits)


def _same_group_rule(abi, dec, fix, ng):
    """lnsfaid_decode against lnsfaid_decode_packed on one context; returns the int8 result"""
    out8, st8 = dec.decode(fix, ng)
    bits, stp = dec.decode_packed(abi.pack_llr4(fix), ng)
    assert bits.size == ng * 32 * dec.code50.N // 32
    assert np.array_equal(_unpack(abi, bits), out8), np.nonzero((_unpack(abi, bits) != out8))[0][:8]
    assert np.array_equal(stp, st8), (stp.tolist(), st8.tolist())
    return out8, st8


def _same_codeword_rule(abi, dec, fix, ng):
    out8, cw8 = dec.decode_codewords(fix, ng)
    bits, cwp = dec.decode_codewords_packed(abi.pack_llr4(fix), ng)
    assert np.array_equal(_unpack(abi, bits), out8)
    assert np.array_equal(cwp, cw8)
    return out8, cw8


def _cfg(abi, method):
    cfg = abi.default_cfg(method, 10)
    if method == 0:
        cfg.factor_1 = cfg.factor_2 = 24  # one normalisation factor: the four-rows kernel (two factors: test_fallbacks)
    return cfg


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("eb", [3.0, 3.6, 4.2])
def test_methods_on_qpsk(abi, code50, method, eb):
    ng = 64 if eb == 3.6 else 16
    fix = oa.ReferenceChannel(code50, 211 + method, 13.0).groups(eb, ng)
    dec = abi.Decoder(code50, _cfg(abi, method), 0, ng)
    assert dec.rows_per_lane() == 4
    _, st = _same_group_rule(abi, dec, fix, ng)
    _same_codeword_rule(abi, dec, fix, ng)
    dec.close()
    if eb == 3.6 and method != 0:
        # a mixed batch: some groups stop early (parking, relaunches), some run all layered iterations
        assert (st[:, 0] < 10).any() and (st[:, 0] == 10).any(), st.tolist()


def test_method_5_on_16qam(abi, code50):
    fix = oa.ReferenceChannel(code50, 223, 12.5, mod_type=4).groups(8.1, 16)
    dec = abi.Decoder(code50, abi.default_cfg(5, 10), 0, 16)
    _same_group_rule(abi, dec, fix, 16)
    _same_codeword_rule(abi, dec, fix, 16)
    dec.close()


@pytest.mark.parametrize("method", [1, 2, 5])
@pytest.mark.parametrize("store", [1, 2])  # MSG_REGISTERS, MSG_HBM
def test_message_stores(abi, code50, method, store):
    fix = oa.ReferenceChannel(code50, 227 + method, 13.0).groups(3.5, 16)
    dec = abi.Decoder(code50, abi.default_cfg(method, 10), 0, 16)
    dec.select_message_store(store)
    assert dec.message_store() == store
    _same_group_rule(abi, dec, fix, 16)
    _same_codeword_rule(abi, dec, fix, 16)
    dec.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_ef_elimination(abi, lib, code50, mode):
    cfg = abi.default_cfg(2, 10)
    assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), mode) == 0
    fix = oa.ReferenceChannel(code50, 233, 13.0).groups(3.5, 16)
    dec = abi.Decoder(code50, cfg, 0, 16)
    _same_group_rule(abi, dec, fix, 16)
    _same_codeword_rule(abi, dec, fix, 16)
    dec.close()


def _fallback_cases(abi):
    nms = abi.default_cfg(0, 10)
    nms.factor_1, nms.factor_2 = 24, 26  # two factors: the two-rows kernel
    table = abi.default_cfg(2, 10)
    table.v2c_map[0][1][3] = 3  # weight classes differ: the two-rows kernel
    return [("nms_24_26", nms, 0), ("table", table, 0), ("nms_default", abi.default_cfg(0, 10), 0),
            ("two_waves", abi.default_cfg(2, 10), 2)]


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_fallbacks(abi, lib, code50, case):
    import torch
    name, cfg, waves = _fallback_cases(abi)[case]
    ng = 8
    fix = oa.ReferenceChannel(code50, 239 + case, 13.0).groups(3.6, ng)
    dec = abi.Decoder(code50, cfg, 0, ng)
    if waves:
        dec.select_waves(waves)
        assert dec.kernel_waves() == 2
    else:
        assert dec.rows_per_lane() == 2, name
    out8, st8 = _same_group_rule(abi, dec, fix, ng)
    llr4 = abi.pack_llr4(fix)
    d_in = torch.from_numpy(llr4).cuda()
    d_bits = torch.zeros(ng * 32 * code50.N // 32, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((ng, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_packed_device(d_in.data_ptr(), ng, d_bits.data_ptr(), d_st.data_ptr())
    assert np.array_equal(_unpack(abi, d_bits.cpu().numpy().view(np.uint32)), out8)
    assert np.array_equal(d_st.cpu().numpy(), st8)
    # no per-codeword decoder for these configurations: E_INVAL, as the int8 calls
    bits = np.zeros(ng * 32 * code50.N // 32, np.uint32)
    assert lib.lnsfaid_decode_codewords_packed(dec.ctx, llr4.ctypes.data, ng, bits.ctypes.data, None) == E_INVAL
    assert lib.lnsfaid_decode_codewords_packed_device(dec.ctx, d_in.data_ptr(), ng, d_bits.data_ptr(), None) == E_INVAL
    dec.set_early_stop(CODEWORD)
    assert lib.lnsfaid_decode_packed(dec.ctx, llr4.ctypes.data, ng, bits.ctypes.data, None) == E_INVAL
    assert lib.lnsfaid_decode_packed_device(dec.ctx, d_in.data_ptr(), ng, d_bits.data_ptr(), None) == E_INVAL
    out = np.empty(fix.size, np.int8)
    assert lib.lnsfaid_decode(dec.ctx, fix.ctypes.data, ng, out.ctypes.data, None) == E_INVAL
    dec.close()


def test_derived_code_with_runtime_row_degree(abi, lib):
    from test_gpu_more import _derived_code
    dc = _derived_code(abi, lib, [67, 68], 2)
    assert list(dc.deg) == [23, 22, 21]
    fix = oa.synth_llr(16, dc.N, 3.9, seed=29)
    dec = abi.Decoder(dc, abi.default_cfg(2, 10), 0, 16)
    _same_group_rule(abi, dec, fix, 16)
    _same_codeword_rule(abi, dec, fix, 16)
    dec.close()


@pytest.mark.parametrize("method", [1, 2, 5])
def test_random_int8_with_minus_8(abi, code50, method):
    rng = np.random.default_rng(31 + method)
    fix = rng.integers(-8, 8, size=8 * 32 * code50.N, dtype=np.int8)
    fix[:64] = -8
    dec = abi.Decoder(code50, abi.default_cfg(method, 10), 0, 8)
    _same_group_rule(abi, dec, fix, 8)
    _same_codeword_rule(abi, dec, fix, 8)
    dec.close()


def test_one_group_against_the_scalar_oracle(abi, code50):
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 241, 13.0).groups(3.6, 1)
    ref, rst = oa.Oracle(code50, cfg).decode(fix, 1)
    dec = abi.Decoder(code50, cfg, 0, 1)
    bits, st = dec.decode_packed(abi.pack_llr4(fix), 1)
    dec.close()
    assert np.array_equal(_unpack(abi, bits), ref)
    assert np.array_equal(st, rst)


@pytest.mark.parametrize("kind", ["pageable", "pinned", "registered"])
def test_host_path_in_pieces(abi, lib, code50, kind):
    import torch
    ng = 256  # several pieces of 64 groups on the pinned / registered path
    cfg = abi.default_cfg(2, 10)
    fix = oa.synth_llr(ng, code50.N, 3.6, seed=43)
    dec = abi.Decoder(code50, cfg, 0, ng)
    out8, st8 = dec.decode(fix, ng)
    cout8, cw8 = dec.decode_codewords(fix, ng)
    llr4 = abi.pack_llr4(fix)
    n_words = ng * 32 * code50.N // 32
    keep = []
    if kind == "pageable":
        src, dst, dst2 = llr4, np.zeros(n_words, np.uint32), np.zeros(n_words, np.uint32)
    elif kind == "pinned":
        t_in = torch.from_numpy(llr4).pin_memory()
        t_out = torch.zeros(n_words, dtype=torch.int32).pin_memory()
        t_out2 = torch.zeros(n_words, dtype=torch.int32).pin_memory()
        keep = [t_in, t_out, t_out2]
        src, dst, dst2 = t_in.numpy(), t_out.numpy().view(np.uint32), t_out2.numpy().view(np.uint32)
    else:
        src, dst, dst2 = llr4.copy(), np.zeros(n_words, np.uint32), np.zeros(n_words, np.uint32)
        for a in (src, dst, dst2):
            assert lib.lnsfaid_host_register(a.ctypes.data, a.nbytes) == 0
    try:
        st = np.zeros((ng, 2), np.int32)
        cw = np.zeros((ng * 32, 3), np.int32)
        assert lib.lnsfaid_decode_packed(dec.ctx, src.ctypes.data, ng, dst.ctypes.data, st.ctypes.data) == 0
        assert lib.lnsfaid_decode_codewords_packed(dec.ctx, src.ctypes.data, ng, dst2.ctypes.data, cw.ctypes.data) == 0
        got, got2 = _unpack(abi, dst), _unpack(abi, dst2)
    finally:
        if kind == "registered":
            for a in (src, dst, dst2):
                lib.lnsfaid_host_unregister(a.ctypes.data)
    dec.close()
    del keep
    assert np.array_equal(got, out8) and np.array_equal(st, st8)
    assert np.array_equal(got2, cout8) and np.array_equal(cw, cw8)


def test_device_path_with_codeword_offsets(abi, code50):
    import torch
    ng, N = 16, code50.N
    fix = oa.ReferenceChannel(code50, 251, 13.0).groups(3.6, ng)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, ng)
    out8, st8 = dec.decode(fix, ng)
    cout8, cw8 = dec.decode_codewords(fix, ng)
    llr4 = abi.pack_llr4(fix)
    pad_in, pad_out = 3 * N // 2, 5 * N // 32  # three codewords of llr4 (bytes), five codewords of bits (words)
    d_in = torch.zeros(pad_in + llr4.size, dtype=torch.uint8, device="cuda")
    d_in[pad_in:] = torch.from_numpy(llr4).cuda()
    d_bits = torch.zeros(pad_out + ng * N, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((ng, 2), dtype=torch.int32, device="cuda")
    d_cw = torch.zeros((ng * 32, 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    in_p, out_p = d_in.data_ptr() + pad_in, d_bits.data_ptr() + 4 * pad_out
    dec.decode_packed_device(in_p, ng, out_p, d_st.data_ptr())
    got = d_bits[pad_out:].cpu().numpy().view(np.uint32)
    assert np.array_equal(_unpack(abi, got), out8) and np.array_equal(d_st.cpu().numpy(), st8)
    assert (d_bits[:pad_out].cpu().numpy() == 0).all()  # nothing written in front of the output
    dec.decode_codewords_packed_device(in_p, ng, out_p, d_cw.data_ptr())
    got = d_bits[pad_out:].cpu().numpy().view(np.uint32)
    assert np.array_equal(_unpack(abi, got), cout8) and np.array_equal(d_cw.cpu().numpy(), cw8)
    # the packed counters on the device output against the int8 counters on the int8 output
    want = dec.count_errors(cout8, None, ng)
    assert dec.count_errors_packed_device(out_p, None, ng) == want
    dec.close()


def test_argument_checks_with_a_context(abi, lib, code50):
    import torch
    ng = 2
    fix = oa.ReferenceChannel(code50, 257, 13.0).groups(3.6, ng)
    llr4 = abi.pack_llr4(fix)
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), 0, ng)
    d_in = torch.from_numpy(np.concatenate([llr4, np.zeros(16, np.uint8)])).cuda()
    d_bits = torch.zeros(ng * code50.N + 4, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((ng, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = (C.c_uint64 * 4)()
    for fn in (lib.lnsfaid_decode_packed_device, lib.lnsfaid_decode_codewords_packed_device):
        assert fn(dec.ctx, d_in.data_ptr() + 1, ng, d_bits.data_ptr(), None) == E_INVAL  # misaligned input
        assert fn(dec.ctx, d_in.data_ptr() + 2, ng, d_bits.data_ptr(), None) == E_INVAL
        assert fn(dec.ctx, d_in.data_ptr(), ng, d_bits.data_ptr() + 2, None) == E_INVAL  # misaligned output
        assert fn(dec.ctx, None, ng, d_bits.data_ptr(), None) == E_INVAL
        assert fn(dec.ctx, d_in.data_ptr(), ng, None, None) == E_INVAL
        assert fn(dec.ctx, d_in.data_ptr(), ng + 1, d_bits.data_ptr(), None) == E_INVAL  # above max_groups
        assert fn(dec.ctx, None, 0, None, None) == 0  # no-op
    assert lib.lnsfaid_decode_packed_device(dec.ctx, d_in.data_ptr(), ng, d_bits.data_ptr(), d_st.data_ptr() + 2) == E_INVAL
    bits = np.zeros(ng * code50.N, np.uint32)
    for fn in (lib.lnsfaid_decode_packed, lib.lnsfaid_decode_codewords_packed):
        assert fn(dec.ctx, None, ng, bits.ctypes.data, None) == E_INVAL
        assert fn(dec.ctx, llr4.ctypes.data, ng, None, None) == E_INVAL
        assert fn(dec.ctx, llr4.ctypes.data, ng + 1, bits.ctypes.data, None) == E_INVAL
        assert fn(dec.ctx, None, 0, None, None) == 0
    # host pointers may have any alignment
    odd_in = np.zeros(llr4.size + 1, np.uint8)
    odd_in[1:] = llr4
    odd_out = np.zeros(bits.nbytes + 1, np.uint8)
    assert lib.lnsfaid_decode_packed(dec.ctx, odd_in.ctypes.data + 1, ng, odd_out.ctypes.data + 1, None) == 0
    assert np.array_equal(_unpack(abi, np.frombuffer(odd_out[1:].tobytes(), np.uint32)), dec.decode(fix, ng)[0])
    assert lib.lnsfaid_count_errors_packed_device(dec.ctx, d_bits.data_ptr() + 2, None, ng, out) == E_INVAL
    assert lib.lnsfaid_count_errors_packed_device(dec.ctx, d_bits.data_ptr(), d_in.data_ptr() + 1, ng, out) == E_INVAL
    assert lib.lnsfaid_count_errors_packed_device(dec.ctx, None, None, ng, out) == E_INVAL
    assert lib.lnsfaid_count_errors_packed_device(dec.ctx, d_bits.data_ptr(), None, ng, None) == E_INVAL
    assert lib.lnsfaid_count_errors_packed(dec.ctx, bits.ctypes.data, None, ng + 1, out) == E_INVAL
    assert lib.lnsfaid_count_errors_packed(dec.ctx, None, None, 0, out) == 0 and list(out) == [0, 0, 0, 0]
    dec.close()


def test_one_group_contexts_from_threads(abi, code50):
    n_threads, n_calls = 4, 3
    cfg = abi.default_cfg(2, 10)
    fixes = [oa.ReferenceChannel(code50, 600 + t, 13.0).groups(3.6, n_calls).reshape(n_calls, -1) for t in range(n_threads)]
    single = abi.Decoder(code50, cfg, 0, 1)
    refs = [[single.decode_packed(abi.pack_llr4(fixes[t][c]), 1) for c in range(n_calls)] for t in range(n_threads)]
    int8 = [[single.decode(np.ascontiguousarray(fixes[t][c]), 1) for c in range(n_calls)] for t in range(n_threads)]
    single.close()
    for t in range(n_threads):
        for c in range(n_calls):
            assert np.array_equal(_unpack(abi, refs[t][c][0]), int8[t][c][0])
    errors = []
    start = threading.Barrier(n_threads)

    def worker(t):
        try:
            dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
            start.wait()
            for rep in range(2):
                for c in range(n_calls):
                    bits, st = dec.decode_packed(abi.pack_llr4(fixes[t][c]), 1)
                    if not np.array_equal(bits, refs[t][c][0]) or not np.array_equal(st, refs[t][c][1]):
                        errors.append((t, rep, c))
            dec.close()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in threads)
    assert not errors, errors[:4]


def _frames_with_errors(code50, info, parity, ng, rng):
    """decodedBits of ng groups: codeword = its information bits then its parity bits; frame i has i % 5 information bits
    flipped (0 .. 4: both sides of the LT3 boundary) and a few parity bits flipped (not counted)"""
    K, N = code50.K, code50.N
    dec = np.concatenate([info.reshape(-1, K), parity.reshape(-1, N - K)], axis=1).copy()
    errs = np.arange(ng * 32) % 5
    for i in range(ng * 32):
        pos = rng.choice(K, errs[i], replace=False)
        dec[i, pos] ^= 1
        dec[i, K + rng.choice(N - K, 3, replace=False)] ^= 1
    want = [ng * 32, int((errs > 0).sum()), int(errs.sum()), int(((errs > 0) & (errs < 3)).sum())]
    return np.ascontiguousarray(dec.reshape(-1)).astype(np.int8), want


@pytest.mark.parametrize("msg_kind", ["null", "encoder"])
def test_packed_counters(abi, code50, msg_kind):
    import torch
    ng, K, N, M = 4, code50.K, code50.N, code50.M
    rng = np.random.default_rng(47)
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, ng)
    if msg_kind == "null":
        info = np.zeros(ng * 32 * K, np.int8)
        parity = np.zeros(ng * 32 * M, np.int8)
    else:
        info = rng.integers(0, 2, size=ng * 32 * K, dtype=np.int8)
        frames = d.encode(info, ng).reshape(ng, 32 * N)  # [32][K] then [32][M] per group
        assert np.array_equal(frames[:, :32 * K].reshape(-1), info)
        parity = np.ascontiguousarray(frames[:, 32 * K:]).reshape(-1)
    decoded, want = _frames_with_errors(code50, info, parity, ng, rng)
    msg8 = info if msg_kind == "encoder" else None
    got8 = d.count_errors(decoded, msg8, ng)
    assert got8 == want
    bits = np.packbits(decoded.view(np.uint8), bitorder="little").view("<u4")
    msgp = abi.pack_bits(info) if msg_kind == "encoder" else None
    assert d.count_errors_packed(bits, msgp, ng) == got8
    d_bits = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    d_msg = torch.from_numpy(msgp).cuda() if msgp is not None else None
    torch.cuda.synchronize()
    assert d.count_errors_packed_device(d_bits.data_ptr(), d_msg.data_ptr() if d_msg is not None else None, ng) == got8
    d.close()
