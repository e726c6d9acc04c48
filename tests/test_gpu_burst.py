"""Burst-format line calls on the GPU (include/lnsfaid.h "burst-format line calls", DESIGN.md §3.18, lnsfaid_kernel4b.hip,
lnsfaid_encoder_burst.hip).  The definition of the decode is lnsfaid_burst_to_llr4: for every codeword lnsfaid_decode_burst* must
return what lnsfaid_decode_codewords_packed_device returns for that llr4 - bits, iterations, bf_iterations, unsatisfied - the
information words minus the known ones as payload, and the two counts of tests/burst_ref.py; the definition of the encode is
lnsfaid_encode_burst_host.  Inputs are random messages with zeros in the known range, encoded with tests/gf2_encoder.py (never the
all-zero frame); every device output lies between 64 guard words in front and 64 behind, which must keep their pattern."""
import ctypes as C

import numpy as np
import pytest

import burst_ref as br
import line_ref as lr

pytestmark = pytest.mark.gpu

HARD, LLR4, TAIL, HEAD = br.HARD, br.LLR4, br.TAIL, br.HEAD
E_INVAL = -1
MAX_ITER = 10
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32
EB_N0 = 3.4           # as tests/test_gpu_line.py: early stops, failures and stops inside the bit-flipping stage
WHERES = pytest.mark.parametrize("where", [TAIL, HEAD], ids=["tail", "head"])
FORMATS = pytest.mark.parametrize("fmt,magnitude", [(HARD, 4), (LLR4, 0)], ids=["hard4", "llr4"])

_batches = {}


def _dims(code):
    N, K = code.n_var, code.n_var - code.n_check
    return N, K, N - code.puncture_tail


def _batch(encoder, name, n, fmt, where):
    """(shortened, burst line, messages, kind, flips, codewords), built once per key and never changed"""
    key = (name, n, fmt, where)
    if key not in _batches:
        s = br.batch(name, n)
        _batches[key] = (s,) + br.planted_burst(encoder, n, encoder.N - 384, fmt, 1, s, where, eb_n0=EB_N0)
    return _batches[key]


def _cfg(abi, method):
    cfg = abi.default_cfg(method, MAX_ITER)
    if method == 0:
        cfg.factor_1 = cfg.factor_2 = 24  # one normalisation factor: the four-rows kernel
    return cfg


def _guarded(torch, n_words):
    t = torch.full((GUARD + n_words + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 4 * GUARD


def _inside(t, n_words):
    """the words between the guards, after checking both guards"""
    h = t.cpu().numpy()
    assert (h[:GUARD] == PATTERN).all() and (h[GUARD + n_words:] == PATTERN).all(), "a guard word was overwritten"
    return h[GUARD:GUARD + n_words].view(np.uint32)


def _to_device(torch, a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, n, with_bits=True, with_stats=True, with_ones=True):
    """lnsfaid_decode_burst_device on a device copy of exactly the burst line's size -> (payload, bits [n, N / 32], stats, short_ones),
    an output that was not passed being the untouched buffer; the guards of all four are checked"""
    import torch
    code = dec.code50.code
    N, K, L = _dims(code)
    _, payload_bits = br.burst_words(n, K, L, np.zeros(n) if s is None else s)
    pw, nw = payload_bits // 32, N // 32
    d_line = _to_device(torch, line)
    d_pay, p_pay = _guarded(torch, pw)
    d_bits, p_bits = _guarded(torch, n * nw)
    d_st, p_st = _guarded(torch, n * 4)
    d_ones, p_ones = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.decode_burst_device(d_line.data_ptr(), fmt, s, where, n, p_pay, p_bits if with_bits else None, p_st if with_stats else None,
                            p_ones if with_ones else None, magnitude)
    return (_inside(d_pay, pw), _inside(d_bits, n * nw).reshape(n, nw), _inside(d_st, n * 4).view(abi.line_stats_dtype()),
            _inside(d_ones, n))


def _reference(abi, lib, dec, line, fmt, magnitude, s, where, n):
    """lnsfaid_decode_codewords_packed_device and lnsfaid_fec_status_packed_host on lnsfaid_burst_to_llr4's output"""
    import torch
    code = dec.code50.code
    N, ng = code.n_var, (n + 31) // 32
    llr4 = abi.burst_to_llr4(code, line, fmt, magnitude, s, where, n, lib)
    d_llr4 = torch.from_numpy(llr4).cuda()
    d_bits = torch.zeros(ng * 32 * N // 32, dtype=torch.int32, device="cuda")
    d_cw = torch.zeros((ng * 32, 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_codewords_packed_device(d_llr4.data_ptr(), ng, d_bits.data_ptr(), d_cw.data_ptr())
    bits = d_bits.cpu().numpy().view(np.uint32)
    rec, _, _ = abi.fec_status_packed_host(code, llr4, bits, None, ng, out=None, lib=lib)
    cw = d_cw.cpu().numpy()
    assert np.array_equal(rec["unsatisfied"][:n], cw[:n, 2])
    return bits.reshape(ng * 32, N // 32)[:n], cw[:n], rec["corrected"][:n].astype(np.int64)


def _assert_equal(abi, lib, dec, line, fmt, magnitude, s, where, n):
    N, K, L = _dims(dec.code50.code)
    want_bits, want_cw, fec_corrected = _reference(abi, lib, dec, line, fmt, magnitude, s, where, n)
    payload, bits, st, ones = _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, n)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, ("bits", bad[:8])
    assert np.array_equal(payload, br.payload_of_bits(want_bits, K, s, where))
    for i, name in enumerate(("iterations", "bf_iterations", "unsatisfied")):
        assert np.array_equal(st[name], want_cw[:, i]), (name, st[name][:8].tolist(), want_cw[:8, i].tolist())
    want_corrected, want_ones = br.counts(want_bits, line, N, K, L, fmt, s, where)
    assert np.array_equal(st["corrected"], want_corrected), (st["corrected"][:8].tolist(), want_corrected[:8].tolist())
    assert np.array_equal(ones, want_ones), (ones[:8].tolist(), want_ones[:8].tolist())
    # the FEC status counts every position below L, the known ones included: a known -7 decided as 1 is a "corrected" bit there
    assert np.array_equal(st["corrected"].astype(np.int64) + ones, fec_corrected)
    return payload, bits, st, ones


def _assert_mixed(st, method):
    """the batch holds a failure (the planted random words) and - where the method has an early stop at all: DecodeMethod 0 has
    none, as in tests/test_gpu_line.py - an early stop (the words received as sent)"""
    assert (st["unsatisfied"] > 0).any(), st["unsatisfied"].tolist()
    if method != 0:
        assert (st["iterations"] < MAX_ITER).any(), st["iterations"].tolist()


@WHERES
@FORMATS
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5])
def test_equivalence(abi, lib, code50, encoder, method, fmt, magnitude, where):
    s, line, msg, kind, flips, cw = _batch(encoder, "cycle", 33, fmt, where)
    dec = abi.Decoder(code50, _cfg(abi, method), 0, 2)
    assert dec.rows_per_lane() == 4
    _, _, st, _ = _assert_equal(abi, lib, dec, line, fmt, magnitude, s, where, 33)
    dec.close()
    _assert_mixed(st, method)


@WHERES
@FORMATS
@pytest.mark.parametrize("name,n", [("burst", 33), ("cycle", 1), ("cycle", 65)], ids=["burst33", "one", "cycle65"])
def test_equivalence_other_batches(abi, lib, code50, encoder, name, n, fmt, magnitude, where):
    s, line, msg, kind, flips, cw = _batch(encoder, name, n, fmt, where)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 3)
    _, _, st, _ = _assert_equal(abi, lib, dec, line, fmt, magnitude, s, where, n)
    dec.close()
    if n >= 33:
        _assert_mixed(st, 2)


@WHERES
@FORMATS
@pytest.mark.parametrize("store", [1, 2], ids=["registers", "hbm"])  # MSG_REGISTERS, MSG_HBM
def test_message_stores(abi, lib, code50, encoder, store, fmt, magnitude, where):
    s, line, _, _, _, _ = _batch(encoder, "cycle", 33, fmt, where)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    dec.select_message_store(store)
    assert dec.message_store() == store
    _, _, st, _ = _assert_equal(abi, lib, dec, line, fmt, magnitude, s, where, 33)
    dec.close()
    _assert_mixed(st, 2)


@WHERES
@FORMATS
def test_ef_elimination_2(abi, lib, code50, encoder, fmt, magnitude, where):
    cfg = abi.default_cfg(2, MAX_ITER)
    assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), 2) == 0
    s, line, _, _, _, _ = _batch(encoder, "cycle", 33, fmt, where)
    dec = abi.Decoder(code50, cfg, 0, 2)
    _, _, st, _ = _assert_equal(abi, lib, dec, line, fmt, magnitude, s, where, 33)
    dec.close()
    _assert_mixed(st, 2)


@FORMATS
def test_no_shortening_is_the_line_decode(abi, code50, encoder, fmt, magnitude):
    """shortened = None and an explicit all-zero array: byte for byte lnsfaid_decode_line_device, short_ones all 0"""
    import torch
    n = 33
    N, K, L = _dims(code50.code)
    line, _, _, _ = lr.planted_batch(encoder, n, L, fmt, 1, eb_n0=EB_N0)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    d_line = _to_device(torch, line)
    d_pay, p_pay = _guarded(torch, n * K // 32)
    d_bits, p_bits = _guarded(torch, n * N // 32)
    d_st, p_st = _guarded(torch, n * 4)
    torch.cuda.synchronize()
    dec.decode_line_device(d_line.data_ptr(), fmt, n, p_pay, p_bits, p_st, magnitude)
    want = [_inside(d_pay, n * K // 32), _inside(d_bits, n * N // 32), _inside(d_st, n * 4)]
    for where in (TAIL, HEAD):
        for s in (None, np.zeros(n, np.uint32)):
            payload, bits, st, ones = _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, n)
            assert payload.tobytes() == want[0].tobytes() and bits.tobytes() == want[1].tobytes()
            assert st.tobytes() == want[2].tobytes() and not ones.any()
    dec.close()


@WHERES
@FORMATS
def test_optional_outputs_and_nothing_outside(abi, lib, code50, encoder, fmt, magnitude, where):
    """an output that is not passed keeps its pattern and the others do not change; every word of every present output is written;
    the guards (checked by _inside) keep theirs"""
    s, line, _, _, _, _ = _batch(encoder, "cycle", 33, fmt, where)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    payload, bits, st, ones = _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, 33)
    for out in (payload, bits, st.view(np.uint32), ones):
        assert not (out.view(np.int32) == PATTERN).any()
    for wb, ws, wo in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        p1, b1, s1, o1 = _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, 33, wb, ws, wo)
        assert np.array_equal(p1, payload)
        assert np.array_equal(b1, bits) if wb else (b1.view(np.int32) == PATTERN).all()
        assert np.array_equal(s1, st) if ws else (s1.view(np.int32) == PATTERN).all()
        assert np.array_equal(o1, ones) if wo else (o1.view(np.int32) == PATTERN).all()
    dec.close()


@WHERES
@FORMATS
def test_host_form(abi, lib, code50, encoder, fmt, magnitude, where):
    n = 33
    s, line, _, _, _, _ = _batch(encoder, "cycle", n, fmt, where)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    payload, bits, st, ones = _decode_burst_device(abi, dec, line, fmt, magnitude, s, where, n)
    h_pay, h_bits, h_st, h_ones = dec.decode_burst(line, fmt, s, where, n, magnitude, with_bits=True)
    assert np.array_equal(h_pay, payload) and np.array_equal(h_bits, bits) and np.array_equal(h_st, st) and np.array_equal(h_ones, ones)
    h_pay, h_bits, h_st, h_ones = dec.decode_burst(line, fmt, s, where, n, magnitude, with_bits=False, with_stats=False, with_ones=False)
    assert np.array_equal(h_pay, payload) and h_bits is None and h_st is None and h_ones is None
    # host pointers of any alignment: every buffer, `shortened` included, at an odd address
    def odd_copy(a):
        o = np.zeros(a.nbytes + 1, np.uint8)
        o[1:] = a.view(np.uint8).reshape(-1)
        return o
    odd_in, odd_s = odd_copy(line), odd_copy(s)
    odd_pay, odd_bits, odd_st, odd_ones = (np.full(a.nbytes + 2, 0x5A, np.uint8) for a in (payload, bits, st, ones))
    assert lib.lnsfaid_decode_burst(dec.ctx, odd_in.ctypes.data + 1, fmt, magnitude, odd_s.ctypes.data + 1, where, n, odd_pay.ctypes.data + 1,
                                    odd_bits.ctypes.data + 1, odd_st.ctypes.data + 1, odd_ones.ctypes.data + 1) == 0
    for odd, want in ((odd_pay, payload), (odd_bits, bits), (odd_st, st), (odd_ones, ones)):
        assert odd[0] == 0x5A and odd[-1] == 0x5A and odd[1:-1].tobytes() == want.tobytes()
    if fmt == HARD:  # the encode's host form the same way, on the decoded (or any) payload
        want_line, want_bits = abi.encode_burst_host(code50.code, payload, s, where, n, True, lib)
        e_line, e_bits = dec.encode_burst(payload, s, where, n, with_bits=True)
        assert np.array_equal(e_line, want_line) and np.array_equal(e_bits, want_bits)
        odd_p = odd_copy(payload)
        odd_l, odd_b = (np.full(a.nbytes + 2, 0x5A, np.uint8) for a in (want_line, want_bits))
        assert lib.lnsfaid_encode_burst(dec.ctx, odd_p.ctypes.data + 1, odd_s.ctypes.data + 1, where, n, odd_l.ctypes.data + 1,
                                        odd_b.ctypes.data + 1) == 0
        for odd, want in ((odd_l, want_line), (odd_b, want_bits)):
            assert odd[0] == 0x5A and odd[-1] == 0x5A and odd[1:-1].tobytes() == want.tobytes()
    dec.close()


def _encode_burst_device(dec, payload, s, where, n, with_bits=True):
    import torch
    N, K, L = _dims(dec.code50.code)
    line_bits, _ = br.burst_words(n, K, L, np.zeros(n) if s is None else s)
    d_pay = _to_device(torch, payload)
    d_line, p_line = _guarded(torch, line_bits // 32)
    d_bits, p_bits = _guarded(torch, n * N // 32)
    torch.cuda.synchronize()
    dec.encode_burst_device(d_pay.data_ptr(), s, where, n, p_line, p_bits if with_bits else None)
    return _inside(d_line, line_bits // 32), _inside(d_bits, n * N // 32).reshape(n, N // 32)


@WHERES
@pytest.mark.parametrize("name", ["cycle", "burst"])
@pytest.mark.parametrize("n", [1, 33, 65])
def test_encode(abi, lib, code50, encoder, n, name, where):
    N, K, L = _dims(code50.code)
    s = br.batch(name, n)
    msg = br.zero_known(np.random.default_rng(100 + n).integers(0, 2, (n, K), dtype=np.uint8), s, where)
    payload = br.burst_payload_of(msg, s, where)
    cw = encoder.encode(msg)
    want_line, want_bits = abi.encode_burst_host(code50.code, payload, s, where, n, True, lib)
    assert want_bits.tobytes() == lr.payload_of(cw).tobytes() and want_line.tobytes() == br.burst_line_of_codewords(cw, K, L, s, where).tobytes()
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 3)
    line, bits = _encode_burst_device(dec, payload, s, where, n)
    assert np.array_equal(line, want_line)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, bad[:8]
    for c, S in enumerate(s):
        k0, k1 = br.known_range(K, S, where)
        assert not bits[c, k0 // 32:k1 // 32].any()
    assert not (line.view(np.int32) == PATTERN).any() and not (bits.view(np.int32) == PATTERN).any()
    line_only, untouched = _encode_burst_device(dec, payload, s, where, n, with_bits=False)
    assert np.array_equal(line_only, want_line) and (untouched.view(np.int32) == PATTERN).all()
    dec.close()


def test_no_shortening_is_the_line_encode(abi, code50):
    import torch
    n = 33
    N, K, L = _dims(code50.code)
    payload = np.random.default_rng(9).integers(0, 2 ** 32, n * K // 32, dtype=np.uint64).astype(np.uint32)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    d_pay = _to_device(torch, payload)
    d_line, p_line = _guarded(torch, n * L // 32)
    d_bits, p_bits = _guarded(torch, n * N // 32)
    torch.cuda.synchronize()
    dec.encode_line_device(d_pay.data_ptr(), n, p_line, p_bits)
    want_line, want_bits = _inside(d_line, n * L // 32), _inside(d_bits, n * N // 32)
    for where in (TAIL, HEAD):
        for s in (None, np.zeros(n, np.uint32)):
            line, bits = _encode_burst_device(dec, payload, s, where, n)
            assert line.tobytes() == want_line.tobytes() and bits.tobytes() == want_bits.tobytes()
    dec.close()


ROUND_TRIP_SEED = 1


def round_trip_batch(encoder, n, where, seed):
    """(shortened, payload, messages, flip mask in burst-line words, flips per codeword): the SHORT cycle, random messages with zeros
    in the known range, a mask with p = 0.005 over the transmitted positions"""
    N, K = encoder.N, encoder.K
    L = N - 384
    s = br.batch("cycle", n)
    rng = np.random.default_rng(seed)
    msg = br.zero_known(rng.integers(0, 2, (n, K), dtype=np.uint8), s, where)
    line_bits, _ = br.burst_words(n, K, L, s)
    mask = (rng.random(line_bits) < 0.005).astype(np.uint8)
    ends = np.cumsum([L - int(S) for S in s])
    flips = np.array([mask[e - (L - int(S)):e].sum() for e, S in zip(ends, s)], dtype=np.int64)
    return s, br.burst_payload_of(msg, s, where), msg, br.pack_words(mask), flips


@WHERES
def test_round_trip(abi, lib, code50, encoder, where):
    """encode_burst_device -> flips with p = 0.005 over the transmitted positions (a numpy mask, XORed on the device) ->
    decode_burst_device, HARD at magnitude 4, DecodeMethod 2, 10 iterations: every codeword returns its payload with unsatisfied 0,
    short_ones 0 and corrected = its flip count.  That needs the decoder itself to succeed on the batch: for seed 1 the CPU port
    under oracle/ (lnsfaid_cpu_decode on lnsfaid_burst_to_llr4's output, 65 codewords in three groups) returns all 65 messages
    with every parity check satisfied, for TAIL and for HEAD, in 4, 4 and 3 iterations per group and no bit-flipping iteration;
    the codewords have 7 .. 103 flips each (seed 2 would do as well: 65 of 65, 9 .. 100 flips)."""
    import torch
    n = 65
    N, K, L = _dims(code50.code)
    s, payload, msg, mask, flips = round_trip_batch(encoder, n, where, ROUND_TRIP_SEED)
    assert flips.min() > 0
    line_bits, payload_bits = br.burst_words(n, K, L, s)
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 3)
    d_pay = _to_device(torch, payload)
    d_line = torch.full((line_bits // 32,), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.encode_burst_device(d_pay.data_ptr(), s, where, n, d_line.data_ptr())
    d_line ^= _to_device(torch, mask)
    d_out, p_out = _guarded(torch, payload_bits // 32)
    d_st, p_st = _guarded(torch, n * 4)
    d_ones, p_ones = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.decode_burst_device(d_line.data_ptr(), HARD, s, where, n, p_out, None, p_st, p_ones, 4)
    dec.close()
    st = _inside(d_st, n * 4).view(abi.line_stats_dtype())
    assert np.array_equal(_inside(d_out, payload_bits // 32), payload)
    assert not st["unsatisfied"].any(), st["unsatisfied"].tolist()
    assert not _inside(d_ones, n).any()
    assert np.array_equal(st["corrected"], flips), (st["corrected"].tolist(), flips.tolist())


def test_refusals(abi, lib, code50, encoder):
    import torch
    n = 33
    N, K, L = _dims(code50.code)
    s, line, _, _, _, _ = _batch(encoder, "cycle", n, HARD, TAIL)
    kw, nw = K // 32, N // 32
    d_line = torch.from_numpy(np.concatenate([line, np.zeros(4, np.uint32)]).view(np.int32)).cuda()
    d_pay, p_pay = _guarded(torch, n * kw + 4)
    d_bits, p_bits = _guarded(torch, n * nw + 4)
    d_st, p_st = _guarded(torch, n * 4 + 4)
    d_ones, p_ones = _guarded(torch, n + 4)
    d_enc, p_enc = _guarded(torch, n * (L // 32) + 4)
    torch.cuda.synchronize()
    p_line, ps = d_line.data_ptr(), s.ctypes.data
    dev, host = lib.lnsfaid_decode_burst_device, lib.lnsfaid_decode_burst
    enc_dev, enc_host = lib.lnsfaid_encode_burst_device, lib.lnsfaid_encode_burst
    h_pay, h_bits, h_line = (np.full(k, 0x5A5A5A5A, np.uint32) for k in (n * kw, n * nw, n * (L // 32)))

    def untouched():
        for t in (d_pay, d_bits, d_st, d_ones, d_enc):
            assert (t.cpu().numpy() == PATTERN).all()
        assert (h_pay == 0x5A5A5A5A).all() and (h_bits == 0x5A5A5A5A).all() and (h_line == 0x5A5A5A5A).all()

    # configurations without a per-codeword decoder refuse the decode, not the encode (tested below on a good context)
    nms = abi.default_cfg(0, MAX_ITER)
    nms.factor_1, nms.factor_2 = 24, 26  # two normalisation factors: the two-rows kernel
    dec = abi.Decoder(code50, nms, 0, 2)
    assert dec.rows_per_lane() == 2
    assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, n, p_pay, p_bits, p_st, p_ones) == E_INVAL
    assert host(dec.ctx, line.ctypes.data, HARD, 4, ps, TAIL, n, h_pay.ctypes.data, h_bits.ctypes.data, None, None) == E_INVAL
    dec.close()
    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 2)
    dec.select_waves(2)
    assert dec.kernel_waves() == 2
    assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, n, p_pay, p_bits, p_st, p_ones) == E_INVAL
    assert host(dec.ctx, line.ctypes.data, HARD, 4, ps, TAIL, n, h_pay.ctypes.data, h_bits.ctypes.data, None, None) == E_INVAL
    dec.close()
    untouched()

    dec = abi.Decoder(code50, _cfg(abi, 2), 0, 1)  # 32 codewords at the most
    assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 33, p_pay, p_bits, p_st, p_ones) == E_INVAL
    assert host(dec.ctx, line.ctypes.data, HARD, 4, ps, TAIL, 33, h_pay.ctypes.data, h_bits.ctypes.data, None, None) == E_INVAL
    assert enc_dev(dec.ctx, p_pay, ps, TAIL, 33, p_enc, p_bits) == E_INVAL
    assert enc_host(dec.ctx, h_pay.ctypes.data, ps, TAIL, 33, h_line.ctypes.data, h_bits.ctypes.data) == E_INVAL
    for off in (1, 2, 3):  # a misaligned device pointer, each of them
        assert dev(dec.ctx, p_line + off, HARD, 4, ps, TAIL, 32, p_pay, p_bits, p_st, p_ones) == E_INVAL
        assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 32, p_pay + off, p_bits, p_st, p_ones) == E_INVAL
        assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 32, p_pay, p_bits + off, p_st, p_ones) == E_INVAL
        assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 32, p_pay, p_bits, p_st + off, p_ones) == E_INVAL
        assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 32, p_pay, p_bits, p_st, p_ones + off) == E_INVAL
        assert enc_dev(dec.ctx, p_pay + off, ps, TAIL, 32, p_enc, p_bits) == E_INVAL
        assert enc_dev(dec.ctx, p_pay, ps, TAIL, 32, p_enc + off, p_bits) == E_INVAL
        assert enc_dev(dec.ctx, p_pay, ps, TAIL, 32, p_enc, p_bits + off) == E_INVAL
    for fn, a, b in ((dev, p_line, p_pay), (host, line.ctypes.data, h_pay.ctypes.data)):
        assert fn(dec.ctx, a, 2, 4, ps, TAIL, 32, b, None, None, None) == E_INVAL   # a bad format
        assert fn(dec.ctx, a, -1, 4, ps, TAIL, 32, b, None, None, None) == E_INVAL
        assert fn(dec.ctx, a, HARD, 0, ps, TAIL, 32, b, None, None, None) == E_INVAL  # a HARD magnitude outside 1 .. 7
        assert fn(dec.ctx, a, HARD, 8, ps, TAIL, 32, b, None, None, None) == E_INVAL
        assert fn(dec.ctx, None, HARD, 4, ps, TAIL, 32, b, None, None, None) == E_INVAL
        assert fn(dec.ctx, a, HARD, 4, ps, TAIL, 32, None, None, None, None) == E_INVAL
        for where in (2, -1):  # a bad `where`
            assert fn(dec.ctx, a, HARD, 4, ps, where, 32, b, None, None, None) == E_INVAL
        for bad in (31, 48, K, K + 32):  # a bad `shortened` entry, the last of the call
            s_bad = s[:32].copy()
            s_bad[31] = bad
            assert fn(dec.ctx, a, HARD, 4, s_bad.ctypes.data, TAIL, 32, b, None, None, None) == E_INVAL, bad
        # n_codewords 0: returns 0 and touches nothing, with buffers or without
        assert fn(dec.ctx, a, HARD, 4, ps, TAIL, 0, b, None, None, None) == 0
        assert fn(dec.ctx, None, LLR4, 0, None, HEAD, 0, None, None, None, None) == 0
    for fn, a, b in ((enc_dev, p_pay, p_enc), (enc_host, h_pay.ctypes.data, h_line.ctypes.data)):
        assert fn(dec.ctx, None, ps, TAIL, 32, b, None) == E_INVAL
        assert fn(dec.ctx, a, ps, TAIL, 32, None, None) == E_INVAL
        for where in (2, -1):
            assert fn(dec.ctx, a, ps, where, 32, b, None) == E_INVAL
        for bad in (31, 48, K, K + 32):
            s_bad = s[:32].copy()
            s_bad[0] = bad
            assert fn(dec.ctx, a, s_bad.ctypes.data, TAIL, 32, b, None) == E_INVAL, bad
        assert fn(dec.ctx, a, ps, TAIL, 0, b, None) == 0
        assert fn(dec.ctx, None, None, HEAD, 0, None, None) == 0
    untouched()
    # and the same context decodes and encodes 32 codewords once the arguments are right (LLR4 ignores the magnitude)
    assert dev(dec.ctx, p_line, HARD, 4, ps, TAIL, 32, p_pay, p_bits, p_st, p_ones) == 0
    assert dev(dec.ctx, p_line, LLR4, 99, None, HEAD, 4, p_pay, None, None, None) == 0
    assert enc_dev(dec.ctx, p_pay, ps, TAIL, 32, p_enc, p_bits) == 0
    dec.select_waves(2)  # the encode does not depend on the decoder configuration
    assert enc_dev(dec.ctx, p_pay, ps, HEAD, 32, p_enc, None) == 0
    dec.close()
