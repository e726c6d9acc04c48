"""Line-format encode on the GPU (include/lnsfaid.h "line-format encode", DESIGN.md §3.15, lnsfaid_encoder_line.hip).  The definition
is lnsfaid_encode_line_host; the expected values of the batches come from the independent numpy encoder (tests/gf2_encoder.py, via
tests/encode_line_ref.py), never the all-zero word alone.  Every device output lies between 64 guard words in front and 64 behind,
which must keep their pattern after every call."""
import ctypes as C

import numpy as np
import pytest

import encode_line_ref as el
import encoder_ref as er
import gf2_encoder
import line_ref as lr
import oracle_abi as oa

pytestmark = pytest.mark.gpu

E_INVAL, E_CODE = -1, -2
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32
MAX_GROUPS = 3


def _words(code):
    return (code.n_var - code.n_check) // 32, (code.n_var - code.puncture_tail) // 32, code.n_var // 32


def _guarded(torch, n_words):
    t = torch.full((GUARD + n_words + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 4 * GUARD


def _inside(t, n_words):
    """the words between the guards, after checking both guards"""
    h = t.cpu().numpy()
    assert (h[:GUARD] == PATTERN).all() and (h[GUARD + n_words:] == PATTERN).all(), "a guard word was overwritten"
    return h[GUARD:GUARD + n_words].view(np.uint32)


def _decoder(abi, code, method=2):
    return abi.Decoder(code, abi.default_cfg(method, 10), 0, MAX_GROUPS)


def _encode_device(dec, payload, n, with_bits=True, extra=0):
    """lnsfaid_encode_line_device on a device copy of exactly the payload's size -> (line [n + extra, L / 32], bits [n + extra,
    N / 32] or the untouched buffer); `extra` codewords of room behind the outputs show what was not written.  Guards checked."""
    import torch
    kw, lw, nw = _words(dec.code50.code)
    assert payload.shape == (n, kw)
    d_pay = torch.from_numpy(np.ascontiguousarray(payload).view(np.int32)).cuda()
    d_line, p_line = _guarded(torch, (n + extra) * lw)
    d_bits, p_bits = _guarded(torch, (n + extra) * nw)
    torch.cuda.synchronize()
    dec.encode_line_device(d_pay.data_ptr(), n, p_line, p_bits if with_bits else None)
    return _inside(d_line, (n + extra) * lw).reshape(n + extra, lw), _inside(d_bits, (n + extra) * nw).reshape(n + extra, nw)


@pytest.fixture(scope="module")
def circ50(abi, lib, code50):
    return abi.code_parity_inverse(code50.code, lib)


@pytest.fixture(scope="module")
def dec(abi, code50):
    d = _decoder(abi, code50)
    yield d
    d.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 96])
def test_device_call_equals_the_host_form(abi, lib, code50, encoder, circ50, dec, n):
    payload, want_line, want_bits = el.batch(encoder, "random", n, 1000 * n)
    h_line, h_bits = abi.encode_line_host(code50.code, payload, n, True, lib, circ50)
    assert np.array_equal(h_line, want_line) and np.array_equal(h_bits, want_bits)  # the definition is the numpy encoder's
    line, bits = _encode_device(dec, payload, n)
    bad = np.nonzero((bits != h_bits).any(axis=1))[0]
    assert bad.size == 0, ("bits", bad[:8].tolist())
    assert np.array_equal(line, h_line)
    line1, bits1 = _encode_device(dec, payload, n, with_bits=False)
    assert np.array_equal(line1, h_line) and (bits1.view(np.int32) == PATTERN).all()


def test_unit_vectors_and_known_answer(abi, code50, encoder, dec):
    payload, want_line, want_bits = el.batch(encoder, "unit")
    line, bits = _encode_device(dec, payload, el.UNIT_VECTORS)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, bad.tolist()
    assert np.array_equal(line, want_line)
    N, K, L = code50.N, code50.K, code50.N - code50.code.puncture_tail
    cw = el.golden_codeword(N)
    line, bits = _encode_device(dec, lr.payload_of(cw[None, :K]), 1)
    assert np.array_equal(np.unpackbits(bits.view(np.uint8), bitorder="little"), cw)
    assert np.array_equal(line, lr.line_of(cw[None, :].astype(np.int8), L, lr.HARD).reshape(1, -1))


@pytest.mark.parametrize("n", [1, 33])
def test_nothing_outside(code50, encoder, dec, n):
    """exactly n * L / 32 and n * N / 32 words change: all of the first n codewords (no word keeps the pattern), nothing of the room
    for two more codewords behind them, and no guard word (checked by _inside)"""
    payload, _, _ = el.batch(encoder, "random", n, 1000 * n)
    kw, lw, nw = _words(code50.code)
    line, bits = _encode_device(dec, payload, n, extra=2)
    for out, per in ((line, lw), (bits, nw)):
        changed = out.view(np.int32) != PATTERN
        assert changed[:n].all() and not changed[n:].any()
        assert int(changed.sum()) == n * per
    assert (lw, nw) == (540, 552)


def test_host_form_of_the_context(abi, lib, code50, encoder, dec):
    n = 33
    payload, want_line, want_bits = el.batch(encoder, "random", n, 1000 * n)
    line, bits = _encode_device(dec, payload, n)
    h_line, h_bits = dec.encode_line(payload, n, with_bits=True)
    assert np.array_equal(h_line, line) and np.array_equal(h_bits, bits)
    h_line, none = dec.encode_line(payload, n)
    assert np.array_equal(h_line, line) and none is None
    # host pointers of any alignment: every buffer at an odd address
    odd_in = np.zeros(payload.nbytes + 1, np.uint8)
    odd_in[1:] = payload.view(np.uint8).reshape(-1)
    odd_line, odd_bits = (np.full(a.nbytes + 2, 0x5A, np.uint8) for a in (line, bits))
    assert lib.lnsfaid_encode_line(dec.ctx, odd_in.ctypes.data + 1, n, odd_line.ctypes.data + 1, odd_bits.ctypes.data + 1) == 0
    for odd, want in ((odd_line, line), (odd_bits, bits)):
        assert odd[0] == 0x5A and odd[-1] == 0x5A and odd[1:-1].tobytes() == want.tobytes()


def test_loopback(abi, code50, encoder):
    """encode_line_device, then decode_line_device (HARD, magnitude 4) on the same device buffers: the payload comes back word for
    word with nothing corrected, and the counters find no wrong frame in `bits`"""
    import torch
    n = 33
    kw, lw, nw = _words(code50.code)
    payload, _, _ = el.batch(encoder, "random", n, 1000 * n)
    d = _decoder(abi, code50, 2)
    d_pay = torch.from_numpy(payload.view(np.int32)).cuda()
    d_line, p_line = _guarded(torch, n * lw)
    d_bits, p_bits = _guarded(torch, n * nw)
    d_back, p_back = _guarded(torch, n * kw)
    d_st, p_st = _guarded(torch, n * 4)
    torch.cuda.synchronize()
    d.encode_line_device(d_pay.data_ptr(), n, p_line, p_bits)
    d.decode_line_device(p_line, abi.LINE_HARD, n, p_back, None, p_st, 4)
    back = _inside(d_back, n * kw).reshape(n, kw)
    st = _inside(d_st, n * 4).view(abi.line_stats_dtype())
    bits = _inside(d_bits, n * nw).reshape(n, nw)
    _inside(d_line, n * lw)
    assert np.array_equal(back, payload)
    assert not st["unsatisfied"].any() and not st["corrected"].any(), st.tolist()
    # the counters take whole groups: the 33 codewords and their payloads in zeroed room for 64
    pad_bits = torch.zeros((64, nw), dtype=torch.int32, device="cuda")
    pad_msg = torch.zeros((64, kw), dtype=torch.int32, device="cuda")
    pad_bits[:n] = torch.from_numpy(bits.view(np.int32)).cuda()
    pad_msg[:n] = d_pay.reshape(n, kw)
    torch.cuda.synchronize()
    out = d.count_errors_packed_device(pad_bits.data_ptr(), pad_msg.data_ptr(), 2)
    d.close()
    assert out == [64, 0, 0, 0], out


def test_independent_of_the_decoder_configuration(abi, code50, encoder):
    n = 33
    payload, want_line, want_bits = el.batch(encoder, "random", n, 1000 * n)
    nms = abi.default_cfg(0, 10)
    nms.factor_1, nms.factor_2 = 24, 26  # two normalisation factors: the two-rows kernel
    d = abi.Decoder(code50, nms, 0, MAX_GROUPS)
    assert d.rows_per_lane() == 2
    line, bits = _encode_device(d, payload, n)
    d.close()
    assert np.array_equal(line, want_line) and np.array_equal(bits, want_bits)
    d = _decoder(abi, code50, 5)
    d.select_waves(2)
    d.set_early_stop(1)  # LNSFAID_STOP_CODEWORD
    line, bits = _encode_device(d, payload, n)
    d.close()
    assert np.array_equal(line, want_line) and np.array_equal(bits, want_bits)


def test_derived_codes(abi, lib):
    import torch
    dc, enc = el.derived(abi, lib)
    n = 33
    kw, lw, nw = _words(dc.code)
    payload, want_line, want_bits = el.expected(enc, el.messages(n, dc.K, 77), dc.N - dc.code.puncture_tail)
    d = _decoder(abi, dc)
    line, bits = _encode_device(d, payload, n)
    h_line, _ = d.encode_line(payload, n)
    d.close()
    assert np.array_equal(line, want_line) and np.array_equal(bits, want_bits) and np.array_equal(h_line, want_line)

    sc = er.derived_code(abi, lib, [68], 11)  # column 68 leaves block row 11: the parity part is singular
    cfg = abi.default_cfg(2, 10)
    d = abi.Decoder(sc, cfg, 0, MAX_GROUPS)
    d_pay = torch.zeros(n * kw, dtype=torch.int32, device="cuda")
    d_line, p_line = _guarded(torch, n * lw)
    h_line = np.full(n * lw, 0x5A5A5A5A, np.uint32)
    torch.cuda.synchronize()
    assert lib.lnsfaid_encode_line_device(d.ctx, d_pay.data_ptr(), n, p_line, None) == E_CODE
    assert lib.lnsfaid_encode_line(d.ctx, payload.ctypes.data, n, h_line.ctypes.data, None) == E_CODE
    assert (d_line.cpu().numpy() == PATTERN).all() and (h_line == 0x5A5A5A5A).all()
    fix = oa.synth_llr(1, sc.N, 3.9, seed=31)
    ref, rst = oa.decode_mt(sc, cfg, fix, 1)
    got, st = d.decode(fix, 1)
    d.close()
    assert np.array_equal(got, ref) and np.array_equal(st, rst)


def test_refusals(abi, lib, code50, encoder, dec):
    import torch
    n = 96
    kw, lw, nw = _words(code50.code)
    payload, _, _ = el.batch(encoder, "random", n, 1000 * n)
    d_pay = torch.from_numpy(np.concatenate([payload.reshape(-1), np.zeros(kw + 4, np.uint32)]).view(np.int32)).cuda()
    d_line, p_line = _guarded(torch, (n + 1) * lw + 4)
    d_bits, p_bits = _guarded(torch, (n + 1) * nw + 4)
    h_pay = np.concatenate([payload.reshape(-1), np.zeros(kw, np.uint32)])
    h_line, h_bits = np.full((n + 1) * lw, 0x5A5A5A5A, np.uint32), np.full((n + 1) * nw, 0x5A5A5A5A, np.uint32)
    torch.cuda.synchronize()
    p_pay = d_pay.data_ptr()
    dev, host = lib.lnsfaid_encode_line_device, lib.lnsfaid_encode_line

    def untouched():
        for t in (d_line, d_bits):
            assert (t.cpu().numpy() == PATTERN).all()
        assert (h_line == 0x5A5A5A5A).all() and (h_bits == 0x5A5A5A5A).all()

    assert dev(dec.ctx, p_pay, 97, p_line, p_bits) == E_INVAL  # more than 32 * max_groups
    assert host(dec.ctx, h_pay.ctypes.data, 97, h_line.ctypes.data, h_bits.ctypes.data) == E_INVAL
    assert dev(dec.ctx, p_pay, n, None, p_bits) == E_INVAL     # a NULL line, a NULL payload
    assert dev(dec.ctx, None, n, p_line, p_bits) == E_INVAL
    assert host(dec.ctx, h_pay.ctypes.data, n, None, h_bits.ctypes.data) == E_INVAL
    assert host(dec.ctx, None, n, h_line.ctypes.data, h_bits.ctypes.data) == E_INVAL
    for off in (1, 2, 3):  # a misaligned device pointer, each of the three
        assert dev(dec.ctx, p_pay + off, n, p_line, p_bits) == E_INVAL
        assert dev(dec.ctx, p_pay, n, p_line + off, p_bits) == E_INVAL
        assert dev(dec.ctx, p_pay, n, p_line, p_bits + off) == E_INVAL
    # n_codewords 0: returns 0 and touches nothing, with buffers or without
    assert dev(dec.ctx, p_pay, 0, p_line, p_bits) == 0 and dev(dec.ctx, None, 0, None, None) == 0
    assert host(dec.ctx, h_pay.ctypes.data, 0, h_line.ctypes.data, h_bits.ctypes.data) == 0 and host(dec.ctx, None, 0, None, None) == 0
    untouched()
    # and the same context encodes once the arguments are right, also at a 4-byte offset (rows no longer on 16 bytes)
    assert dev(dec.ctx, p_pay + 4, 1, p_line + 4, p_bits + 4) == 0
    want_line, want_bits = dec.encode_line(np.ascontiguousarray(h_pay[1:1 + kw]).reshape(1, kw), 1, with_bits=True)
    assert np.array_equal(_inside(d_line, (n + 1) * lw + 4)[1:1 + lw], want_line[0])
    assert np.array_equal(_inside(d_bits, (n + 1) * nw + 4)[1:1 + nw], want_bits[0])


def test_group_encoder_is_not_disturbed(abi, code50, encoder):
    """lnsfaid_encode_device after the line call came first on the context (both use the context's one B^-1): the int8 groups of the
    numpy encoder, as before"""
    import torch
    n = 64
    K, N, M = code50.K, code50.N, code50.M
    msg = el.messages(n, K, 4242)
    payload, want_line, _ = el.expected(encoder, msg, N - code50.code.puncture_tail)
    d = _decoder(abi, code50)
    line, _ = _encode_device(d, payload, n)
    assert np.array_equal(line, want_line)
    info = np.ascontiguousarray(msg.astype(np.int8).reshape(-1))
    d_in = torch.from_numpy(info).cuda()
    d_out = torch.zeros(n * N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    d.encode_device(d_in.data_ptr(), 2, d_out.data_ptr())
    out = d_out.cpu().numpy()
    h_out = d.encode(info, 2)
    d.close()
    want = gf2_encoder.to_group_layout(encoder.encode(msg), K)
    assert np.array_equal(out, want) and np.array_equal(h_out, want)
