"""Every kernel that takes the code as an argument, on codes that are not 12 x 69 blocks (tests/code_shapes.py holds the shapes, the
batches and the cached CPU references; tests/test_code_shapes_cpu.py checks those without a GPU).  One context per (shape,
DecodeMethod), kept for the module; all comparisons are byte for byte: group decodes against the CPU port on every kernel path the
context can be steered to, the steering asserted through the library's own queries and a refusal asserted where the shape has no
such instance; the per-codeword entries against the 32-copies restatement; the line, burst and encode calls, the FEC status and
the failure capture against the definitions tests/test_gpu_line.py and its neighbours use on the built-in code; lnsfaid_create at
and beyond each of its limits."""
import ctypes as C

import numpy as np
import pytest

import burst_ref as br
import code_shapes as cs
import early_stop_ref as esr
import encode_line_ref as el
import fec_status_ref as fs
import line_ref as lr
import oracle_abi as oa

pytestmark = pytest.mark.gpu

NG = cs.NG
E_INVAL, E_CODE = -1, -2
FAMILIES = tuple("m%d" % m for m in cs.METHODS)
PATHS = ("default", "loop", "rotating", "hbm", "rows2", "waves2", "packed")
LINE_SHAPES = ("few", "thirteen", "most", "wide")
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32


@pytest.fixture(scope="module")
def decoders(abi, lib):
    """(shape, family) -> its one context, created on first use and kept until the module is done"""
    made = {}

    def get(name, family):
        if (name, family) not in made:
            made[(name, family)] = abi.Decoder(cs.code(name), cs.cfg_of(abi, lib, family), device=0, max_groups=NG, lib=lib)
        return made[(name, family)]

    yield get
    for d in made.values():
        d.close()


_props = {}


def _caps(abi, lib, name, family):
    """what the library has for a (shape, family), from the limits in tests/code_shapes.py's docstring"""
    if name not in _props:
        _props[name] = cs.properties(cs.describe(name), abi, lib)
    p = _props[name]
    method = int(family[1])
    registers = method != 0 and p["layers"] <= 12
    zero = registers and any((d == 23 and zg >= 1) or (d == 22 and zg >= 5) for d, zg in zip(p["degrees"], p["zero_groups"]))
    return {"registers": registers, "zero": zero, "waves2": method != 0 and p["N"] // 32 >= 448}


def _reset(dec):
    dec.select_waves(0)
    dec.select_kernel(0)
    dec.select_message_store(0)
    dec.select_zero_shift(0)


def _select(abi, dec, caps, path):
    """steer `dec` to `path` and assert through the queries that the path is what runs next; False where the library refuses the
    path for this shape (the refusal asserted)"""
    _reset(dec)
    store = abi.MSG_REGISTERS if caps["registers"] else abi.MSG_HBM
    assert not dec.static_layers() and not dec.window_free()  # not the built-in table
    if path in ("default", "packed"):
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1 and dec.message_store() == store
        assert dec.zero_shift_groups()[0] == caps["zero"]
    elif path == "loop":
        if not caps["zero"]:
            for mode in (abi.ZERO_SHIFT_LOOP, abi.ZERO_SHIFT_ON, abi.ZERO_SHIFT_STATIC, abi.ZERO_SHIFT_WINDOWED):
                with pytest.raises(RuntimeError):
                    dec.select_zero_shift(mode)
            return False
        for mode in (abi.ZERO_SHIFT_STATIC, abi.ZERO_SHIFT_WINDOWED):
            with pytest.raises(RuntimeError):
                dec.select_zero_shift(mode)
        dec.select_zero_shift(abi.ZERO_SHIFT_LOOP)
        on, groups = dec.zero_shift_groups()
        assert on and max(groups) >= 1 and not dec.static_layers()
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1 and dec.message_store() == abi.MSG_REGISTERS
    elif path == "rotating":
        dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
        assert not dec.zero_shift_groups()[0]
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1 and dec.message_store() == store
    elif path == "hbm":
        if not caps["registers"]:
            with pytest.raises(RuntimeError):
                dec.select_message_store(abi.MSG_REGISTERS)
        dec.select_message_store(abi.MSG_HBM)
        assert dec.message_store() == abi.MSG_HBM and dec.rows_per_lane() == 4 and dec.kernel_waves() == 1
        assert not dec.zero_shift_groups()[0]
    elif path == "rows2":
        dec.select_kernel(2)
        assert dec.rows_per_lane() == 2 and dec.kernel_waves() == 1 and dec.message_store() == abi.MSG_HBM
        assert not dec.zero_shift_groups()[0]
    elif path == "waves2":
        if not caps["waves2"]:
            with pytest.raises(RuntimeError):
                dec.select_waves(2)
            return False
        dec.select_waves(2)
        assert dec.kernel_waves() == 2 and dec.rows_per_lane() == 4 and dec.message_store() == abi.MSG_HBM
        assert not dec.zero_shift_groups()[0]
    else:
        raise AssertionError(path)
    return True


def _bad_frames(h, out, ref):
    return np.nonzero((out.reshape(-1, h.N) != ref.reshape(-1, h.N)).any(axis=1))[0][:8].tolist()


def _decode_and_compare(abi, lib, dec, name, key, which, packed=False, what=""):
    h = cs.code(name)
    fix = cs.batch(name, cs.method_of(key), which)[0]
    ref, ref_st = cs.reference(abi, lib, name, key, which)
    if packed:
        bits, st = dec.decode_packed(abi.pack_llr4(fix, lib), NG)
        out = abi.unpack_bits(bits, lib)
    else:
        out, st = dec.decode(fix, NG)
    print("%s %s %s %s: iterations / bit-flipping iterations %s" % (name, key, which, what, st.tolist()))
    assert np.array_equal(out, ref), (name, key, which, what, _bad_frames(h, out, ref))
    assert np.array_equal(st, ref_st), (name, key, which, what, st.tolist(), ref_st.tolist())
    return st


# ---- selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.NAMES)
def test_selection_follows_the_shape(abi, lib, decoders, name):
    dec = decoders(name, "m2")
    caps = _caps(abi, lib, name, "m2")
    _reset(dec)
    assert not dec.static_layers() and not dec.window_free()
    if name in ("thirteen", "most"):
        assert dec.message_store() == abi.MSG_HBM
        with pytest.raises(RuntimeError):
            dec.select_message_store(abi.MSG_REGISTERS)
        with pytest.raises(RuntimeError):
            dec.select_zero_shift(abi.ZERO_SHIFT_ON)
        assert not dec.zero_shift_groups()[0]
    else:
        assert dec.message_store() == abi.MSG_REGISTERS
        assert dec.zero_shift_groups()[0] == (name == "few") == caps["zero"]
    if name == "few":
        on, groups = dec.zero_shift_groups()
        assert on and groups[:4] == [0, 1, 0, 0]
        dec.select_zero_shift(abi.ZERO_SHIFT_ON)
        assert dec.zero_shift_groups()[0]
    # DecodeMethod 0 never keeps its messages in registers
    d0 = decoders(name, "m0")
    _reset(d0)
    assert d0.rows_per_lane() == 4 and d0.message_store() == abi.MSG_HBM and not d0.zero_shift_groups()[0]
    with pytest.raises(RuntimeError):
        d0.select_message_store(abi.MSG_REGISTERS)
    _reset(dec)


# ---- group decode -----------------------------------------------------------------------------------------------------------------
def _group_params():
    for name in cs.NAMES:
        for family in FAMILIES:
            for path in PATHS:
                yield pytest.param(name, family, path, id="%s-%s-%s" % (name, family, path))


@pytest.mark.parametrize("name,family,path", list(_group_params()))
def test_group_decode_equals_the_port(abi, lib, decoders, name, family, path):
    dec = decoders(name, family)
    if not _select(abi, dec, _caps(abi, lib, name, family), path):
        _reset(dec)
        return
    for which in ("mixed", "clean"):
        st = _decode_and_compare(abi, lib, dec, name, family, which, packed=path == "packed", what=path)
        if which == "mixed" and int(family[1]) in (2, 4, 5):
            assert st[:, 1].max() > 0  # the bit-flipping stage ran (on `noflip` it runs and flips nothing)
    _reset(dec)


@pytest.mark.parametrize("name", cs.NAMES)
def test_scalar_oracle_pins_the_port(abi, lib, name):
    """the scalar oracle on one group of the mixed batch, DecodeMethods 2 and 5: what the other tests compare against is right on
    this shape"""
    for key in ("m2", "m5"):
        ref, ref_st = cs.reference(abi, lib, name, key, "mixed", "oracle", 1)
        port, port_st = cs.reference(abi, lib, name, key, "mixed")
        assert np.array_equal(ref, port[:ref.size]) and np.array_equal(ref_st, port_st[:1])


@pytest.mark.parametrize("name", cs.NAMES)
def test_nms_with_two_factors(abi, lib, decoders, name):
    """DecodeMethod 0 with factors 24 / 28: the two-rows kernel (one factor, the four-rows kernel, is family m0 above)"""
    dec = decoders(name, "m0")
    _reset(dec)
    dec.set_cfg(cs.cfg_of(abi, lib, "m0two"))
    try:
        assert dec.rows_per_lane() == 2 and dec.message_store() == abi.MSG_HBM
        with pytest.raises(RuntimeError):
            dec.select_kernel(4)
        for which in ("mixed", "clean"):
            _decode_and_compare(abi, lib, dec, name, "m0two", which, what="two factors")
            _decode_and_compare(abi, lib, dec, name, "m0two", which, packed=True, what="two factors, packed")
    finally:
        dec.set_cfg(cs.cfg_of(abi, lib, "m0"))
    assert dec.rows_per_lane() == 4


@pytest.mark.parametrize("ef", [1, 2])
@pytest.mark.parametrize("name", ["few", "thirteen"])
def test_ef_elimination(abi, lib, decoders, name, ef):
    dec = decoders(name, "m2")
    key = "m2ef%d" % ef
    caps = _caps(abi, lib, name, "m2")
    _reset(dec)
    dec.set_cfg(cs.cfg_of(abi, lib, key))
    try:
        # the erasing instance of EF_ELIMINATION 2 streams its messages; neither exists in the two-rows kernel
        registers = caps["registers"] and ef == 1
        assert dec.rows_per_lane() == 4 and dec.message_store() == (abi.MSG_REGISTERS if registers else abi.MSG_HBM)
        assert dec.zero_shift_groups()[0] == (caps["zero"] and ef == 1)
        with pytest.raises(RuntimeError):
            dec.select_kernel(2)
        for which in ("mixed", "clean"):
            _decode_and_compare(abi, lib, dec, name, key, which, what="default")
            _decode_and_compare(abi, lib, dec, name, key, which, packed=True, what="packed")
            dec.select_message_store(abi.MSG_HBM)
            _decode_and_compare(abi, lib, dec, name, key, which, what="hbm")
            dec.select_message_store(0)
    finally:
        _reset(dec)
        dec.set_cfg(cs.cfg_of(abi, lib, "m2"))


@pytest.mark.parametrize("key", ["m2classes", "m5classes"])
def test_tables_that_differ_between_the_weight_classes(abi, lib, decoders, key):
    """`most` holds columns of all four weight classes (3 / 6 / 11 / other); a table set that differs between them runs on the
    two-rows kernel"""
    dec = decoders("most", key[:2])
    _reset(dec)
    dec.set_cfg(cs.cfg_of(abi, lib, key))
    try:
        assert dec.rows_per_lane() == 2
        with pytest.raises(RuntimeError):
            dec.select_kernel(4)
        for which in ("mixed", "clean"):
            _decode_and_compare(abi, lib, dec, "most", key, which, what="per-class tables")
        # (tests/test_code_shapes_cpu.py holds that these references differ from those of the uniform tables)
    finally:
        dec.set_cfg(cs.cfg_of(abi, lib, key[:2]))


# ---- the per-codeword rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2, 5])
@pytest.mark.parametrize("name", cs.NAMES)
def test_codeword_decode_equals_the_port(abi, lib, decoders, name, method):
    """lnsfaid_decode_codewords and lnsfaid_decode_codewords_packed: decisions and iterations / bf_iterations of eight codewords of
    each batch against 32 copies of the codeword through the CPU port; `unsatisfied` of every codeword against numpy"""
    h = cs.code(name)
    key = "m%d" % method
    dec = decoders(name, key)
    _reset(dec)
    sub = list(cs.CODEWORDS)
    for which in ("mixed", "clean"):
        fix = cs.batch(name, method, which)[0]
        ref, ref_st = cs.codeword_reference(abi, lib, name, key, which)
        out, cw = dec.decode_codewords(fix, NG)
        out = out.reshape(cs.FRAMES, h.N)
        assert np.array_equal(out[sub], ref), (name, key, which, np.nonzero((out[sub] != ref).any(axis=1))[0].tolist())
        assert np.array_equal(cw[sub, :2], ref_st), (name, key, which, cw[sub, :2].tolist(), ref_st.tolist())
        assert np.array_equal(cw[:, 2], esr.unsatisfied(h, out)), (name, key, which)
        bits, cwp = dec.decode_codewords_packed(abi.pack_llr4(fix, lib), NG)
        assert np.array_equal(abi.unpack_bits(bits, lib).reshape(cs.FRAMES, h.N), out), (name, key, which, "packed")
        assert np.array_equal(cwp, cw), (name, key, which, "packed")
    assert dec.early_stop() == abi.STOP_GROUP


# ---- line and burst calls -----------------------------------------------------------------------------------------------------------
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


def _words(code):
    return (code.n_var - code.n_check) // 32, (code.n_var - code.puncture_tail) // 32, code.n_var // 32


def _packed_codeword_reference(abi, lib, dec, llr4, n):
    """lnsfaid_decode_codewords_packed_device and lnsfaid_fec_status_packed_host on an llr4 input: (bits [n, N / 32], iterations /
    bf_iterations / unsatisfied [n, 3], corrected [n])"""
    import torch
    code = dec.code50.code
    N, ng = code.n_var, (n + 31) // 32
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


def _decode_line_device(abi, dec, line, fmt, magnitude, n):
    import torch
    kw, _, nw = _words(dec.code50.code)
    d_line = _to_device(torch, line)
    d_pay, p_pay = _guarded(torch, n * kw)
    d_bits, p_bits = _guarded(torch, n * nw)
    d_st, p_st = _guarded(torch, n * 4)
    torch.cuda.synchronize()
    dec.decode_line_device(d_line.data_ptr(), fmt, n, p_pay, p_bits, p_st, magnitude)
    return _inside(d_pay, n * kw).reshape(n, kw), _inside(d_bits, n * nw).reshape(n, nw), _inside(d_st, n * 4).view(abi.line_stats_dtype())


@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("fmt,magnitude", [(lr.HARD, 4), (lr.LLR4, 0)], ids=["hard4", "llr4"])
@pytest.mark.parametrize("family", ["m2", "m5"])
@pytest.mark.parametrize("name", LINE_SHAPES)
def test_decode_line(abi, lib, decoders, name, family, fmt, magnitude, n):
    """lnsfaid_decode_line_device against lnsfaid_decode_codewords_packed_device on lnsfaid_line_to_llr4's output"""
    h = cs.code(name)
    dec = decoders(name, family)
    _reset(dec)
    fix = cs.batch(name, int(family[1]), "mixed")[0]
    line = abi.line_from_fixinput(h.code, fix, n, fmt, lib) if n > 64 else abi.line_from_fixinput(h.code, fix[:(n + 31) // 32 * 32 * h.N], n, fmt, lib)
    want_bits, want_cw, want_corrected = _packed_codeword_reference(abi, lib, dec, abi.line_to_llr4(h.code, line, fmt, magnitude, n, lib), n)
    payload, bits, st = _decode_line_device(abi, dec, line, fmt, magnitude, n)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, ("bits", bad[:8].tolist())
    assert np.array_equal(payload, want_bits[:, :payload.shape[1]])
    for i, field in enumerate(("iterations", "bf_iterations", "unsatisfied")):
        assert np.array_equal(st[field], want_cw[:, i]), (field, st[field][:8].tolist(), want_cw[:8, i].tolist())
    assert np.array_equal(st["corrected"], want_corrected)
    print("%s %s n = %d: %d codewords stop early, %d end with unsatisfied checks" % (name, family, n, int((st["iterations"] < cs.MAX_ITER).sum()),
                                                                                   int((st["unsatisfied"] > 0).sum())))
    h_pay, h_bits, h_st = dec.decode_line(line, fmt, n, magnitude, with_bits=True)  # the host form
    assert np.array_equal(h_pay, payload) and np.array_equal(h_bits, bits) and np.array_equal(h_st, st)


def _burst_pattern(K, n):
    """S_c of n codewords: nothing, one word, beside the edge of a block column on either side, half of K, the maximum K - 32"""
    short = (0, 32, 224, 256, 288, K // 2 // 32 * 32 + 32, K - 32)
    return np.array([short[c % len(short)] for c in range(n)], dtype=np.uint32)


def _burst_case(name, fmt, where, n=33):
    """(S, burst line, messages, codewords): random messages with zeros in the known range, encoded, through the channel of the
    shape's DecodeMethod 2 mixed batch (LLR4) or with two bits of every codeword inverted (HARD)"""
    h, enc = cs.code(name), cs.encoder(name)
    N, K, L = h.N, h.K, h.N - h.code.puncture_tail
    s = _burst_pattern(K, n)
    rng = np.random.default_rng(1100 + where)
    msg = br.zero_known(rng.integers(0, 2, (n, K), dtype=np.uint8), s, where)
    cw = enc.encode(msg)
    if fmt == lr.LLR4:
        frames = cs.qpsk_awgn(lr.pad_to_groups(cw), cs.BATCHES[(name, 2)][0][0], 1100)[:n].copy()
    else:
        rx = cw.astype(np.uint8).copy()
        for c in range(n):
            rx[c, [40 + 3 * c, K + 5 + c]] ^= 1  # one in the information part (outside every known range but the longest), one in the parity
        frames = np.where(rx > 0, 1, -1).astype(np.int8)
    frames[:, L:] = 0
    return s, br.burst_line_of(frames, K, L, fmt, s, where), msg, cw


@pytest.mark.parametrize("fmt,magnitude,where", [(lr.HARD, 4, br.HEAD), (lr.LLR4, 0, br.TAIL)], ids=["hard4-head", "llr4-tail"])
@pytest.mark.parametrize("name", LINE_SHAPES)
def test_decode_burst(abi, lib, decoders, name, fmt, magnitude, where):
    """lnsfaid_decode_burst_device against lnsfaid_decode_codewords_packed_device on lnsfaid_burst_to_llr4's output"""
    import torch
    h = cs.code(name)
    N, K, L = h.N, h.K, h.N - h.code.puncture_tail
    n = 33
    dec = decoders(name, "m2")
    _reset(dec)
    s, line, msg, cw = _burst_case(name, fmt, where, n)
    llr4 = abi.burst_to_llr4(h.code, line, fmt, magnitude, s, where, n, lib)
    assert np.array_equal(llr4, br.llr4_of_burst(line, n, N, K, L, fmt, magnitude, s, where))  # the host form on this shape
    want_bits, want_cw, fec_corrected = _packed_codeword_reference(abi, lib, dec, llr4, n)
    _, payload_bits = br.burst_words(n, K, L, s)
    pw, nw = payload_bits // 32, N // 32
    d_line = _to_device(torch, line)
    d_pay, p_pay = _guarded(torch, pw)
    d_bits, p_bits = _guarded(torch, n * nw)
    d_st, p_st = _guarded(torch, n * 4)
    d_ones, p_ones = _guarded(torch, n)
    torch.cuda.synchronize()
    dec.decode_burst_device(d_line.data_ptr(), fmt, s, where, n, p_pay, p_bits, p_st, p_ones, magnitude)
    payload, bits = _inside(d_pay, pw), _inside(d_bits, n * nw).reshape(n, nw)
    st, ones = _inside(d_st, n * 4).view(abi.line_stats_dtype()), _inside(d_ones, n)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, ("bits", bad[:8].tolist())
    assert np.array_equal(payload, br.payload_of_bits(want_bits, K, s, where))
    for i, field in enumerate(("iterations", "bf_iterations", "unsatisfied")):
        assert np.array_equal(st[field], want_cw[:, i]), (field, st[field][:8].tolist(), want_cw[:8, i].tolist())
    want_corrected, want_ones = br.counts(want_bits, line, N, K, L, fmt, s, where)
    assert np.array_equal(st["corrected"], want_corrected) and np.array_equal(ones, want_ones)
    assert np.array_equal(st["corrected"].astype(np.int64) + ones, fec_corrected)
    print("%s: %d of %d burst codewords end with unsatisfied checks" % (name, int((st["unsatisfied"] > 0).sum()), n))


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("name", LINE_SHAPES)
def test_encoders(abi, lib, decoders, name, n):
    """lnsfaid_encode_device, lnsfaid_encode_line_device (with and without bits) and lnsfaid_encode_burst_device against the numpy
    encoder on random payloads"""
    import torch
    h, enc = cs.code(name), cs.encoder(name)
    N, K, L = h.N, h.K, h.N - h.code.puncture_tail
    kw, lw, nw = _words(h.code)
    dec = decoders(name, "m2")
    msg = el.messages(n, K, 500 + n)
    payload, want_line, want_bits = el.expected(enc, msg, L)
    # the line form
    for with_bits in (True, False):
        d_pay = _to_device(torch, np.ascontiguousarray(payload))
        d_line, p_line = _guarded(torch, n * lw)
        d_bits, p_bits = _guarded(torch, n * nw)
        torch.cuda.synchronize()
        dec.encode_line_device(d_pay.data_ptr(), n, p_line, p_bits if with_bits else None)
        assert np.array_equal(_inside(d_line, n * lw).reshape(n, lw), want_line)
        got = _inside(d_bits, n * nw).reshape(n, nw)
        assert np.array_equal(got, want_bits) if with_bits else (got.view(np.int32) == PATTERN).all()
    # the group form: int8 bits, [32][K] in, [32][K] then [32][M] out
    ng = (n + 31) // 32
    gmsg = el.messages(32 * ng, K, 900 + n)
    info = np.ascontiguousarray(gmsg.astype(np.int8).reshape(-1))
    d_in = torch.from_numpy(info).cuda()
    d_out = torch.full((ng * 32 * N + 2 * GUARD,), 0x5A, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    dec.encode_device(d_in.data_ptr(), ng, d_out.data_ptr() + GUARD)
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == 0x5A).all() and (out[-GUARD:] == 0x5A).all()
    assert np.array_equal(out[GUARD:-GUARD], cs.group_layout(enc.encode(gmsg), K))
    # the burst form
    s = _burst_pattern(K, n)
    bmsg = br.zero_known(msg, s, br.TAIL)
    bcw = enc.encode(bmsg)
    line_bits, payload_bits = br.burst_words(n, K, L, s)
    d_pay = _to_device(torch, br.burst_payload_of(bmsg, s, br.TAIL))
    d_line, p_line = _guarded(torch, line_bits // 32)
    d_bits, p_bits = _guarded(torch, n * nw)
    torch.cuda.synchronize()
    dec.encode_burst_device(d_pay.data_ptr(), s, br.TAIL, n, p_line, p_bits)
    assert np.array_equal(_inside(d_line, line_bits // 32), br.burst_line_of_codewords(bcw, K, L, s, br.TAIL))
    assert np.array_equal(_inside(d_bits, n * nw).reshape(n, nw), lr.payload_of(bcw))


@pytest.mark.parametrize("name", LINE_SHAPES)
def test_line_round_trip(abi, lib, decoders, name):
    """encode_line -> line_bsc at a low p -> decode_line on device buffers: the payload comes back, `corrected` is the flips"""
    import torch
    h = cs.code(name)
    n = 33
    kw, lw, nw = _words(h.code)
    dec = decoders(name, "m2")
    _reset(dec)
    payload, line, bits, thr, rx, flips = cs.round_trip_case(abi, lib, name, n)
    d_pay = _to_device(torch, np.ascontiguousarray(payload))
    d_line, p_line = _guarded(torch, n * lw)
    d_rx, p_rx = _guarded(torch, n * lw)
    d_flips, p_flips = _guarded(torch, n)
    d_back, p_back = _guarded(torch, n * kw)
    d_st, p_st = _guarded(torch, n * 4)
    torch.cuda.synchronize()
    dec.encode_line_device(d_pay.data_ptr(), n, p_line, None)
    total = dec.line_bsc_device(p_line, n, cs.ROUND_TRIP_KEY + 1, 0, thr, p_rx, p_flips)
    dec.decode_line_device(p_rx, lr.HARD, n, p_back, None, p_st, 4)
    assert np.array_equal(_inside(d_line, n * lw).reshape(n, lw), line)
    assert np.array_equal(_inside(d_rx, n * lw).reshape(n, lw), rx) and np.array_equal(_inside(d_flips, n), flips)
    assert total == int(flips.sum()) > 0
    st = _inside(d_st, n * 4).view(abi.line_stats_dtype())
    assert np.array_equal(_inside(d_back, n * kw).reshape(n, kw), payload)
    assert not st["unsatisfied"].any() and np.array_equal(st["corrected"], flips), (st["corrected"].tolist(), flips.tolist())


# ---- the syndrome outside the decoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.NAMES)
def test_fec_status(abi, lib, decoders, name):
    """lnsfaid_fec_status_device / _packed_device, with and without sent frames, against the host forms on the CPU port's decisions"""
    import torch
    h = cs.code(name)
    dec = decoders(name, "m2")
    fix, cw = cs.batch(name, 2, "mixed")
    out, _ = cs.reference(abi, lib, name, "m2", "mixed")
    sent = cs.group_layout(cw, h.K)
    llr4, bits = abi.pack_llr4(fix, lib), fs.pack_decisions(out)
    d_fix, d_out, d_sent = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (fix, out, sent))
    d_llr4, d_bits = torch.from_numpy(llr4).cuda(), _to_device(torch, bits)
    torch.cuda.synchronize()
    for with_sent in (True, False):
        sp, s = (d_sent.data_ptr(), sent) if with_sent else (None, None)
        want = abi.fec_status_host(h.code, fix, out, s, NG, vs_sent=True, lib=lib)
        assert want[1][1] > 0 and want[1][1] < cs.FRAMES  # uncorrectable and corrected codewords
        got = dec.fec_status_device(d_fix.data_ptr(), d_out.data_ptr(), sp, NG, vs_sent=True)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (got[1], want[1], got[2], want[2])
        wantp = abi.fec_status_packed_host(h.code, llr4, bits, s, NG, vs_sent=True, lib=lib)
        assert np.array_equal(wantp[0], want[0]) and wantp[1:] == want[1:]
        got = dec.fec_status_packed_device(d_llr4.data_ptr(), d_bits.data_ptr(), sp, NG, vs_sent=True)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    want = abi.fec_status_host(h.code, None, out, None, NG, lib=lib)  # no channel input either: the syndrome alone
    got = dec.fec_status_device(None, d_out.data_ptr(), None, NG)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("fmt", [lr.HARD, lr.LLR4], ids=["hard", "llr4"])
@pytest.mark.parametrize("name", cs.NAMES)
def test_line_capture(abi, lib, decoders, name, fmt):
    """lnsfaid_line_capture_device against lnsfaid_line_capture_host, 33 codewords, select 3"""
    import torch
    h = cs.code(name)
    n = 33
    dec = decoders(name, "m2")
    idx, lines, bits, sent = cs.capture_case(abi, lib, name, n)
    line = lines[fmt]
    d_line, d_bits, d_sent = (_to_device(torch, np.ascontiguousarray(a)) for a in (line, bits, sent))
    torch.cuda.synchronize()
    want = abi.line_capture_host(h.code, line, fmt, bits, sent, n, 5, 3, 0, 256, lib)
    got = dec.line_capture_device(d_line.data_ptr(), fmt, d_bits.data_ptr(), d_sent.data_ptr(), n, 5, 3, 0, 256)
    assert 0 < want[0] < n and got[0] == want[0] and np.array_equal(got[1], want[1])
    for k in want[2]:
        assert np.array_equal(got[2][k], want[2][k]), k
    want = abi.line_capture_host(h.code, None, fmt, bits, None, n, 0, 1, 1, 4, lib)  # no line, no sent word: a page of the syndromes
    got = dec.line_capture_device(None, fmt, d_bits.data_ptr(), None, n, 0, 1, 1, 4)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and all(np.array_equal(got[2][k], want[2][k]) for k in want[2])


# ---- lnsfaid_create at and beyond its limits --------------------------------------------------------------------------------------------
def _create(abi, lib, holder, cfg, max_groups=1):
    ctx = C.c_void_p()
    rc = lib.lnsfaid_create(C.byref(ctx), C.byref(holder.code), C.byref(cfg), 0, max_groups)
    if rc == 0:
        lib.lnsfaid_destroy(ctx)
    return rc


@pytest.mark.parametrize("bad,good", list(cs.REFUSED.items()))
def test_create_refuses_what_lies_beyond_a_limit(abi, lib, bad, good):
    """33 block rows, a degree of 25, a degree of 1, a block column twice in a row, a descending row, a column of weight 17, an LDS
    image beyond 16-bit addresses: LNSFAID_E_CODE; the neighbour on the other side of the limit is accepted"""
    cfg = cs.cfg_of(abi, lib, "m2")
    assert _create(abi, lib, cs.build(cs.limit_shape(bad), abi), cfg) == E_CODE
    assert b"quasi-cyclic" in lib.lnsfaid_strerror(E_CODE)
    assert _create(abi, lib, cs.build(cs.limit_shape(good), abi), cfg) == 0


def _zero_group(h, sigma, seed):
    return cs.group_layout(cs.qpsk_awgn(np.zeros((32, h.N), np.int8), sigma, seed), h.K)


# sigma per component: the CPU port stops early on the group of rows32 and degree2 (DecodeMethod 2 records [[5, 0]] and [[6, 0]]) and
# runs every iteration and the bit-flipping stage on degree24 and lds_last ([[10, 10]], 1 frame of 32 wrong)
LIMIT_SIGMA = {"rows32": 0.30, "degree24": 0.25, "degree2": 0.30, "lds_last": 0.26}


@pytest.mark.parametrize("good", list(LIMIT_SIGMA))
def test_codes_on_a_limit_decode_like_the_port(abi, lib, good):
    """the last accepted code of a limit decodes one group like the CPU port - `lds_last` is the widest code the 16-bit LDS
    addresses take (20 x 224 blocks, N = 57344, an LDS image of 65320 bytes)"""
    h = cs.build(cs.limit_shape(good), abi)
    fix = _zero_group(h, LIMIT_SIGMA[good], 77)
    for key in ("m2", "m1"):
        cfg = cs.cfg_of(abi, lib, key)
        ref, ref_st = oa.Oracle(h, cfg, "avx2").decode(fix, 1)
        dec = abi.Decoder(h, cfg, device=0, max_groups=1, lib=lib)
        out, st = dec.decode(fix, 1)
        wg, lim = dec.kernel_residency()
        dec.close()
        print("%s %s: records %s, kernel_residency (%d, %d)" % (good, key, st.tolist(), wg, lim))
        assert np.array_equal(out, ref), (good, key, _bad_frames(h, out, ref))
        assert np.array_equal(st, ref_st), (good, key, st.tolist(), ref_st.tolist())


def test_a_column_of_weight_16(abi, lib):
    """accepted for DecodeMethod 2, refused at creation for DecodeMethod 3 (its vote count has four bit planes), and lnsfaid_set_cfg
    to DecodeMethod 3 on the accepted context is refused and leaves it decoding as before"""
    h = cs.build(cs.limit_shape("weight16"), abi)
    assert cs.column_weights(h.shape).max() == 16
    cfg2, cfg3 = cs.cfg_of(abi, lib, "m2"), cs.cfg_of(abi, lib, "m3")
    assert _create(abi, lib, h, cfg3) == E_CODE
    fix = _zero_group(h, 0.34, 78)
    ref, ref_st = oa.Oracle(h, cfg2, "avx2").decode(fix, 1)
    dec = abi.Decoder(h, cfg2, device=0, max_groups=1, lib=lib)
    out, st = dec.decode(fix, 1)
    assert np.array_equal(out, ref) and np.array_equal(st, ref_st), (st.tolist(), ref_st.tolist())
    assert lib.lnsfaid_set_cfg(dec.ctx, C.byref(cfg3)) == E_CODE
    out, st = dec.decode(fix, 1)
    dec.close()
    assert np.array_equal(out, ref) and np.array_equal(st, ref_st), (st.tolist(), ref_st.tolist())


# ---- residency --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.NAMES)
def test_kernel_residency(abi, lib, decoders, name):
    """the residency of the default selection: what the LDS image of this shape allows, at most the 8 the kernels are built for"""
    h = cs.code(name)
    lds = cs.lds_bytes(h.N, h.M)
    dec = decoders(name, "m2")
    _reset(dec)
    wg, lim = dec.kernel_residency()
    print("%s: LDS image %d bytes, kernel_residency (%d, %d)" % (name, lds, wg, lim))
    assert wg == lim, (name, wg, lim)
    assert lim == min(8, 160 * 1024 // lds), (name, lim, lds)
