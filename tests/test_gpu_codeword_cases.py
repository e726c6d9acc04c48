"""Every decode kernel on random codewords of the built-in code, against the CPU port (tests/codeword_cases.py holds the batches, the
table of kernel selections and the cached references; tests/test_codeword_cases_cpu.py pins them without a GPU).  One context per
(DecodeMethod, batch), kept for the module; every comparison is byte for byte.

The int8 group rule on each kernel a context can be steered to through the lnsfaid_select_* calls - the selection asserted through
the library's own queries before the launch, a refusal asserted where the table lists one, any other refusal a failure - and a
second time with floor_iter_thresh = -1 for the DecodeMethods whose preset window keeps them off the window-free kernels.  Then the
other ways into a decode kernel: the packed group entry, the per-codeword entries (int8 and packed), the line entry and the burst
entry, each against the per-codeword rule of the CPU port on the image the entry is defined to decode; every device output of the
line and burst entries lies between guard words."""
import numpy as np
import pytest

import burst_ref as br
import codeword_cases as cc
import early_stop_ref as esr
import line_ref as lr
import oracle_abi as oa

pytestmark = pytest.mark.gpu

NG, FRAMES = cc.NG, cc.FRAMES
GUARD = 64
PATTERN = 0x5A5AA5A5  # fits an int32


@pytest.fixture(scope="module")
def decoders(abi, lib, code50):
    """(DecodeMethod, batch) -> its one context, created on first use and kept until the module is done"""
    made = {}

    def get(method, name):
        if (method, name) not in made:
            made[(method, name)] = abi.Decoder(code50, cc.cfg_of(abi, lib, method), device=0, max_groups=NG, lib=lib)
        return made[(method, name)]

    yield get
    for d in made.values():
        d.close()


def _reset(dec):
    dec.select_waves(0)
    dec.select_kernel(0)
    dec.select_message_store(0)
    dec.select_zero_shift(0)
    dec.select_edge_words(True)


def _queries(dec):
    """(rotation-free, layer-static, window-free, edge words, rows per lane, waves per codeword, message store)"""
    return (dec.zero_shift_groups(12)[0], dec.static_layers(), dec.window_free(), dec.edge_words(), dec.rows_per_lane(),
            dec.kernel_waves(), dec.message_store())


def _select(abi, dec, method, free, selection):
    """steer `dec` (its configuration already set; free: it cannot open the error-floor window) to `selection` and assert through
    the queries that the intended kernel runs next.  Returns "run", "refused" (the refusal asserted) or "absent" (see
    codeword_cases.selection_state; the queries asserted)"""
    REG, HBM = abi.MSG_REGISTERS, abi.MSG_HBM
    _reset(dec)
    nms = method == 0
    default = (False, False, False, False, 4, 1, HBM) if nms else (True, True, free, free, 4, 1, REG)
    state = cc.selection_state(method, "off" if free and method in cc.WINDOW_METHODS else "preset", selection)
    calls = {"edge_off": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_STATIC), "windowed": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED),
             "loop": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_LOOP), "on": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_ON),
             "rotating": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_OFF), "hbm": lambda: dec.select_message_store(HBM),
             "rows2": lambda: dec.select_kernel(2), "waves2": lambda: dec.select_waves(2), "default": lambda: None}
    if state == "refused":
        with pytest.raises(RuntimeError):
            calls[selection]()
        assert _queries(dec) == default  # a refused call changes nothing
        return state
    if selection == "hbm" and "registers" in cc.REFUSED.get(method, ()):
        with pytest.raises(RuntimeError):
            dec.select_message_store(REG)
    calls[selection]()
    got = _queries(dec)
    if selection in ("default", "on"):
        want = default
    elif selection == "edge_off":
        dec.select_edge_words(False)
        got = _queries(dec)
        want = (True, True, free, False, 4, 1, REG)
    elif selection == "windowed":
        want = (True, True, False, False, 4, 1, REG)
    elif selection == "loop":
        want = (True, False, False, False, 4, 1, REG)
    elif selection == "rotating":
        want = (False, False, False, False, 4, 1, HBM if nms else REG)
    elif selection == "hbm":
        want = (False, False, False, False, 4, 1, HBM)
    elif selection == "rows2":
        want = (False, False, False, False, 2, 1, HBM)
    elif selection == "waves2":
        want = (False, False, False, False, 4, 2, HBM)
    else:
        raise AssertionError(selection)
    assert got == want, (method, free, selection, got, want)
    assert (state == "absent") == (selection == "edge_off" and not free), (state, selection, free)
    return state


def _bad_frames(code50, out, ref):
    return np.nonzero((np.asarray(out).reshape(-1, code50.N) != np.asarray(ref).reshape(-1, code50.N)).any(axis=1))[0][:8].tolist()


_counts = {}


def _reference_counters(abi, lib, code50, method, name, window):
    """lnsfaid_oracle_count_errors of the CPU port's decisions given the sent information bits"""
    k = (method, name, window)
    if k not in _counts:
        ref, _ = cc.reference(abi, lib, code50, method, name, window)
        _counts[k] = oa.Oracle(code50, cc.cfg_of(abi, lib, method, window)).count_errors(ref, cc.sent_info(code50), NG)
    return _counts[k]


def _compare_group(abi, lib, code50, dec, method, name, window, what, out, st):
    ref, ref_st = cc.reference(abi, lib, code50, method, name, window)
    print("DecodeMethod %d %s window %s on %s: iterations / bit-flipping iterations %s" % (method, name, window, what, st.tolist()))
    assert np.array_equal(out, ref), (method, name, window, what, _bad_frames(code50, out, ref))
    assert np.array_equal(st, ref_st), (method, name, window, what, st.tolist(), ref_st.tolist())
    info = cc.sent_info(code50)
    assert dec.count_errors(out, info, NG) == _reference_counters(abi, lib, code50, method, name, window), (method, name, window, what)


# ---- the int8 group rule, every kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", cc.SELECTIONS)
@pytest.mark.parametrize("name", cc.BATCHES)
@pytest.mark.parametrize("method", cc.METHODS)
def test_group_decode_equals_the_port(abi, lib, code50, decoders, method, name, selection):
    dec = decoders(method, name)
    fix = cc.batch(code50, method, name)
    try:
        for window in cc.windows_of(method):
            cfg = cc.cfg_of(abi, lib, method, window)
            dec.set_cfg(cfg)
            state = _select(abi, dec, method, cfg.floor_iter_thresh < 0, selection)
            assert state == cc.selection_state(method, window, selection)
            if state != "run":
                continue
            out, st = dec.decode(fix, NG)
            _compare_group(abi, lib, code50, dec, method, name, window, selection, out, st)
    finally:
        dec.set_cfg(cc.cfg_of(abi, lib, method))
        _reset(dec)


# ---- the packed group entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.BATCHES)
@pytest.mark.parametrize("method", cc.METHODS)
def test_packed_decode_equals_the_port(abi, lib, code50, decoders, method, name):
    """lnsfaid_decode_packed on lnsfaid_pack_llr4 of the batch (minus8: the one nibble the int8 batches of the other tests never hold)"""
    dec = decoders(method, name)
    llr4 = abi.pack_llr4(cc.batch(code50, method, name), lib)
    assert np.array_equal(llr4, lr.pack_nibbles(cc.batch(code50, method, name)))
    try:
        for window in cc.windows_of(method):
            dec.set_cfg(cc.cfg_of(abi, lib, method, window))
            _reset(dec)
            bits, st = dec.decode_packed(llr4, NG)
            assert np.array_equal(bits.reshape(FRAMES, -1), cc.pack_frames(cc.reference(abi, lib, code50, method, name, window)[0].reshape(FRAMES, -1)))
            _compare_group(abi, lib, code50, dec, method, name, window, "packed", abi.unpack_bits(bits, lib), st)
    finally:
        dec.set_cfg(cc.cfg_of(abi, lib, method))


# ---- the per-codeword rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.BATCHES)
@pytest.mark.parametrize("method", cc.METHODS)
def test_codeword_decode_equals_the_port(abi, lib, code50, decoders, method, name):
    """lnsfaid_decode_codewords and lnsfaid_decode_codewords_packed: decisions, iterations and bf_iterations of every codeword
    against 32 copies of it through the CPU port, `unsatisfied` against numpy's H x of the reference decisions"""
    dec = decoders(method, name)
    _reset(dec)
    fix = cc.batch(code50, method, name)
    ref, ref_st = cc.codeword_reference(abi, lib, code50, method, name)
    want_unsat = esr.unsatisfied(code50, ref)
    out, cw = dec.decode_codewords(fix, NG)
    print("DecodeMethod %d %s: own iterations %s" % (method, name, np.bincount(cw[:, 0], minlength=cc.MAX_ITER + 1).tolist()))
    assert np.array_equal(out.reshape(FRAMES, -1), ref), (method, name, _bad_frames(code50, out, ref))
    assert np.array_equal(cw[:, :2], ref_st), (method, name, np.nonzero((cw[:, :2] != ref_st).any(axis=1))[0][:8].tolist())
    assert np.array_equal(cw[:, 2], want_unsat), (method, name)
    bits, cwp = dec.decode_codewords_packed(abi.pack_llr4(fix, lib), NG)
    assert np.array_equal(bits.reshape(FRAMES, -1), cc.pack_frames(ref)), (method, name, "packed")
    assert np.array_equal(cwp[:, :2], ref_st) and np.array_equal(cwp[:, 2], want_unsat), (method, name, "packed")
    assert dec.early_stop() == abi.STOP_GROUP


# ---- the line and burst entries --------------------------------------------------------------------------------------------------------
def _guarded(torch, n_words):
    t = torch.full((GUARD + n_words + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 4 * GUARD


def _inside(t, n_words):
    """the words between the guards, after checking both guards"""
    h = t.cpu().numpy()
    assert (h[:GUARD] == PATTERN).all() and (h[GUARD + n_words:] == PATTERN).all(), "a guard word was overwritten"
    return h[GUARD:GUARD + n_words].view(np.uint32)


def _to_device(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _line_params():
    for name, fmt, magnitude in cc.LINE_CASES:
        for method in cc.line_methods(fmt):
            yield pytest.param(method, name, fmt, magnitude, id="m%d-%s" % (method, name))


def _compare_stats(st, n, ref_st, unsatisfied, corrected, what):
    assert np.array_equal(st["iterations"], ref_st[:n, 0]), (what, "iterations", st["iterations"][:8].tolist(), ref_st[:8, 0].tolist())
    assert np.array_equal(st["bf_iterations"], ref_st[:n, 1]), (what, "bf_iterations", st["bf_iterations"][:8].tolist(), ref_st[:8, 1].tolist())
    assert np.array_equal(st["unsatisfied"], unsatisfied[:n]), (what, "unsatisfied")
    assert np.array_equal(st["corrected"], corrected), (what, "corrected", st["corrected"][:8].tolist(), corrected[:8].tolist())


@pytest.mark.parametrize("method,name,fmt,magnitude", list(_line_params()))
def test_line_decode_equals_the_port(abi, lib, code50, decoders, method, name, fmt, magnitude):
    """lnsfaid_decode_line_device: payload, bits and the four statistics of 96 codewords and of the first 33; `corrected` counted in
    numpy by the rule of include/lnsfaid.h (positions k < L where the decision differs from the channel's own)"""
    import torch
    N, K, L = code50.N, code50.K, code50.N - cc.PUNCTURED
    kw, lw, nw = K // 32, L // 32, N // 32
    dec = decoders(method, name)
    _reset(dec)
    line, ref, ref_st = cc.line_case(abi, lib, code50, method, name, fmt, magnitude)
    want_bits, unsat = cc.pack_frames(ref), esr.unsatisfied(code50, ref)
    per = lw if fmt == lr.HARD else L // 2
    for n in cc.LINE_COUNTS:
        part = line[:n * per]
        corrected = (ref[:n, :L] != lr.channel_decisions(part, n, L, fmt)).sum(axis=1)
        d_line = _to_device(torch, part)
        d_pay, p_pay = _guarded(torch, n * kw)
        d_bits, p_bits = _guarded(torch, n * nw)
        d_st, p_st = _guarded(torch, n * 4)
        torch.cuda.synchronize()
        dec.decode_line_device(d_line.data_ptr(), fmt, n, p_pay, p_bits, p_st, magnitude if fmt == lr.HARD else 0)
        payload, bits = _inside(d_pay, n * kw).reshape(n, kw), _inside(d_bits, n * nw).reshape(n, nw)
        st = _inside(d_st, n * 4).view(abi.line_stats_dtype())
        bad = np.nonzero((bits != want_bits[:n]).any(axis=1))[0]
        assert bad.size == 0, (method, name, n, "bits", bad[:8].tolist())
        assert np.array_equal(payload, want_bits[:n, :kw]), (method, name, n, "payload")
        _compare_stats(st, n, ref_st, unsat, corrected, (method, name, n))
    print("DecodeMethod %d %s: %d of %d codewords stop early, %d end with unsatisfied checks" % (
        method, name, int((ref_st[:, 0] < cc.MAX_ITER).sum()), FRAMES, int((unsat > 0).sum())))


@pytest.mark.parametrize("where", [br.TAIL, br.HEAD], ids=["tail", "head"])
@pytest.mark.parametrize("method,name,fmt,magnitude", list(_line_params()))
def test_burst_decode_equals_the_port(abi, lib, code50, decoders, method, name, fmt, magnitude, where):
    """lnsfaid_decode_burst_device with S_c cycling through 0, 5760 and K - 32: payload, bits, the four statistics and short_ones
    of 96 codewords and of the first 33"""
    import torch
    N, K, L = code50.N, code50.K, code50.N - cc.PUNCTURED
    nw = N // 32
    dec = decoders(method, name)
    _reset(dec)
    rx, ref, ref_st = cc.burst_case(abi, lib, code50, method, name, fmt, magnitude, where)
    want_bits, unsat = cc.pack_frames(ref), esr.unsatisfied(code50, ref)
    for n in cc.LINE_COUNTS:
        s = cc.burst_shortened()[:n]
        line = br.burst_line_of(rx[:n], K, L, fmt, s, where)
        line_bits, payload_bits = br.burst_words(n, K, L, s)
        assert (line_bits, payload_bits) == abi.burst_words(code50.code, s, n, lib)
        pw = payload_bits // 32
        corrected, ones = br.counts(want_bits[:n], line, N, K, L, fmt, s, where)
        d_line = _to_device(torch, line)
        d_pay, p_pay = _guarded(torch, pw)
        d_bits, p_bits = _guarded(torch, n * nw)
        d_st, p_st = _guarded(torch, n * 4)
        d_ones, p_ones = _guarded(torch, n)
        torch.cuda.synchronize()
        dec.decode_burst_device(d_line.data_ptr(), fmt, s, where, n, p_pay, p_bits, p_st, p_ones, magnitude if fmt == lr.HARD else 0)
        payload, bits = _inside(d_pay, pw), _inside(d_bits, n * nw).reshape(n, nw)
        st, got_ones = _inside(d_st, n * 4).view(abi.line_stats_dtype()), _inside(d_ones, n)
        bad = np.nonzero((bits != want_bits[:n]).any(axis=1))[0]
        assert bad.size == 0, (method, name, where, n, "bits", bad[:8].tolist())
        assert np.array_equal(payload, br.payload_of_bits(want_bits[:n], K, s, where)), (method, name, where, n, "payload")
        _compare_stats(st, n, ref_st, unsat, corrected, (method, name, where, n))
        assert np.array_equal(got_ones, ones), (method, name, where, n, "short_ones")
    print("DecodeMethod %d %s where %d: %d of %d codewords stop early, %d end with unsatisfied checks" % (
        method, name, where, int((ref_st[:, 0] < cc.MAX_ITER).sum()), FRAMES, int((unsat > 0).sum())))
