"""The error-floor window off its presets on every decode kernel (tests/floor_window_cases.py holds the batches, the case table and
the cached references).  Every case's hard decisions and group records byte for byte against the scalar oracle, on each kernel
path a context can be steered to, with the selection asserted through the library's own queries; one context per family moves
from case to case with lnsfaid_set_cfg, so the live switch between the layer-static kernel and its window-free twin is part of
every test.  The per-codeword entries against the 32-copies restatement through the CPU port, the line entry against the packed
per-codeword entry on lnsfaid_line_to_llr4's output."""
import concurrent.futures
import ctypes as C

import numpy as np
import pytest

import floor_window_cases as fw
import oracle_abi as oa

pytestmark = pytest.mark.gpu

NG = fw.NG
KINDS = ("cast", "boundary", "position", "presets")  # "presets": the preset and window-off cases of both batches
PATHS = ("default", "loop", "rotating", "hbm", "rows2", "waves2", "packed")
# what a family has no instance of: lnsfaid_select_* refuses it (asserted below)
REFUSED = {"m2ef1": ("rows2",), "m2ef2": ("rows2", "waves2", "loop")}
# EF_ELIMINATION 2 keeps its messages in HBM and has no rotation-free instance: its default selection already is the rotating
# four-rows kernel with messages through HBM, so these two paths would repeat "default"
SAME_AS_DEFAULT = {"m2ef2": ("rotating", "hbm")}


@pytest.fixture(scope="module")
def decoders(abi, lib, code50):
    """family -> its one context, created on first use and kept until the module is done"""
    made = {}

    def get(family):
        if family not in made:
            made[family] = abi.Decoder(code50, fw.cfg_of(abi, lib, fw.family_cases(family)[0]), device=0, max_groups=NG, lib=lib)
        return made[family]

    yield get
    for d in made.values():
        d.close()


def _cases(family, kind):
    return [c for c in fw.family_cases(family) if (c.kind in ("preset", "off") if kind == "presets" else c.kind == kind)]


def _reset(dec):
    dec.select_waves(0)
    dec.select_kernel(0)
    dec.select_message_store(0)
    dec.select_zero_shift(0)


def _select(abi, dec, family, path, thresh):
    """steer `dec` (its configuration already set) to `path` and assert through the queries that the path is what runs next"""
    registers = family != "m2ef2"  # the erasing instance streams its messages
    _reset(dec)
    if path in ("default", "packed"):
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1
        assert dec.message_store() == (abi.MSG_REGISTERS if registers else abi.MSG_HBM)
        assert dec.zero_shift_groups()[0] == registers and dec.static_layers() == registers
        assert dec.window_free() == (registers and thresh < 0), thresh
    elif path == "loop":
        dec.select_zero_shift(abi.ZERO_SHIFT_LOOP)
        on, groups = dec.zero_shift_groups()
        assert on and max(groups) >= 1 and not dec.static_layers() and not dec.window_free()
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1 and dec.message_store() == abi.MSG_REGISTERS
    elif path == "rotating":
        dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
        assert not dec.zero_shift_groups()[0] and not dec.static_layers() and not dec.window_free()
        assert dec.rows_per_lane() == 4 and dec.kernel_waves() == 1 and dec.message_store() == abi.MSG_REGISTERS
    elif path == "hbm":
        dec.select_message_store(abi.MSG_HBM)
        assert dec.message_store() == abi.MSG_HBM and dec.rows_per_lane() == 4 and dec.kernel_waves() == 1
        assert not dec.zero_shift_groups()[0] and not dec.static_layers() and not dec.window_free()
    elif path == "rows2":
        dec.select_kernel(2)
        assert dec.rows_per_lane() == 2 and dec.kernel_waves() == 1 and dec.message_store() == abi.MSG_HBM
        assert not dec.zero_shift_groups()[0] and not dec.static_layers() and not dec.window_free()
    elif path == "waves2":
        dec.select_waves(2)
        assert dec.kernel_waves() == 2 and dec.rows_per_lane() == 4 and dec.message_store() == abi.MSG_HBM
        assert not dec.zero_shift_groups()[0] and not dec.static_layers() and not dec.window_free()
    else:
        raise AssertionError(path)


def _bad_frames(code50, out, ref):
    return np.nonzero((out.reshape(fw.FRAMES, code50.N) != ref.reshape(fw.FRAMES, code50.N)).any(axis=1))[0][:8].tolist()


def _params():
    for family in fw.FAMILIES:
        for path in PATHS:
            if path in SAME_AS_DEFAULT.get(family, ()):
                continue
            for kind in KINDS:
                yield pytest.param(family, path, kind, id="%s-%s-%s" % (family, path, kind))


@pytest.mark.parametrize("family,path,kind", list(_params()))
def test_group_decode_equals_the_oracle(abi, lib, code50, decoders, family, path, kind):
    dec = decoders(family)
    if path in REFUSED.get(family, ()):
        _reset(dec)
        with pytest.raises(RuntimeError):
            {"rows2": lambda: dec.select_kernel(2), "waves2": lambda: dec.select_waves(2),
             "loop": lambda: dec.select_zero_shift(abi.ZERO_SHIFT_LOOP)}[path]()
        return
    cases = _cases(family, kind)
    refs = fw.references(abi, lib, code50, cases)
    for c, (ref, ref_st) in zip(cases, refs):
        cfg = fw.cfg_of(abi, lib, c)
        dec.set_cfg(cfg)
        _select(abi, dec, family, path, cfg.floor_iter_thresh)
        fix = fw.batch(code50, c.batch)
        if path == "packed":
            bits, st = dec.decode_packed(abi.pack_llr4(fix, lib), NG)
            out = abi.unpack_bits(bits, lib)
        else:
            out, st = dec.decode(fix, NG)
        print("%s on %s: iterations / bit-flipping iterations %s" % (fw.case_id(c), path, st.tolist()))
        assert np.array_equal(out, ref), (fw.case_id(c), path, _bad_frames(code50, out, ref))
        assert np.array_equal(st, ref_st), (fw.case_id(c), path, st.tolist(), ref_st.tolist())
        if path == "default" and dec.window_free():
            # the layer-static kernel itself with a window its threshold keeps shut
            dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED)
            assert dec.static_layers() and not dec.window_free()
            out, st = dec.decode(fix, NG)
            assert np.array_equal(out, ref), (fw.case_id(c), "windowed", _bad_frames(code50, out, ref))
            assert np.array_equal(st, ref_st), (fw.case_id(c), "windowed", st.tolist(), ref_st.tolist())
    _reset(dec)


def _codeword_pairs(family):
    """neighbours under the per-codeword rule: (top, top + 1), the `<` pair, thresholds 0 and 1 of the position cases"""
    top = fw.FAMILIES[family][2]
    lo, hi = fw.BOUNDARY[family]
    return [(fw.find(family, "cast", count=top), fw.find(family, "cast", count=top + 1)),
            (fw.find(family, "boundary", count=lo), fw.find(family, "boundary", count=hi)),
            (fw.find(family, "position", thresh=0), fw.find(family, "position", thresh=1))]


@pytest.mark.parametrize("pair", [0, 1, 2], ids=["top", "boundary", "position"])
@pytest.mark.parametrize("family", list(fw.FAMILIES))
def test_codeword_decode_equals_the_port(abi, lib, code50, decoders, family, pair):
    """lnsfaid_decode_codewords and lnsfaid_decode_codewords_packed: decisions and iterations / bf_iterations of every codeword"""
    dec = decoders(family)
    a, b = _codeword_pairs(family)[pair]
    ra, rb = fw.references(abi, lib, code50, [a, b], kind="avx2", rule="codeword")
    frames, records = fw.differ(ra, rb)
    print("%s against %s under the per-codeword rule: %d frames differ, records differ: %s" % (fw.case_id(a), fw.case_id(b), frames, records))
    assert frames >= 1 or records, "the two cases do not tell a wrong window from a right one under the per-codeword rule"
    for c, (ref, ref_st) in ((a, ra), (b, rb)):
        dec.set_cfg(fw.cfg_of(abi, lib, c))
        _reset(dec)
        fix = fw.batch(code50, c.batch)
        out, cw = dec.decode_codewords(fix, NG)
        assert np.array_equal(out, ref), (fw.case_id(c), _bad_frames(code50, out, ref))
        assert np.array_equal(cw[:, :2], ref_st), (fw.case_id(c), np.nonzero((cw[:, :2] != ref_st).any(axis=1))[0][:8].tolist())
        bits, cwp = dec.decode_codewords_packed(abi.pack_llr4(fix, lib), NG)
        out = abi.unpack_bits(bits, lib)
        assert np.array_equal(out, ref), (fw.case_id(c), "packed", _bad_frames(code50, out, ref))
        assert np.array_equal(cwp, cw), (fw.case_id(c), "packed")


@pytest.mark.parametrize("family", list(fw.FAMILIES))
def test_line_decode_equals_the_packed_codeword_entry(abi, lib, code50, decoders, family):
    """lnsfaid_decode_line with LINE_LLR4 on the line of `channel`: payload and statistics of the packed per-codeword call on
    lnsfaid_line_to_llr4's output (the definition tests/test_gpu_line.py uses), at top and top + 1"""
    dec = decoders(family)
    code = code50.code
    n, kw = fw.FRAMES, code50.K // 32
    fix = fw.batch(code50, "channel")
    line = abi.line_from_fixinput(code, fix, n, abi.LINE_LLR4, lib)
    llr4 = abi.line_to_llr4(code, line, abi.LINE_LLR4, 0, n, lib)
    top = fw.FAMILIES[family][2]
    seen = []
    for count in (top, top + 1):
        dec.set_cfg(fw.cfg_of(abi, lib, fw.find(family, "cast", count=count)))
        _reset(dec)
        want_bits, want_cw = dec.decode_codewords_packed(llr4, NG)
        payload, bits, st = dec.decode_line(line, abi.LINE_LLR4, n, magnitude=0, with_bits=True)
        want_bits = want_bits.reshape(n, code50.N // 32)
        assert np.array_equal(bits, want_bits), count
        assert np.array_equal(payload, want_bits[:, :kw]), count
        for i, name in enumerate(("iterations", "bf_iterations", "unsatisfied")):
            assert np.array_equal(st[name], want_cw[:, i]), (count, name)
        seen.append((payload.copy(), st.copy()))
    # the two counts are told apart on this entry too
    assert not (np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1]))


def test_live_switching_between_the_window_free_kernel_and_its_twin(abi, lib, code50):
    """one context, a fixed sequence of lnsfaid_set_cfg calls: the selection follows floor_iter_thresh at once, both ways, and
    every decode of `channel` is the oracle's for the configuration in force"""
    def cfg(method, thresh=None, ef=None, count=None):
        c = abi.default_cfg(method, 6, lib)
        if ef is not None:
            assert lib.lnsfaid_cfg_ef_elimination(C.byref(c), ef) == 0
        if thresh is not None:
            c.floor_iter_thresh = thresh
        if count is not None:
            c.floor_err_count = count
        return c

    steps = [  # (configuration, window-free, the step whose results it must repeat)
        (cfg(2, -1), True, None),
        (cfg(2, 6, ef=1), False, None),
        (cfg(2, 6, ef=0, count=127), False, 0),  # without the _ef tables an open window changes nothing
        (cfg(1, -1), True, None),
        (cfg(1), False, None),
        (cfg(2, -1), True, 0),
    ]
    assert steps[0][0].floor_iter_thresh < 0 and steps[0][0].ef_elimination == 0 and steps[4][0].floor_iter_thresh >= 0
    fix = fw.batch(code50, "channel")
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        refs = list(ex.map(lambda s: oa.decode_mt(code50, s[0], fix, NG, threads=NG), steps[:5]))
    refs.append(refs[0])
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[3][0], refs[4][0])  # the window shows on this batch
    dec = abi.Decoder(code50, steps[0][0], device=0, max_groups=NG, lib=lib)
    for i, (c, window_free, same_as) in enumerate(steps):
        dec.set_cfg(c)
        assert dec.static_layers() and dec.window_free() == window_free, i
        out, st = dec.decode(fix, NG)
        assert np.array_equal(out, refs[i][0]), (i, _bad_frames(code50, out, refs[i][0]))
        assert np.array_equal(st, refs[i][1]), (i, st.tolist(), refs[i][1].tolist())
        if same_as is not None:
            assert np.array_equal(refs[i][0], refs[same_as][0]) and np.array_equal(refs[i][1], refs[same_as][1]), i
    dec.close()
