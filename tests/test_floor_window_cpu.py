"""The case table of tests/floor_window_cases.py without a GPU: the scalar oracle equals the AVX2 port on every case (the link the
large-batch GPU tests rest on, tested elsewhere at the presets only); every case tells a wrong window rule from the right one (the
sensitivity conditions, asserted on the reference so that an edit of a batch or of the table cannot turn a case into a no-op); the
host-compiled layer step (oracle/libswar_emul.so) follows the oracle when the window moves."""
import ctypes as C

import numpy as np
import pytest

import floor_window_cases as fw
import oracle_abi as oa
from test_swar_emul import EMU

FAMILIES = list(fw.FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_equals_the_port_on_every_case(abi, lib, code50, family):
    cases = fw.family_cases(family)
    refs = fw.references(abi, lib, code50, cases)
    port = fw.references(abi, lib, code50, cases, kind="avx2")
    for c, r, p in zip(cases, refs, port):
        frames, records = fw.differ(r, p)
        assert frames == 0 and not records, (fw.case_id(c), frames, r[1].tolist(), p[1].tolist())


@pytest.mark.parametrize("family", FAMILIES)
def test_sensitivity_conditions(abi, lib, code50, family):
    top = fw.FAMILIES[family][2]
    cases = fw.family_cases(family)
    ref = dict(zip(cases, fw.references(abi, lib, code50, cases)))

    def d(a, b):
        frames, records = fw.differ(ref[a], ref[b])
        print("%s against %s: %d frames, records differ: %s" % (fw.case_id(a), fw.case_id(b), frames, records))
        return frames, records

    # count cast and presets: the window shows against the same case with the window configured away ...
    for c in cases:
        if c.kind not in ("cast", "preset"):
            continue
        frames, records = d(c, fw.twin(c))
        if c.kind == "cast" and c.count in fw.NEVER[family]:
            assert (frames, records) == (0, False), fw.case_id(c)  # ... or, where the cast leaves a count nothing is below, does not
        elif not (c.kind == "preset" and (family, c.batch) in fw.INSENSITIVE_PRESETS):
            assert frames >= 8 or records, fw.case_id(c)
    # the two casts: top is the largest count left as it is, top + 1 wraps to "never"
    assert d(fw.find(family, "cast", count=top), fw.find(family, "cast", count=top + 1))[0] >= 16
    if family in fw.OMS:  # (uint8_t)-1 is the top
        assert d(fw.find(family, "cast", count=-1), fw.find(family, "cast", count=top)) == (0, False)
    # a count above 256 is its low byte
    wrap = fw.WRAP[family]
    assert 0 < wrap - 256 <= top
    low = fw.Case(family, "cast", "channel", 6, 6, wrap - 256)
    assert fw.differ(ref[fw.find(family, "cast", count=wrap)], fw.reference(abi, lib, code50, low)) == (0, False)
    # `<`, not `<=`
    lo, hi = fw.BOUNDARY[family]
    assert hi == lo + 1 and hi <= top
    assert d(fw.find(family, "boundary", count=lo), fw.find(family, "boundary", count=hi))[0] >= 1
    # where the window begins: every step of the threshold up to the number of iterations shows, none beyond does
    pos = [fw.find(family, "position", thresh=t) for t in (-1, 0, 1, 2, 3, fw.HUGE)]
    for a, b in zip(pos[:3], pos[1:4]):
        frames, records = d(a, b)
        assert frames >= 1 or records, (fw.case_id(a), fw.case_id(b))
    for c in pos[4:]:
        assert d(pos[3], c) == (0, False), fw.case_id(c)


@pytest.mark.parametrize("family", ["m1", "m5"])
def test_emulated_layer_step_follows_the_window(abi, lib, code50, family):
    """csrc/lnsfaid_swar.h compiled for the host against the oracle's a-posteriori LLRs after the three iterations of the position
    cases, first group of `near_clean`, with the compile-time-degree instances and without.  The entry point takes the
    configuration and derives `lme` and `window` from it like a kernel does, so the two integers reach the layer step from outside."""
    olib = oa.load()
    olib.lnsfaid_oracle_layered_en.restype = C.c_int
    olib.lnsfaid_oracle_layered_en.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    em = C.CDLL(EMU)
    em.swar_emul_layered.restype = C.c_int
    em.swar_emul_layered.argtypes = [C.POINTER(abi.Code), C.POINTER(abi.Cfg), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    fix = np.ascontiguousarray(fw.batch(code50, "near_clean")[:32 * code50.N])
    en = {}
    for thresh in (-1, 0, 1, 2, 3, fw.HUGE):
        c = fw.find(family, "position", thresh=thresh)
        cfg = fw.cfg_of(abi, lib, c)
        o = oa.Oracle(code50, cfg)
        ref = np.empty(32 * code50.N, dtype=np.int8)
        assert olib.lnsfaid_oracle_layered_en(o.h, fix.ctypes.data, c.max_iter, ref.ctypes.data) == 0
        o.close()
        for spec in (0, 1):
            got = np.empty(32 * code50.N, dtype=np.int8)
            assert em.swar_emul_layered(C.byref(code50.code), C.byref(cfg), fix.ctypes.data, c.max_iter, spec, got.ctypes.data) == 0
            bad = np.nonzero(ref != got)[0]
            assert bad.size == 0, (thresh, spec, bad[:8].tolist(), ref[bad[:8]].tolist(), got[bad[:8]].tolist())
        en[thresh] = ref
    # the window moved: the a-posteriori LLRs differ between thresholds -1, 0, 1 and 2 and are the same from 2 on
    for a, b in ((-1, 0), (0, 1), (1, 2)):
        assert not np.array_equal(en[a], en[b]), (a, b)
    for t in (3, fw.HUGE):
        assert np.array_equal(en[2], en[t]), t
