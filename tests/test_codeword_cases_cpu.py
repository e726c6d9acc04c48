"""The batches of tests/codeword_cases.py without a GPU: on every batch and DecodeMethod the scalar oracle and the CPU port agree, so
the port is a valid reference for tests/test_gpu_codeword_cases.py; the host-compiled layer step (oracle/swar_emul.cpp) leaves the
oracle's En; and every batch meets the conditions it was chosen for.  These are conditions on the reference alone: a batch that no
longer meets one fails here, it is never skipped.

    mixed      DecodeMethods 1 .. 5: a group stops before MAX_ITER and a group runs every layered iteration; a record has
               bf_iterations > 0 where the method has a flip stage; under the per-codeword rule a codeword has 1 <= own iterations
               < its group's.  Every method: at least one frame is decoded wrong and at least one right.
    clean      no wrong frame; DecodeMethods 1 .. 5: every group stops early, the records not all equal
    staggered  DecodeMethods 1 .. 5: own iterations take at least four different values inside one group
    every batch but hard1, DecodeMethods 0, 1, 2, 5: En of the first group reaches +31 and -31 after MAX_ITER iterations
(DecodeMethod 0 has no early stop, and at magnitude 1 no decoder drives En to its limits: see tests/codeword_cases.py.  On hard1 the
test asserts what the reference does instead: both signs, neither limit.)"""
import concurrent.futures
import ctypes as C
import os

import numpy as np
import pytest

import codeword_cases as cc
import oracle_abi as oa

EMU = os.path.join(oa.ORACLE_DIR, "libswar_emul.so")


def test_batches_are_what_the_table_says(code50):
    cw = cc.codewords(code50)
    N, K = code50.N, code50.K
    assert cw.shape == (cc.FRAMES, N) and 0.45 < cw.mean() < 0.55
    for method in cc.METHODS:
        mixed, minus8 = cc.frames(code50, method, "mixed"), cc.frames(code50, method, "minus8")
        assert mixed.min() == -7 and mixed.max() == 7 and minus8.min() == -8 and (minus8 == -7).sum() == 0
        assert np.array_equal(np.where(minus8 == -8, -7, minus8), mixed)
        assert cc.batch(code50, method, "mixed").size == cc.FRAMES * N
    for mag in (1, 4, 7):
        f = cc.frames(code50, 2, "hard%d" % mag)
        flips = ((f > 0) != (cw > 0)).sum(axis=1)
        assert set(np.unique(f).tolist()) == {-mag, mag} and flips.min() > 0.005 * N and flips.max() < 0.015 * N
    assert np.array_equal(cc.frames(code50, 2, "hard1") * 7, cc.frames(code50, 2, "hard7"))
    e = cc.frames(code50, 2, "erasures")
    assert not e[cc.ERASED_LANE::32].any() and e.shape[0] // 32 == cc.NG
    assert np.array_equal(e[cc.COMPLEMENT_LANE::32], np.where(cw[cc.COMPLEMENT_LANE::32] > 0, -7, 7))
    rest = np.ones(cc.FRAMES, bool)
    rest[cc.ERASED_LANE::32] = rest[cc.COMPLEMENT_LANE::32] = False
    assert 0.08 < (e[rest] == 0).mean() < 0.12 and np.array_equal(e[rest][e[rest] != 0] > 0, cw[rest][e[rest] != 0] > 0)
    s = cc.frames(code50, 2, "staggered")
    wrong = ((s > 0) != (cw > 0)).mean(axis=1).reshape(cc.NG, 32).mean(axis=0)
    assert wrong[:8].mean() > 1.5 * wrong[24:].mean()  # the channel gets better along the lanes


@pytest.mark.parametrize("name", cc.BATCHES)
@pytest.mark.parametrize("method", cc.METHODS)
def test_the_scalar_oracle_and_the_port_agree(abi, lib, code50, method, name):
    todo = [(method, name, w, kind) for w in cc.windows_of(method) for kind in ("avx2", "oracle")]
    refs = cc.references(abi, lib, code50, todo)
    for i in range(0, len(todo), 2):
        (port, port_st), (scalar, scalar_st) = refs[i], refs[i + 1]
        print(method, name, todo[i][2], port_st.tolist(), int(cc.wrong_frames(code50, port).sum()), "frames wrong")
        assert np.array_equal(scalar_st, port_st), (todo[i], scalar_st.tolist(), port_st.tolist())
        assert np.array_equal(scalar, port), (todo[i], np.nonzero(cc.wrong_frames(code50, scalar) != cc.wrong_frames(code50, port))[0].tolist())


def _en(abi, lib, code50, method, fix, n_iter, spec):
    olib = oa.load()
    olib.lnsfaid_oracle_layered_en.restype = C.c_int
    olib.lnsfaid_oracle_layered_en.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    em = C.CDLL(EMU)
    em.swar_emul_layered.restype = C.c_int
    em.swar_emul_layered.argtypes = [C.POINTER(abi.Code), C.POINTER(abi.Cfg), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    cfg = cc.cfg_of(abi, lib, method)
    ref = np.empty(32 * code50.N, dtype=np.int8)
    if spec is None:
        o = oa.Oracle(code50, cfg)  # (kept in a name: the call must not outlive it)
        assert olib.lnsfaid_oracle_layered_en(o.h, fix.ctypes.data, n_iter, ref.ctypes.data) == 0
        o.close()
    else:
        assert em.swar_emul_layered(C.byref(code50.code), C.byref(cfg), fix.ctypes.data, n_iter, spec, ref.ctypes.data) == 0
    return ref


@pytest.mark.parametrize("name", cc.BATCHES)
@pytest.mark.parametrize("method", cc.SWAR_METHODS)
def test_the_layer_step_leaves_the_oracles_en(abi, lib, code50, method, name):
    """the first group, after 1 and MAX_ITER iterations, both `spec` values; and En spans -31 .. 31"""
    fix = np.ascontiguousarray(cc.batch(code50, method, name)[:32 * code50.N])
    runs = [(n_iter, spec) for n_iter in (1, cc.MAX_ITER) for spec in (None, 0, 1)]  # spec None: the oracle
    with concurrent.futures.ThreadPoolExecutor(len(runs)) as ex:  # (the libraries release the interpreter)
        en = dict(zip(runs, ex.map(lambda r: _en(abi, lib, code50, method, fix, r[0], r[1]), runs)))
    for n_iter, spec in runs:
        ref, got = en[(n_iter, None)], en[(n_iter, spec)]
        bad = np.nonzero(ref != got)[0]
        assert bad.size == 0, (n_iter, spec, bad[:8].tolist(), ref[bad[:8]].tolist(), got[bad[:8]].tolist())
    ref = en[(cc.MAX_ITER, None)]
    print(method, name, "En after %d iterations: %d .. %d" % (cc.MAX_ITER, ref.min(), ref.max()))
    if (method, name) in cc.EN_STAYS:
        want = cc.frames(code50, method, name)[:32].copy()  # (En comes frame-major; the punctured tail enters as 0)
        want[:, code50.N - cc.PUNCTURED:] = 0
        assert np.array_equal(ref.reshape(32, code50.N), want)
    elif name in cc.EN_UNSATURATED:
        assert -31 < ref.min() < 0 < ref.max() < 31, (ref.min(), ref.max())
    else:
        assert ref.max() == 31 and ref.min() == -31, (ref.min(), ref.max())


@pytest.mark.parametrize("method", cc.METHODS)
def test_mixed_and_clean_meet_their_conditions(abi, lib, code50, method):
    for window in cc.windows_of(method):
        (mixed, mst), (clean, cst) = cc.references(abi, lib, code50, [(method, "mixed", window), (method, "clean", window)])
        wrong = cc.wrong_frames(code50, mixed)
        print(method, window, "mixed", mst.tolist(), int(wrong.sum()), "frames wrong; clean", cst.tolist())
        assert wrong.any() and not wrong.all(), int(wrong.sum())
        assert not cc.wrong_frames(code50, clean).any()
        if method not in cc.EARLY_STOP_METHODS:
            assert (mst == [cc.MAX_ITER, 0]).all() and (cst == [cc.MAX_ITER, 0]).all()
            continue
        assert (mst[:, 0] < cc.MAX_ITER).any() and (mst[:, 0] == cc.MAX_ITER).any(), mst.tolist()
        if method in cc.BF_METHODS:
            assert (mst[:, 1] > 0).any(), mst.tolist()
        assert (cst[:, 0] < cc.MAX_ITER).all() and len(set(cst[:, 0].tolist())) > 1 and not cst[:, 1].any(), cst.tolist()
    if method in cc.EARLY_STOP_METHODS:
        _, mst = cc.reference(abi, lib, code50, method, "mixed")
        _, own = cc.codeword_reference(abi, lib, code50, method, "mixed")
        group = np.repeat(mst[:, 0], 32)
        assert ((own[:, 0] >= 1) & (own[:, 0] < group)).any()


@pytest.mark.parametrize("method", cc.EARLY_STOP_METHODS)
def test_staggered_spreads_the_own_iterations(abi, lib, code50, method):
    _, own = cc.codeword_reference(abi, lib, code50, method, "staggered")
    _, gst = cc.reference(abi, lib, code50, method, "staggered")
    values = [sorted(set(own[g * 32:(g + 1) * 32, 0].tolist())) for g in range(cc.NG)]
    print(method, "groups", gst.tolist(), "own iterations per group", values)
    assert max(len(v) for v in values) >= 4, values


def test_the_case_table_names_every_selection():
    for method in cc.METHODS:
        for window in cc.windows_of(method):
            states = {s: cc.selection_state(method, window, s) for s in cc.SELECTIONS}
            assert states["default"] == states["rotating"] == states["hbm"] == states["rows2"] == "run"
            assert (states["edge_off"] == "absent") == (window == "preset" and method in cc.WINDOW_METHODS)
            assert [s for s, v in states.items() if v == "refused"] == [s for s in cc.SELECTIONS if s in cc.REFUSED.get(method, ())]
    assert set(cc.KERNEL_OF) == set(cc.SELECTIONS)
