"""The layer-static decode kernel on the GPU (lnsfaid_kernel4s.hip): hard decisions, group records and error
counters against the scalar oracle byte for byte, and against the same context switched to the rotation-free kernel's layer loop
and to the rotating kernel; which kernel a context selects; a code that is not the built-in one never gets the static kernel."""
import ctypes as C

import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

ZG_50GPON = [0, 5, 0, 0, 1, 0, 0, 2, 4, 1, 0, 1]


@pytest.fixture(scope="module")
def llrs(code50):
    """the synthetic generator's frames, drawn once: (Eb/N0, groups) -> int8 fixInput"""
    return {(eb, ng): oa.synth_llr(ng, code50.N, eb, seed=900 + ng) for eb in (3.55, 3.0) for ng in (1, 3)}


def _decode(dec, fix, ng):
    out, stats = dec.decode(fix, ng)
    return out, stats, dec.count_errors(out, None, ng)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("method", [2, 1, 5])
@pytest.mark.parametrize("eb_n0", [3.55, 3.0])
@pytest.mark.parametrize("ng", [1, 3])
def test_equals_the_oracle_the_layer_loop_and_the_rotating_kernel(abi, code50, llrs, ng, eb_n0, method):
    """3.55 dB is in the waterfall: the codewords of a group stop at different iterations, so records of parked codewords go
    through HBM and come back; at 3.0 dB every codeword runs to the end of both stages."""
    fix = llrs[(eb_n0, ng)]
    cfg = abi.default_cfg(method, 10)
    oracle = oa.Oracle(code50, cfg)
    ref, ref_stats = oracle.decode(fix, ng)
    ref_counters = oracle.count_errors(ref, None, ng)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    assert dec.static_layers() and dec.zero_shift_groups(12) == (True, ZG_50GPON)
    new = _decode(dec, fix, ng)
    dec.select_zero_shift(abi.ZERO_SHIFT_LOOP)
    assert not dec.static_layers() and dec.zero_shift_groups(12) == (True, ZG_50GPON)
    loop = _decode(dec, fix, ng)
    dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
    assert not dec.static_layers() and dec.zero_shift_groups(12) == (False, [0] * 12)
    rotating = _decode(dec, fix, ng)
    dec.close()
    print("method %d, %.2f dB, %d groups: iterations / bit-flipping iterations %s" % (method, eb_n0, ng, ref_stats.tolist()))
    assert np.array_equal(new[0], ref), np.nonzero((new[0] != ref).reshape(ng * 32, code50.N).any(axis=1))[0][:8].tolist()
    assert np.array_equal(new[1], ref_stats), (new[1].tolist(), ref_stats.tolist())
    assert new[2] == ref_counters
    assert _same(new, loop) and _same(new, rotating)


def test_selection(abi, lib, code50):
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.static_layers() and dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_LOOP)
    assert not dec.static_layers() and dec.zero_shift_groups(12)[0] and dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_STATIC)
    assert dec.static_layers()
    dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
    assert not dec.static_layers()
    dec.select_zero_shift(abi.ZERO_SHIFT_ON)
    assert dec.static_layers()
    # outside the rotation-free kernel's configurations there is no static kernel either
    dec.select_zero_shift(0)
    dec.select_message_store(abi.MSG_HBM)
    assert not dec.static_layers()
    with pytest.raises(RuntimeError):
        dec.select_zero_shift(abi.ZERO_SHIFT_STATIC)
    dec.close()
    for method in (1, 3, 4, 5):
        dec = abi.Decoder(code50, abi.default_cfg(method, 10), device=0, max_groups=1)
        assert dec.static_layers() and dec.kernel_residency() == (8, 8), method
        dec.close()
    dec = abi.Decoder(code50, abi.default_cfg(0, 10), device=0, max_groups=1)
    assert not dec.static_layers()
    dec.close()


def _one_shift_moved(abi, lib):
    """the 50G-PON table with the first circulant of layer 2 shifted by one more row: same layers, degrees and block columns"""
    base = abi.Code50GPON(lib)
    pos = np.ctypeslib.as_array(base.pos_vn).copy()
    e = 256 * 23 + 256 * 22  # first entry of layer 2
    first = pos[e:e + 256 * 23:23]
    pos[e:e + 256 * 23:23] = (first // 256) * 256 + (first % 256 + 1) % 256
    base.pos_vn = (C.c_uint16 * pos.size)(*pos.tolist())
    base.code.pos_vn = base.pos_vn
    return base


def test_another_code_stays_on_the_layer_loop(abi, lib, code50):
    other = _one_shift_moved(abi, lib)
    cfg = abi.default_cfg(2, 10)
    fix = oa.synth_llr(1, other.N, 3.55, seed=77)
    oracle = oa.Oracle(other, cfg)
    ref, ref_stats = oracle.decode(fix, 1)
    dec = abi.Decoder(other, cfg, device=0, max_groups=1)
    assert not dec.static_layers() and dec.zero_shift_groups(12) == (True, ZG_50GPON)
    with pytest.raises(RuntimeError):
        dec.select_zero_shift(abi.ZERO_SHIFT_STATIC)
    out, stats = dec.decode(fix, 1)
    counters = dec.count_errors(out, None, 1)
    dec.close()
    assert np.array_equal(out, ref) and np.array_equal(stats, ref_stats) and counters == oracle.count_errors(ref, None, 1)
    # and the built-in code next to it still gets the static kernel
    dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
    assert dec.static_layers()
    dec.close()
