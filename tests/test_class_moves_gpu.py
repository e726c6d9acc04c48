"""The window-free kernel written for the issue classes (SW_FORM_VK | SW_FORM_MUL) on the GPU against the layer-static
kernel, which runs the layer step's default text (lnsfaid_kernel4s.hip, forced with ZERO_SHIFT_WINDOWED on the same context): hard
decisions and group records byte for byte on 8 groups (256 codewords), max_iter 1, 2 and 10 with and without the bit-flipping stage,
at 3.0 dB (nothing converges: every iteration runs) and at 3.6 dB (codewords park at decision points and resume from their stored
messages); DecodeMethods 1 and 5 with the window configured away; the selection and the residency."""
import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

NG = 8


@pytest.fixture(scope="module")
def frames(code50):
    """the restated reference channel's frames, drawn once: Eb/N0 -> int8 fixInput"""
    return {eb: oa.ReferenceChannel(code50, 2301, 13.0).groups(eb, NG) for eb in (3.0, 3.6)}


def _both(abi, code50, cfg, fix):
    dec = abi.Decoder(code50, cfg, device=0, max_groups=NG)
    assert dec.static_layers() and dec.window_free()
    new = dec.decode(fix, NG)
    dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED)
    assert dec.static_layers() and not dec.window_free()
    old = dec.decode(fix, NG)
    dec.select_zero_shift(0)
    assert dec.window_free()
    return dec, new, old


@pytest.mark.parametrize("max_bf", [0, 10])
@pytest.mark.parametrize("max_iter", [1, 2, 10])
@pytest.mark.parametrize("eb_n0", [3.0, 3.6])
def test_equals_the_default_text(abi, code50, frames, eb_n0, max_iter, max_bf):
    fix = frames[eb_n0]
    cfg = abi.default_cfg(2, max_iter)
    cfg.max_bf_iter = max_bf
    assert cfg.floor_iter_thresh < 0 and cfg.max_iteration == max_iter
    dec, new, old = _both(abi, code50, cfg, fix)
    print("%.1f dB, %d + %d iterations: iterations / bit-flipping iterations %s" % (eb_n0, max_iter, max_bf, new[1].tolist()))
    if max_iter == 10 and eb_n0 == 3.6:
        # precondition of the mixed batch: codewords that are clean before their group stops have parked and resumed
        _, own = dec.decode_codewords(fix, NG)
        group_its = np.repeat(new[1][:, 0], 32)
        resumed = int(((own[:, 0] < group_its) & (own[:, 0] >= 1)).sum())
        print("codewords clean before their group stopped, after at least one iteration: %d of %d" % (resumed, NG * 32))
        if resumed == 0:
            pytest.fail("precondition: no codeword of this batch parks and resumes - the batch does not test the resume path")
    if max_iter == 10 and eb_n0 == 3.0:
        assert (new[1][:, 0] == max_iter).all(), new[1].tolist()
    dec.close()
    assert np.array_equal(new[0], old[0]), np.nonzero((new[0] != old[0]).reshape(NG * 32, code50.N).any(axis=1))[0][:8].tolist()
    assert np.array_equal(new[1], old[1]), (new[1].tolist(), old[1].tolist())


@pytest.mark.parametrize("method", [1, 5])
def test_other_methods_without_a_window(abi, code50, frames, method):
    cfg = abi.default_cfg(method, 10)
    cfg.floor_iter_thresh = -1
    dec, new, old = _both(abi, code50, cfg, frames[3.6])
    dec.close()
    print("method %d: iterations / bit-flipping iterations %s" % (method, new[1].tolist()))
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]), (new[1].tolist(), old[1].tolist())


def test_selection_and_residency(abi, code50):
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.window_free() and dec.static_layers()
    assert dec.kernel_residency() == (8, 8)
    dec.close()
