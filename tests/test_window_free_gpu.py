"""The window-free layer-static kernel on the GPU (lnsfaid_kernel4w.hip) against the layer-static kernel it stands in
for (lnsfaid_kernel4s.hip, forced with ZERO_SHIFT_WINDOWED on the same context): hard decisions and per-group iteration counts byte
for byte, for every number of layered iterations at which the choice of the iteration's form changes (1: the only iteration is the
first; 2: no iteration but the first has a predecessor that was the first; 3, 10: first and later ones), with and without the
bit-flipping stage, at 3.0 dB (nothing converges: every iteration runs) and at 3.6 dB (codewords park at decision points and resume
with their messages from HBM).  Which kernel a context selects; DecodeMethods 1 and 5 with the window configured away."""
import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

GROUPS = {3.0: 2, 3.6: 8}


@pytest.fixture(scope="module")
def frames(code50):
    """the restated reference channel's frames, drawn once: Eb/N0 -> int8 fixInput"""
    return {eb: oa.ReferenceChannel(code50, 1901, 13.0).groups(eb, ng) for eb, ng in GROUPS.items()}


def _both(abi, code50, cfg, fix, ng, want_window_free=True):
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    assert dec.static_layers() and dec.window_free() == want_window_free
    new = dec.decode(fix, ng)
    dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED)
    assert dec.static_layers() and not dec.window_free()
    old = dec.decode(fix, ng)
    dec.select_zero_shift(0)
    assert dec.window_free() == want_window_free
    return dec, new, old


@pytest.mark.parametrize("max_bf", [0, 10])
@pytest.mark.parametrize("max_iter", [1, 2, 3, 10])
@pytest.mark.parametrize("eb_n0", [3.0, 3.6])
def test_equals_the_layer_static_kernel(abi, code50, frames, eb_n0, max_iter, max_bf):
    ng = GROUPS[eb_n0]
    fix = frames[eb_n0]
    cfg = abi.default_cfg(2, max_iter)
    cfg.max_bf_iter = max_bf
    assert cfg.floor_iter_thresh < 0 and cfg.max_iteration == max_iter
    dec, new, old = _both(abi, code50, cfg, fix, ng)
    print("%.1f dB, %d + %d iterations, %d groups: iterations / bit-flipping iterations %s" % (eb_n0, max_iter, max_bf, ng, new[1].tolist()))
    if max_iter == 10:
        if eb_n0 == 3.0:
            assert (new[1][:, 0] == max_iter).all(), new[1].tolist()  # nothing converges: every layered iteration ran
        else:
            # precondition of the mixed batch: a codeword that is clean on its own before its group stops has parked at a decision
            # point and run on, from its stored messages, when its group mates passed that point
            _, own = dec.decode_codewords(fix, ng)
            group_its = np.repeat(new[1][:, 0], 32)
            resumed = int(((own[:, 0] < group_its) & (own[:, 0] >= 1)).sum())
            print("codewords clean before their group stopped, after at least one iteration: %d of %d" % (resumed, ng * 32))
            if resumed == 0:
                pytest.fail("precondition: no codeword of this batch parks and resumes - the batch does not test the resume path")
    dec.close()
    assert np.array_equal(new[0], old[0]), np.nonzero((new[0] != old[0]).reshape(ng * 32, code50.N).any(axis=1))[0][:8].tolist()
    assert np.array_equal(new[1], old[1]), (new[1].tolist(), old[1].tolist())


def test_equals_the_oracle(abi, code50, frames):
    ng = GROUPS[3.0]
    cfg = abi.default_cfg(2, 10)
    ref, ref_stats = oa.Oracle(code50, cfg).decode(frames[3.0], ng)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    assert dec.window_free()
    out, stats = dec.decode(frames[3.0], ng)
    dec.close()
    assert np.array_equal(out, ref) and np.array_equal(stats, ref_stats), (stats.tolist(), ref_stats.tolist())


@pytest.mark.parametrize("method", [1, 5])
def test_other_methods_without_a_window(abi, code50, frames, method):
    """the min-sum rows (their selective offset as the one table) and the 2B1C rows, with the window configured away"""
    ng = GROUPS[3.6]
    cfg = abi.default_cfg(method, 10)
    assert cfg.floor_iter_thresh >= 0
    cfg.floor_iter_thresh = -1
    dec, new, old = _both(abi, code50, cfg, frames[3.6], ng)
    dec.close()
    print("method %d: iterations / bit-flipping iterations %s" % (method, new[1].tolist()))
    assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]), (new[1].tolist(), old[1].tolist())


def test_selection(abi, code50):
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.window_free() and dec.static_layers() and dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED)
    assert not dec.window_free() and dec.static_layers() and dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_STATIC)
    assert dec.window_free()
    for mode in (abi.ZERO_SHIFT_LOOP, abi.ZERO_SHIFT_OFF):
        dec.select_zero_shift(mode)
        assert not dec.window_free() and not dec.static_layers()
    dec.select_zero_shift(0)
    dec.select_message_store(abi.MSG_HBM)  # outside the layer-static kernel's configurations
    assert not dec.window_free()
    with pytest.raises(RuntimeError):
        dec.select_zero_shift(abi.ZERO_SHIFT_WINDOWED)
    dec.close()
    # a window that can open keeps the layer-static kernel
    for thresh in (0, 6):
        cfg = abi.default_cfg(2, 10)
        cfg.floor_iter_thresh = thresh
        dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
        assert dec.static_layers() and not dec.window_free(), thresh
        dec.close()
    for method in (1, 3, 4, 5):
        cfg = abi.default_cfg(method, 10)
        dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
        assert dec.static_layers() and not dec.window_free(), method  # their presets have a window
        dec.close()
        cfg.floor_iter_thresh = -1
        dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
        assert dec.window_free() and dec.kernel_residency() == (8, 8), method
        dec.close()
