"""The window-free kernel's edge-word twin on the GPU (lnsfaid_kernel4e.hip) against the kernel it stands in for
(lnsfaid_kernel4w.hip, selected on the same context with select_edge_words(False)): hard decisions and per-group iteration counts byte
for byte on the same inputs - at 3.0 dB, where nothing converges, with 1, 2 and 10 layered iterations (the first form alone, one
later iteration, many) with and without the bit-flipping stage; at 3.6 dB, where codewords park at decision points and resume;
DecodeMethods 1 and 5 with the window configured away.  Which kernel a context selects, by default, through the call and through
the environment; residency."""
import os

import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

GROUPS = {3.0: 2, 3.6: 8}


@pytest.fixture(scope="module")
def frames(code50):
    """the restated reference channel's frames, drawn once: Eb/N0 -> int8 fixInput"""
    return {eb: oa.ReferenceChannel(code50, 2601, 13.0).groups(eb, ng) for eb, ng in GROUPS.items()}


def _on_then_off(abi, code50, cfg, fix, ng):
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    assert dec.window_free() and dec.edge_words()
    new = dec.decode(fix, ng)
    dec.select_edge_words(False)
    assert dec.window_free() and not dec.edge_words()
    old = dec.decode(fix, ng)
    dec.select_edge_words(True)
    assert dec.edge_words()
    return dec, new, old


def _same(new, old, ng, n):
    assert np.array_equal(new[0], old[0]), np.nonzero((new[0] != old[0]).reshape(ng * 32, n).any(axis=1))[0][:8].tolist()
    assert np.array_equal(new[1], old[1]), (new[1].tolist(), old[1].tolist())


@pytest.mark.parametrize("max_bf", [0, 10])
@pytest.mark.parametrize("max_iter", [1, 2, 10])
def test_nothing_converges(abi, code50, frames, max_iter, max_bf):
    ng = GROUPS[3.0]
    cfg = abi.default_cfg(2, max_iter)
    cfg.max_bf_iter = max_bf
    assert cfg.floor_iter_thresh < 0 and cfg.max_iteration == max_iter
    dec, new, old = _on_then_off(abi, code50, cfg, frames[3.0], ng)
    dec.close()
    print("3.0 dB, %d + %d iterations: iterations / bit-flipping iterations %s" % (max_iter, max_bf, new[1].tolist()))
    assert (new[1][:, 0] == max_iter).all(), new[1].tolist()  # every layered iteration ran
    _same(new, old, ng, code50.N)


def test_codewords_park_and_resume(abi, code50, frames):
    ng = GROUPS[3.6]
    dec, new, old = _on_then_off(abi, code50, abi.default_cfg(2, 10), frames[3.6], ng)
    # the batch is mixed: a codeword that is clean on its own before its group stops has parked at a decision point and run on, from
    # its stored messages, when its group mates passed that point
    _, own = dec.decode_codewords(frames[3.6], ng)
    dec.close()
    group_its = np.repeat(new[1][:, 0], 32)
    resumed = int(((own[:, 0] < group_its) & (own[:, 0] >= 1)).sum())
    print("codewords clean before their group stopped, after at least one iteration: %d of %d" % (resumed, ng * 32))
    assert resumed > 0, "precondition: no codeword of this batch parks and resumes"
    _same(new, old, ng, code50.N)


def test_equals_the_oracle(abi, code50, frames):
    ng = GROUPS[3.0]
    cfg = abi.default_cfg(2, 10)
    ref, ref_stats = oa.Oracle(code50, cfg).decode(frames[3.0], ng)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    assert dec.edge_words()
    out, stats = dec.decode(frames[3.0], ng)
    dec.close()
    assert np.array_equal(out, ref) and np.array_equal(stats, ref_stats), (stats.tolist(), ref_stats.tolist())


@pytest.mark.parametrize("method", [1, 5])
def test_other_methods_without_a_window(abi, code50, frames, method):
    ng = 2
    fix = frames[3.6][:ng * 32 * code50.N]
    cfg = abi.default_cfg(method, 10)
    cfg.floor_iter_thresh = -1
    dec, new, old = _on_then_off(abi, code50, cfg, fix, ng)
    dec.close()
    print("method %d: iterations / bit-flipping iterations %s" % (method, new[1].tolist()))
    _same(new, old, ng, code50.N)


def test_selection_and_residency(abi, code50, monkeypatch):
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.window_free() and dec.edge_words() and dec.kernel_residency() == (8, 8)  # on by default
    dec.select_edge_words(False)
    assert dec.window_free() and not dec.edge_words() and dec.kernel_residency() == (8, 8)
    dec.select_edge_words(True)
    # never on where the window-free form is not selected
    for mode in (abi.ZERO_SHIFT_WINDOWED, abi.ZERO_SHIFT_LOOP, abi.ZERO_SHIFT_OFF):
        dec.select_zero_shift(mode)
        assert not dec.window_free() and not dec.edge_words(), mode
    dec.select_zero_shift(0)
    assert dec.edge_words()
    dec.select_message_store(abi.MSG_HBM)
    assert not dec.window_free() and not dec.edge_words()
    dec.close()
    cfg = abi.default_cfg(2, 10)
    cfg.floor_iter_thresh = 6  # a window that can open
    dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
    assert not dec.window_free() and not dec.edge_words()
    dec.close()
    for method in (1, 3, 4, 5):
        cfg = abi.default_cfg(method, 10)
        cfg.floor_iter_thresh = -1
        dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
        assert dec.window_free() and dec.edge_words() and dec.kernel_residency() == (8, 8), method
        dec.close()
    # the environment variable is read when a context is created
    monkeypatch.setenv("LNSFAID_EDGE_WORDS", "off")
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.window_free() and not dec.edge_words()
    dec.select_edge_words(True)  # the call overrides it
    assert dec.edge_words()
    dec.close()
    monkeypatch.delenv("LNSFAID_EDGE_WORDS")
    assert "LNSFAID_EDGE_WORDS" not in os.environ
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.edge_words()
    dec.close()
