"""The layer step with its byte masks expanded in pairs (sw_mask7x2 / sw_zero_mask2) on the GPU, against the oracle
port byte for byte: hard decisions and the groups' iteration counts of two groups (64 codewords) of the built-in code at 3.0 dB
(every codeword runs both stages to the end) and at 4.2 dB (all stop early).  The code has layers of degree 23 and of degree 22, so
groups of edges with an odd last edge and without.  DecodeMethods 0 (one factor), 1, 2 and 5 on the default kernel; DecodeMethod 2
also on the rotating kernel and on the rotation-free kernel's layer loop (environment switches: fresh child processes), with the
messages streamed through HBM (the generic instance of the layer step next to the per-degree ones), through the packed entry point
and through the per-codeword entry point (there against the 32-copy restatement through the port)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_abi as oa
from early_stop_ref import per_codeword_oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NG = 2
EB = [3.0, 4.2]


def _cfg(abi, method):
    cfg = abi.default_cfg(method, 10)
    if method == 0:
        cfg.factor_1 = cfg.factor_2 = 24  # one normalisation factor: the four-rows kernel
    return cfg


@pytest.fixture(scope="module")
def frames(code50):
    """Eb/N0 -> int8 fixInput of two groups, drawn once"""
    return {eb: oa.ReferenceChannel(code50, 318, 13.0).groups(eb, NG) for eb in EB}


@pytest.fixture(scope="module")
def port(abi, code50, frames):
    """(method, Eb/N0) -> (decodedBits, [NG, 2] iterations) of the oracle port, each computed once and left unchanged"""
    cache = {}

    def get(method, eb):
        if (method, eb) not in cache:
            oracle = oa.Oracle(code50, _cfg(abi, method))
            ref, stats = oracle.decode(frames[eb], NG)
            oracle.close()
            ref.setflags(write=False)
            stats.setflags(write=False)
            cache[(method, eb)] = (ref, stats)
        return cache[(method, eb)]
    return get


def _equal(code50, out, stats, want):
    ref, ref_stats = want
    assert np.array_equal(stats, ref_stats), (np.asarray(stats).tolist(), ref_stats.tolist())
    assert np.array_equal(out, ref), np.nonzero((out != ref).reshape(NG * 32, code50.N).any(axis=1))[0][:8].tolist()


@pytest.mark.parametrize("eb", EB)
@pytest.mark.parametrize("method", [0, 1, 2, 5])
def test_methods(abi, code50, frames, port, method, eb):
    dec = abi.Decoder(code50, _cfg(abi, method), device=0, max_groups=NG)
    assert dec.rows_per_lane() == 4 and dec.static_layers() == (method != 0)
    out, stats = dec.decode(frames[eb], NG)
    dec.close()
    print("method %d, %.1f dB: iterations / bit-flipping iterations %s" % (method, eb, stats.tolist()))
    _equal(code50, out, stats, port(method, eb))
    if method == 2:
        assert (stats[:, 0] == 10).all() if eb == 3.0 else (stats[:, 0] < 10).all(), stats.tolist()


@pytest.mark.parametrize("switch,zero_shift", [("off", False), ("loop", True)])
def test_method_2_on_the_other_kernels(tmp_path, code50, frames, port, switch, zero_shift):
    """LNSFAID_ZERO_SHIFT=off: the rotating kernel (lnsfaid_kernel4.hip); loop: the layer loop of lnsfaid_kernel4z.hip.  The
    switch is read when a context is made: a fresh process per value (tests/dirty_check_worker.py decodes what it is given)."""
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, **{"fix_%d" % i: frames[eb] for i, eb in enumerate(EB)})
    r = subprocess.run([sys.executable, os.path.join(HERE, "dirty_check_worker.py"), str(src), str(dst), "group"],
                       env=dict(os.environ, LNSFAID_ZERO_SHIFT=switch), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    got = np.load(dst)
    assert not bool(got["static"]) and bool(got["zero_shift"]) == zero_shift and int(got["waves"]) == 1
    for i, eb in enumerate(EB):
        _equal(code50, got["out_%d" % i], got["stats_%d" % i], port(2, eb))


@pytest.mark.parametrize("eb", EB)
def test_method_2_messages_through_hbm(abi, code50, frames, port, eb):
    dec = abi.Decoder(code50, _cfg(abi, 2), device=0, max_groups=NG)
    dec.select_message_store(abi.MSG_HBM)
    assert dec.message_store() == abi.MSG_HBM and not dec.static_layers()
    out, stats = dec.decode(frames[eb], NG)
    dec.close()
    _equal(code50, out, stats, port(2, eb))


@pytest.mark.parametrize("eb", EB)
def test_method_2_packed_entry_point(abi, code50, frames, port, eb):
    llr4 = abi.pack_llr4(frames[eb])
    dec = abi.Decoder(code50, _cfg(abi, 2), device=0, max_groups=NG)
    bits, stats = dec.decode_packed(llr4, NG)
    dec.close()
    _equal(code50, abi.unpack_bits(bits), stats, port(2, eb))


@pytest.mark.parametrize("eb", EB)
def test_method_2_per_codeword_entry_point(abi, code50, frames, eb):
    cfg = _cfg(abi, 2)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=NG)
    out, cw = dec.decode_codewords(frames[eb], NG)
    dec.close()
    ref, ref_stats = per_codeword_oracle(code50, cfg, frames[eb], NG, kind="oracle")
    assert np.array_equal(cw[:, :2], ref_stats), np.nonzero((cw[:, :2] != ref_stats).any(axis=1))[0][:8].tolist()
    assert np.array_equal(out.reshape(NG * 32, code50.N), ref)
