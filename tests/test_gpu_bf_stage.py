"""The bit-flipping stage of the one-wave kernels with its constants taken out of the iterations (the walk of the
weight-3 columns on top of a fixed share, finished flip addresses, one threshold choice per iteration), through the C ABI against
the scalar oracle: hard decisions, the groups' (iterations, bit-flipping iterations) and the four error counters, on 32 and on 96
codewords (one and three groups).

Cases: DecodeMethod 2 at 3.0 dB with MaxIteration 10 (every group runs all ten iterations of the stage); DecodeMethod 2 with
MaxIteration 3 on a batch with a group that never enters the stage, one that stops clean inside it and one that runs all of it;
DecodeMethods 4 and 5 (5 on 16-QAM: hard2 and the big jump), alpha 0 and 1, DecodeMethod 3 (plain flipping: the full walk kept).
In the group that stops inside the stage most codewords are clean before their group is: they park inside the stage and are
resumed by the next launch (asserted on the per-codeword restatement of the oracle); the same 32 codewords run under the per-codeword
rule (lnsfaid_kernel4cw.hip).  The first two cases again in child processes on the other kernels that compile the shared header.

The three kinds of group do not occur at one Eb/N0: at 4.2 dB (seed 211, 48 groups, MaxIteration 3) 37 groups run all ten
iterations of the stage, 11 stop inside it and none stays out of it, which takes all 32 codewords clean after two iterations
(5.6 dB and above).  The batch therefore takes groups 0 and 4 of the 4.2 dB draw and group 0 of the 5.6 dB draw of the same seed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_abi as oa
from early_stop_ref import per_codeword_oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_CASES = ["m2_3dB", "m2_spread"]


def _cfg(abi, method, max_iter, alpha=None):
    cfg = abi.default_cfg(method, max_iter)
    if alpha is not None:
        cfg.bf_alpha = alpha
    return cfg


def _spread_batch(code50):
    per = 32 * code50.N
    low = oa.ReferenceChannel(code50, 211, 13.0).groups(4.2, 5).reshape(5, per)
    high = oa.ReferenceChannel(code50, 211, 13.0).groups(5.6, 1).reshape(1, per)
    return np.ascontiguousarray(np.stack([low[4], low[0], high[0]]).reshape(-1))  # stops inside / runs all / never enters


@pytest.fixture(scope="module")
def cases(abi, code50):
    """name -> (method, MaxIteration, alpha or None, fixInput of three groups, oracle bits, records, counters), computed once"""
    qpsk = oa.ReferenceChannel(code50, 311, 13.0).groups(3.0, 3)
    qpsk35 = oa.ReferenceChannel(code50, 311, 13.0).groups(3.5, 3)
    qam16 = oa.ReferenceChannel(code50, 311, 12.5, mod_type=4).groups(5.6, 3)
    spread = _spread_batch(code50)
    todo = {"m2_3dB": (2, 10, None, qpsk), "m2_spread": (2, 3, None, spread), "m2_alpha0": (2, 10, 0, qpsk),
            "m2_spread_alpha0": (2, 3, 0, spread), "m4": (4, 10, None, qpsk35), "m5_16qam": (5, 10, None, qam16),
            "m5_16qam_alpha0": (5, 10, 0, qam16), "m5_spread": (5, 3, None, spread), "m3": (3, 10, None, qpsk35)}
    res = {}
    for name, (method, max_iter, alpha, fix) in todo.items():
        cfg = _cfg(abi, method, max_iter, alpha)
        ref, stats = oa.decode_mt(code50, cfg, fix, 3)
        oracle = oa.Oracle(code50, cfg)
        counters = [oracle.count_errors(np.ascontiguousarray(ref[:n * 32 * code50.N]), None, n) for n in (1, 3)]
        oracle.close()
        res[name] = (method, max_iter, alpha, fix, ref, stats, counters)
    return res


def test_the_cases_are_what_they_say(abi, code50, cases):
    for name, c in cases.items():
        print(name, "alpha", _cfg(abi, c[0], c[1], c[2]).bf_alpha, "records", c[5].tolist())
    max_bf = abi.default_cfg(2, 10).max_bf_iter
    assert cases["m2_3dB"][5].tolist() == [[10, max_bf]] * 3 and cases["m2_alpha0"][5].tolist() == [[10, max_bf]] * 3
    assert abi.default_cfg(2, 10).bf_alpha == 1
    stats = cases["m2_spread"][5]
    assert stats[0][0] == 3 and 0 < stats[0][1] < max_bf  # stops clean inside the stage
    assert stats[1].tolist() == [3, max_bf]               # runs all of it
    assert stats[2][0] < 3 and stats[2][1] == 0           # never enters it
    for name in ("m4", "m5_16qam", "m5_16qam_alpha0", "m5_spread", "m3"):
        assert cases[name][5][:, 1].max() > 0, name       # the stage is exercised
    assert cases["m5_16qam"][5][0][1] > 0                 # also by the 32-codeword run
    # relaunches: codewords of the first group are clean inside the stage before their group is (they park there and resume)
    _, per_cw = per_codeword_oracle(code50, abi.default_cfg(2, 3), cases["m2_spread"][3][:32 * code50.N], 1)
    inside = (per_cw[:, 0] == 3) & (per_cw[:, 1] > 0) & (per_cw[:, 1] < stats[0][1])
    print("codewords that park inside the stage before their group stops:", int(inside.sum()), "first decision point", int((per_cw[:, 1] == 0).sum()))
    assert inside.sum() >= 4


@pytest.mark.parametrize("name", ["m2_3dB", "m2_spread", "m2_alpha0", "m2_spread_alpha0", "m4", "m5_16qam", "m5_16qam_alpha0", "m5_spread", "m3"])
@pytest.mark.parametrize("n_groups", [1, 3])
def test_stage_equals_the_oracle(abi, code50, cases, name, n_groups):
    method, max_iter, alpha, fix, ref, ref_stats, ref_counters = cases[name]
    n = n_groups * 32 * code50.N
    dec = abi.Decoder(code50, _cfg(abi, method, max_iter, alpha), device=0, max_groups=n_groups)
    out, stats = dec.decode(np.ascontiguousarray(fix[:n]), n_groups)
    counters = dec.count_errors(out, None, n_groups)
    dec.close()
    print("%s, %d codewords: records %s, oracle %s, counters %s" % (name, 32 * n_groups, stats.tolist(), ref_stats[:n_groups].tolist(), counters))
    assert np.array_equal(stats, ref_stats[:n_groups]), (stats.tolist(), ref_stats.tolist())
    assert np.array_equal(out, ref[:n]), np.nonzero((out != ref[:n]).reshape(-1, code50.N).any(axis=1))[0][:8].tolist()
    assert counters == ref_counters[0 if n_groups == 1 else 1]


@pytest.mark.parametrize("method", [2, 5])
def test_per_codeword_rule_stops_inside_the_stage(abi, code50, cases, method):
    """lnsfaid_kernel4cw.hip on the 32 codewords of the group that stops inside the stage: every codeword as the oracle decodes 32
    copies of it"""
    cfg = abi.default_cfg(method, 3)
    fix = np.ascontiguousarray(cases["m2_spread"][3][:32 * code50.N])
    ref, ref_stats = per_codeword_oracle(code50, cfg, fix, 1)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
    out, cw = dec.decode_codewords(fix, 1)
    dec.close()
    assert ((ref_stats[:, 1] > 0) & (ref_stats[:, 1] < cfg.max_bf_iter)).sum() >= 4
    assert np.array_equal(cw[:, :2], ref_stats), np.nonzero((cw[:, :2] != ref_stats).any(axis=1))[0][:8].tolist()
    assert np.array_equal(out.reshape(32, code50.N), ref)


def test_other_kernels_in_child_processes(cases, tmp_path):
    """the first two cases on the rotation-free kernel's layer loop (lnsfaid_kernel4z.hip), the rotating kernel (lnsfaid_kernel4.hip),
    two waves per codeword (lnsfaid_kernel5.hip, which keeps the walk of all columns) and the messages streamed through HBM.  One
    child after the other, each under its own time limit; the first failure ends the chain."""
    src = tmp_path / "in.npz"
    np.savez(src, **{"fix_" + name: cases[name][3] for name in CHILD_CASES}, **{"iter_" + name: np.array(cases[name][1]) for name in CHILD_CASES})
    for tag, env, waves in (("loop", {"LNSFAID_ZERO_SHIFT": "loop"}, 1), ("off", {"LNSFAID_ZERO_SHIFT": "off"}, 1),
                            ("waves2", {"LNSFAID_WAVES_PER_CODEWORD": "2"}, 2), ("hbm", {"LNSFAID_MSG_STORE": "hbm"}, 1)):
        dst = tmp_path / ("out_%s.npz" % tag)
        r = subprocess.run([sys.executable, os.path.join(HERE, "bf_stage_worker.py"), str(src), str(dst)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (tag, r.stdout[-1000:] + r.stderr[-2000:])
        got = np.load(dst)
        assert int(got["waves"]) == waves, (tag, got["waves"])
        if tag == "loop":
            assert bool(got["zero_shift"]) and not bool(got["static"])
        if tag == "off":
            assert not bool(got["zero_shift"]) and not bool(got["static"])
        if tag == "hbm":
            assert int(got["msg_store"]) == oa.pyabi.MSG_HBM
        for name in CHILD_CASES:
            _, _, _, _, ref, ref_stats, ref_counters = cases[name]
            assert np.array_equal(got["stats_" + name], ref_stats), (tag, name, got["stats_" + name].tolist(), ref_stats.tolist())
            assert np.array_equal(got["out_" + name], ref), (tag, name)
            assert got["counters_" + name].tolist() == ref_counters[1], (tag, name)
