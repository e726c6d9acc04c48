"""The decision points' cheap "certainly dirty" test on the GPU, through the C ABI with DecodeMethod 2: the test only
decides whether the exact syndrome is skipped for a codeword that is dirty anyway, so decoded bits, the groups' (iterations,
bit-flipping iterations) and the error counters must equal the scalar oracle's whatever it reports - a false "dirty" lets a clean
group run on (iterations >= 1 where the oracle stops at 0), a false "clean" only costs time.  Batches of two groups (64 codewords)
built from valid codewords at LLR +-7 whose punctured tail is zero, so that a noiseless group is clean at the first decision
point: noiseless; one lane with one wrong-sign node in a block column of the layer stage 1 asks (layer 1: column 1), of the layer
only stage 2 asks (layer 0: column 0), of neither (column 2: the full syndrome has to find it); one lane with LLRs 0; 3.6 dB noise,
where lanes park and resume.  Default kernel selection: the layer-static kernel, the test on compile-time tables.  The first four
again in fresh child processes on the kernels that take the test on run-time tables (sw_row_parity): the layer loop
(lnsfaid_kernel4z.hip, LNSFAID_ZERO_SHIFT=loop) and two waves per codeword (lnsfaid_kernel5.hip, LNSFAID_WAVES_PER_CODEWORD=2)
against the same oracle, and the per-codeword stop rule (lnsfaid_kernel4cw.hip) against the oracle's 32-copy restatement of that
rule; and with LNSFAID_ZERO_SHIFT=off on the rotating kernel (lnsfaid_kernel4.hip), which keeps the old text of the test
(layer0_dirty4_edgewise).  lnsfaid_kernel4p.hip (packed I/O) compiles sw_row_parity too and has NO case here: its decisions are
checked against the oracle only by the packed-I/O suite that was there before (test_gpu_packed_io.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gf2_encoder
import oracle_abi as oa
from early_stop_ref import per_codeword_oracle

pytestmark = pytest.mark.gpu

TAIL = 384  # punctured variable nodes at the end of the codeword: erased at the input
LANE = 5    # the lane of group 0 that carries the disturbance
GENERIC = ["noiseless", "stage1_column", "stage2_column", "neither_column"]


def _zero_tail_codewords(encoder, N, K, n):
    """n different non-zero codewords whose last TAIL bits are 0: combinations of random codewords from the null space (over GF(2))
    of their tails"""
    rng = np.random.default_rng(20261)
    cws = encoder.encode(rng.integers(0, 2, size=(TAIL + n, K), dtype=np.uint8)).astype(np.uint8)
    a = cws[:, N - TAIL:].copy()
    b = np.eye(TAIL + n, dtype=np.uint8)
    rank = 0
    for col in range(TAIL):
        piv = np.nonzero(a[rank:, col])[0]
        if piv.size == 0:
            continue
        p = rank + int(piv[0])
        a[[rank, p]] = a[[p, rank]]
        b[[rank, p]] = b[[p, rank]]
        rows = rank + 1 + np.nonzero(a[rank + 1:, col])[0]
        a[rows] ^= a[rank]
        b[rows] ^= b[rank]
        rank += 1
    assert not a[rank:].any() and TAIL + n - rank >= n
    out = (b[rank:rank + n].astype(np.float32) @ cws.astype(np.float32)).astype(np.int64) & 1
    assert not out[:, N - TAIL:].any() and out.any(axis=1).all()
    return out.astype(np.int8)


@pytest.fixture(scope="module")
def batches(abi, code50, encoder):
    """name -> (fixInput of two groups, oracle bits, oracle records, oracle counters), computed once"""
    N, K = code50.N, code50.K
    words = _zero_tail_codewords(encoder, N, K, 8)
    frames = words[np.arange(64) % 8]  # [64, N]
    llr = np.where(frames > 0, 7, -7).astype(np.int8)

    def flipped(node):
        x = llr.copy()
        x[LANE, node] = -x[LANE, node]
        return x

    zeros = llr.copy()
    zeros[LANE, np.random.default_rng(7).choice(K, size=300, replace=False)] = 0
    cases = {"noiseless": llr, "stage1_column": flipped(1 * 256 + 77), "stage2_column": flipped(0 * 256 + 200),
             "neither_column": flipped(2 * 256 + 13), "zero_llrs": zeros}
    fix = {name: gf2_encoder.to_group_layout(x, K) for name, x in cases.items()}
    fix["noise_3p6dB"] = gf2_encoder.qpsk_llr(frames, 3.6, seed=36)
    oracle = oa.Oracle(code50, abi.default_cfg(2, 10))
    res = {}
    for name, f in fix.items():
        ref, stats = oracle.decode(f, 2)
        res[name] = (f, ref, stats, oracle.count_errors(ref, None, 2))
    oracle.close()
    return res


def test_the_cases_are_what_they_say(abi, batches, code50):
    """noiseless groups are clean at the first decision point (no iteration); a single wrong-sign node is repaired by the first
    iteration; the columns are columns of layer 1 only / layer 0 only / neither (csrc/lnsfaid_gpon_base.h)"""
    assert batches["noiseless"][2].tolist() == [[0, 0], [0, 0]]
    for name in ("stage1_column", "stage2_column", "neither_column"):
        stats = batches[name][2].tolist()
        print(name, stats)
        assert stats[0][0] >= 1 and stats[1] == [0, 0], (name, stats)
    pos = np.ctypeslib.as_array(code50.pos_vn).astype(np.int64)
    cols = [set((pos[e:e + d] // 256).tolist()) for e, d in ((0, 23), (256 * 23, 22))]  # layers 0 and 1: their first rows
    assert 1 in cols[1] and 1 not in cols[0] and 0 in cols[0] and 0 not in cols[1] and 2 not in cols[0] | cols[1]
    # 3.6 dB: some lane of a group is clean at a decision point its group passes (it parks there and resumes): under the
    # per-codeword rule it stops earlier than its group does
    fix, _, stats, _ = batches["noise_3p6dB"]
    _, per_cw = per_codeword_oracle(code50, abi.default_cfg(2, 10), fix, 2)
    early = [int((per_cw[32 * g:32 * g + 32, 0] < stats[g][0]).sum()) for g in range(2)]
    print("3.6 dB: groups %s, lanes clean before their group's end %s" % (stats.tolist(), early))
    assert sum(early) >= 1, (stats.tolist(), per_cw[:, 0].tolist())


@pytest.mark.parametrize("name", GENERIC + ["zero_llrs", "noise_3p6dB"])
def test_static_kernel_equals_the_oracle(abi, code50, batches, name):
    fix, ref, ref_stats, ref_counters = batches[name]
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=2)
    assert dec.static_layers() and dec.zero_shift_groups(12)[0]  # default selection: lnsfaid_zero_shift_groups reports the static kernel
    out, stats = dec.decode(fix, 2)
    counters = dec.count_errors(out, None, 2)
    dec.close()
    print("%s: iterations / bit-flipping iterations %s, oracle %s" % (name, stats.tolist(), ref_stats.tolist()))
    assert np.array_equal(stats, ref_stats), (stats.tolist(), ref_stats.tolist())
    assert np.array_equal(out, ref), np.nonzero((out != ref).reshape(64, code50.N).any(axis=1))[0][:8].tolist()
    assert counters == ref_counters


def _child(tmp_path, batches, env, rule):
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, **{"fix_" + name: batches[name][0] for name in GENERIC})
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dirty_check_worker.py"), str(src), str(dst), rule],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    return np.load(dst)


def _group_rule_equals_the_oracle(got, batches):
    for name in GENERIC:
        _, ref, ref_stats, ref_counters = batches[name]
        assert np.array_equal(got["stats_" + name], ref_stats), (name, got["stats_" + name].tolist(), ref_stats.tolist())
        assert np.array_equal(got["out_" + name], ref), name
        assert got["counters_" + name].tolist() == ref_counters, name


@pytest.mark.parametrize("env,waves,zero_shift", [({"LNSFAID_ZERO_SHIFT": "loop"}, 1, True), ({"LNSFAID_WAVES_PER_CODEWORD": "2"}, 2, False)])
def test_run_time_tables_group_rule(batches, tmp_path, env, waves, zero_shift):
    """the layer loop of lnsfaid_kernel4z.hip and the two-wave kernel lnsfaid_kernel5.hip: layer0_dirty4 -> sw_row_parity on
    LfDevCode's tables, group rule, the same oracle"""
    got = _child(tmp_path, batches, env, "group")
    assert int(got["waves"]) == waves and not bool(got["static"]), (got["waves"], got["static"])
    if zero_shift:
        assert bool(got["zero_shift"])  # the rotation-free kernel's layer loop, not the rotating kernel
    _group_rule_equals_the_oracle(got, batches)


def test_run_time_tables_per_codeword_rule(abi, code50, batches, tmp_path):
    """lnsfaid_kernel4cw.hip: layer0_dirty4 -> sw_row_parity; every codeword stops on its own, so the reference is the oracle run on
    32 copies of each codeword.  The noiseless codewords stop at decision point 1 (0 iterations), the disturbed lane after one."""
    got = _child(tmp_path, batches, {}, "codeword")
    assert int(got["early_stop"]) == abi.STOP_CODEWORD and int(got["waves"]) == 1
    cfg = abi.default_cfg(2, 10)
    for name in GENERIC:
        ref, ref_stats = per_codeword_oracle(code50, cfg, batches[name][0], 2)
        out, stats = got["out_" + name].reshape(64, code50.N), got["stats_" + name]
        assert np.array_equal(stats[:, :2], ref_stats), (name, np.nonzero((stats[:, :2] != ref_stats).any(axis=1))[0][:8].tolist())
        assert np.array_equal(out, ref), name
        want = [[0, 0]] * 64
        if name != "noiseless":
            want[LANE] = [1, 0]
        assert ref_stats.tolist() == want, (name, ref_stats[LANE].tolist())


def test_old_text_kernel_equals_the_oracle(batches, tmp_path):
    """the rotating kernel of lnsfaid_kernel4.hip stays on layer0_dirty4_edgewise: unchanged device code, the cases
    run on it for the hook that selects that text"""
    got = _child(tmp_path, batches, {"LNSFAID_ZERO_SHIFT": "off"}, "group")
    assert not bool(got["static"]) and not bool(got["zero_shift"]) and int(got["waves"]) == 1, (got["static"], got["zero_shift"])
    _group_rule_equals_the_oracle(got, batches)
