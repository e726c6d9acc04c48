"""The per-codeword early stop on the GPU (lnsfaid_set_early_stop, lnsfaid_decode_codewords*, lnsfaid_kernel4cw.hip): every
codeword decodes as the reference decodes a group of 32 copies of it (hard decisions, I and J), its record says how many checks
its output leaves unsatisfied, and nothing of the group rule changes."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle_abi as oa
from early_stop_ref import per_codeword_oracle, unsatisfied

pytestmark = pytest.mark.gpu

CODEWORD = 1


def _check(code, cfg, fix, ng, kind="avx2", store=0, dec=None):
    own = dec is None
    if own:
        dec = oa.pyabi.Decoder(code, cfg, 0, ng)
    if store:
        dec.select_message_store(store)
    out, cw = dec.decode_codewords(fix, ng)
    if own:
        dec.close()
    ref, rst = per_codeword_oracle(code, cfg, fix, ng, kind=kind)
    out = out.reshape(ng * 32, code.N)
    bad = np.nonzero((out != ref).any(axis=1))[0]
    assert bad.size == 0, ("decisions differ", bad[:8].tolist())
    assert np.array_equal(cw[:, :2], rst), np.nonzero((cw[:, :2] != rst).any(axis=1))[0][:8].tolist()
    assert np.array_equal(cw[:, 2], unsatisfied(code, out))
    return out, cw


@pytest.mark.parametrize("method", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("eb", [3.4, 3.5, 3.6])
def test_matches_the_32_copy_port(abi, code50, method, eb):
    cfg = abi.default_cfg(method, 10)
    fix = oa.ReferenceChannel(code50, 101 + method, 13.0).groups(eb, 16)
    _, cw = _check(code50, cfg, fix, 16)
    if eb <= 3.5 and method in (2, 5):
        assert cw[:, 1].max() > 0  # the bit-flipping stage is exercised


def test_matches_the_scalar_oracle(abi, code50):
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 131, 13.0).groups(3.5, 16)
    _check(code50, cfg, fix, 16, kind="oracle")


@pytest.mark.parametrize("method", [1, 2, 5])
def test_messages_streamed_through_hbm(abi, code50, method):
    cfg = abi.default_cfg(method, 10)
    fix = oa.ReferenceChannel(code50, 107, 13.0).groups(3.5, 16)
    _check(code50, cfg, fix, 16, store=abi.MSG_HBM)


def test_method_5_on_16qam(abi, code50):
    cfg = abi.default_cfg(5, 10)
    fix = oa.ReferenceChannel(code50, 109, 12.5, mod_type=4).groups(5.6, 16)
    _check(code50, cfg, fix, 16)


@pytest.mark.parametrize("mode", [1, 2])
def test_ef_elimination(abi, lib, code50, mode):
    cfg = abi.default_cfg(2, 10)
    assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), mode) == 0
    fix = oa.ReferenceChannel(code50, 113, 13.0).groups(3.5, 16)
    _check(code50, cfg, fix, 16)


@pytest.mark.parametrize("preset", [1, 2])
def test_table_presets(abi, lib, code50, preset):
    cfg = abi.default_cfg(2, 10)
    assert lib.lnsfaid_cfg_table_preset(C.byref(cfg), preset) == 0
    fix = oa.ReferenceChannel(code50, 127, 13.0).groups(3.5, 16)
    _check(code50, cfg, fix, 16)


def test_derived_code_with_runtime_row_degree(abi, lib):
    from test_gpu_more import _derived_code
    dc = _derived_code(abi, lib, [67, 68], 2)
    assert list(dc.deg) == [23, 22, 21]
    cfg = abi.default_cfg(2, 10)
    fix = oa.synth_llr(16, dc.N, 3.9, seed=23)
    _check(dc, cfg, fix, 16)


def test_unsatisfied_is_zero_exactly_where_the_codeword_stopped_clean(abi, code50):
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 137, 13.0).groups(3.4, 32)
    d = abi.Decoder(code50, cfg, 0, 32)
    out, cw = d.decode_codewords(fix, 32)
    d.close()
    host = unsatisfied(code50, out)
    assert np.array_equal(cw[:, 2], host)
    stopped = ~((cw[:, 0] == 10) & (cw[:, 1] == cfg.max_bf_iter))
    assert (cw[stopped, 2] == 0).all()
    assert (cw[~stopped, 2] > 0).any() and stopped.any()  # both kinds occur at 3.4 dB


def test_group_stats_are_the_maxima_and_method_0_is_the_same_under_both_rules(abi, code50):
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 139, 13.0).groups(3.6, 8)
    d = abi.Decoder(code50, cfg, 0, 8)
    out_cw, cw = d.decode_codewords(fix, 8)
    d.set_early_stop(CODEWORD)
    out, st = d.decode(fix, 8)
    assert np.array_equal(out, out_cw)
    assert np.array_equal(st, cw[:, :2].reshape(8, 32, 2).max(axis=1))
    d.close()
    nms = abi.default_cfg(0, 10)
    nms.factor_1 = nms.factor_2 = 24
    a, b = abi.Decoder(code50, nms, 0, 8), abi.Decoder(code50, nms, 0, 8)
    b.set_early_stop(CODEWORD)
    oa_, sa = a.decode(fix, 8)
    ob, sb = b.decode(fix, 8)
    oc, cwc = a.decode_codewords(fix, 8)
    a.close(); b.close()
    assert np.array_equal(oa_, ob) and np.array_equal(oa_, oc) and np.array_equal(sa, sb)
    assert (cwc[:, 0] == 10).all() and np.array_equal(cwc[:, 2], unsatisfied(code50, oc))


def test_the_setter(abi, code50):
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 149, 13.0).groups(3.5, 4)
    d = abi.Decoder(code50, cfg, 0, 4)
    assert d.early_stop() == 0
    with pytest.raises(RuntimeError):
        d.set_early_stop(2)
    g0, gs0 = d.decode(fix, 4)
    d.set_early_stop(CODEWORD)
    assert d.early_stop() == CODEWORD
    c1, cs1 = d.decode(fix, 4)
    d.set_early_stop(0)
    g2, gs2 = d.decode(fix, 4)
    d.close()
    fresh = abi.Decoder(code50, cfg, 0, 4)
    g3, gs3 = fresh.decode(fix, 4)
    fresh.close()
    ref, rst = oa.Oracle(code50, cfg, "avx2").decode(fix, 4)
    assert np.array_equal(g0, ref) and np.array_equal(g2, ref) and np.array_equal(g3, ref)
    assert np.array_equal(gs0, rst) and np.array_equal(gs2, rst) and np.array_equal(gs3, rst)
    pc, pst = per_codeword_oracle(code50, cfg, fix, 4)
    assert np.array_equal(c1.reshape(-1, code50.N), pc)
    assert np.array_equal(cs1, pst.reshape(4, 32, 2).max(axis=1))
    assert not np.array_equal(c1, g0)  # at 3.5 dB the rules differ somewhere


def test_mixed_rules_through_the_call_combiner(abi, code50):
    n_threads, n_calls = 6, 4
    methods = [2, 2, 5, 1, 2, 5]
    rules = [0, 1, 1, 0, 1, 0]
    fixes, refs = [], []
    for t in range(n_threads):
        cfg = abi.default_cfg(methods[t], 10)
        fix = oa.ReferenceChannel(code50, 400 + t, 13.0).groups(3.5, n_calls)
        d = abi.Decoder(code50, cfg, 0, n_calls)  # more than one group: direct path
        d.set_early_stop(rules[t])
        fixes.append(fix.reshape(n_calls, -1))
        refs.append(d.decode(fix, n_calls))
        d.close()
    errors = []
    start = threading.Barrier(n_threads)

    def worker(t):
        try:
            dec = abi.Decoder(code50, abi.default_cfg(methods[t], 10), device=0, max_groups=1)
            dec.set_early_stop(rules[t])
            start.wait()
            for rep in range(2):
                for c in range(n_calls):
                    out, st = dec.decode(np.ascontiguousarray(fixes[t][c]), 1)
                    ref = refs[t][0].reshape(n_calls, -1)[c]
                    if not np.array_equal(out, ref) or st.tolist() != [refs[t][1][c].tolist()]:
                        errors.append((t, rep, c))
            dec.close()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in threads)
    assert not errors, errors[:4]


def test_pinned_and_device_pointer_paths(abi, lib, code50):
    import torch
    ng = 128  # two pieces of 64 groups on the pinned path
    cfg = abi.default_cfg(2, 10)
    fix = oa.synth_llr(ng, code50.N, 3.6, seed=17)
    d = abi.Decoder(code50, cfg, 0, ng)
    out, cw = d.decode_codewords(fix, ng)  # pageable
    pin_in = np.empty_like(fix)
    pin_in[:] = fix
    pin_out = np.empty(ng * 32 * code50.N, np.int8)
    assert lib.lnsfaid_host_register(pin_in.ctypes.data, pin_in.nbytes) == 0
    assert lib.lnsfaid_host_register(pin_out.ctypes.data, pin_out.nbytes) == 0
    cw2 = np.zeros_like(cw)
    try:
        assert lib.lnsfaid_decode_codewords(d.ctx, pin_in.ctypes.data, ng, pin_out.ctypes.data, cw2.ctypes.data) == 0
    finally:
        lib.lnsfaid_host_unregister(pin_in.ctypes.data)
        lib.lnsfaid_host_unregister(pin_out.ctypes.data)
    assert np.array_equal(pin_out, out) and np.array_equal(cw2, cw)
    d_fix = torch.from_numpy(fix).cuda()
    d_out = torch.empty(fix.size, dtype=torch.int8, device="cuda")
    d_cw = torch.zeros((ng * 32, 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.decode_codewords_device(d_fix.data_ptr(), ng, d_out.data_ptr(), d_cw.data_ptr())
    assert np.array_equal(d_out.cpu().numpy(), out) and np.array_equal(d_cw.cpu().numpy(), cw)
    d.set_early_stop(CODEWORD)
    d_st = torch.zeros((ng, 2), dtype=torch.int32, device="cuda")
    d.decode_device(d_fix.data_ptr(), ng, d_out.data_ptr(), d_st.data_ptr())
    assert np.array_equal(d_out.cpu().numpy(), out)
    assert np.array_equal(d_st.cpu().numpy(), cw[:, :2].reshape(ng, 32, 2).max(axis=1))
    d.close()
    sub = np.random.default_rng(3).choice(ng * 32, 256, replace=False)
    ref, rst = per_codeword_oracle(code50, cfg, fix, ng, cws=sub)
    assert np.array_equal(out.reshape(-1, code50.N)[sub], ref) and np.array_equal(cw[sub, :2], rst)


def test_refusals(abi, lib, code50):
    fix = oa.synth_llr(1, code50.N, 3.6, seed=1)
    out = np.empty(fix.size, np.int8)
    nms = abi.default_cfg(0, 10)
    nms.factor_1, nms.factor_2 = 24, 26  # two factors: the two-rows kernel
    table = abi.default_cfg(2, 10)
    table.v2c_map[0][1][3] = 3  # weight classes differ: the two-rows kernel
    for cfg in (nms, table):
        d = abi.Decoder(code50, cfg, 0, 1)
        assert lib.lnsfaid_decode_codewords(d.ctx, fix.ctypes.data, 1, out.ctypes.data, None) == -1
        d.set_early_stop(CODEWORD)
        assert lib.lnsfaid_decode(d.ctx, fix.ctypes.data, 1, out.ctypes.data, None) == -1
        d.set_early_stop(0)
        d.decode(fix, 1)  # the group rule still decodes it
        d.close()
    d = abi.Decoder(code50, abi.default_cfg(2, 10), 0, 1)
    d.select_waves(2)
    assert lib.lnsfaid_decode_codewords(d.ctx, fix.ctypes.data, 1, out.ctypes.data, None) == -1
    d.set_early_stop(CODEWORD)
    assert lib.lnsfaid_decode(d.ctx, fix.ctypes.data, 1, out.ctypes.data, None) == -1
    d.select_waves(0)
    d.decode(fix, 1)
    d.close()


def test_host_driver_early_stop_codeword(tmp_path, abi, code50):
    """lnsfaid_sim --early-stop codeword: the counters of one round of 2 streams at 3.5 dB equal the 32-copy port fed by the
    restated channel with the same seeds"""
    import re
    exe = os.path.join(oa.PKG_DIR, "host", "lnsfaid_sim")
    prof = open(os.path.join(oa.PKG_DIR, "host", "Profile.txt")).read()
    prof = prof.replace("StartSNR: 3.3", "StartSNR: 3.5").replace("EndSNR: 3.85", "EndSNR: 3.55")
    (tmp_path / "Profile.txt").write_text(prof)
    res = subprocess.run([exe, "--streams", "2", "--gpus", "1", "--max-rounds", "1", "--early-stop", "codeword"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert "early stop: codeword" in res.stdout
    row = [l for l in res.stdout.splitlines() if re.match(r"\s*3.5\s", l)][-1].split()
    got = [int(row[1]), int(row[2]), int(row[3]), int(row[6])]
    cfg = abi.default_cfg(2, 10)
    want = [0, 0, 0, 0]
    for seed in (101, 103):
        fix = oa.ReferenceChannel(code50, seed, 13.0).groups(3.5, 50)
        dec, _ = per_codeword_oracle(code50, cfg, fix, 50)
        c = oa.Oracle(code50, cfg).count_errors(np.ascontiguousarray(dec.reshape(-1)), None, 50)
        want = [w + x for w, x in zip(want, c)]
    assert got == want, (got, want, res.stdout)


def test_batch_of_65536_codewords(abi, code50):
    ng = 2048
    cfg = abi.default_cfg(2, 10)
    fix = oa.synth_llr(ng, code50.N, 3.6, seed=2024)
    d = abi.Decoder(code50, cfg, 0, ng)
    out, cw = d.decode_codewords(fix, ng)
    d.close()
    out = out.reshape(ng * 32, code50.N)
    assert np.array_equal(cw[:, 2], unsatisfied(code50, out))
    sub = np.sort(np.random.default_rng(4096).choice(ng * 32, 4096, replace=False))
    ref, rst = per_codeword_oracle(code50, cfg, fix, ng, cws=sub)
    assert np.array_equal(out[sub], ref) and np.array_equal(cw[sub, :2], rst)
