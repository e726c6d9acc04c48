"""The rotation-free layer step on the GPU (lnsfaid_kernel4z.hip, lnsfaid_select_zero_shift): the kernel that skips the byte
rotations on identity circulants against the rotating kernel forced by the switch and against the oracle - hard decisions, group
records and error counters - on bench.py's synthetic LLRs at the smallest shape, and which kernel a context selects."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_abi as oa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZG_50GPON = [0, 5, 0, 0, 1, 0, 0, 2, 4, 1, 0, 1]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("lnsfaid_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def llrs(bench):
    """bench.py's frames, drawn once: (Eb/N0, groups) -> int8 fixInput on the host"""
    import torch
    return {(eb, ng): bench.synth_llr(torch, "cuda:0", ng, eb, 1234 + ng).cpu().numpy().reshape(-1)
            for eb, ng in [(3.0, 1), (3.6, 1), (4.2, 1), (3.6, 3)]}


def _three_ways(abi, code50, method, fix, ng):
    cfg = abi.default_cfg(method, 10)
    oracle = oa.Oracle(code50, cfg)
    ref, ref_stats = oracle.decode(fix, ng)
    dec = abi.Decoder(code50, cfg, device=0, max_groups=ng)
    on, zg = dec.zero_shift_groups(12)
    assert on and zg == ZG_50GPON
    new, new_stats = dec.decode(fix, ng)
    new_counters = dec.count_errors(new, None, ng)
    dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
    assert dec.zero_shift_groups(12) == (False, [0] * 12)
    old, old_stats = dec.decode(fix, ng)
    old_counters = dec.count_errors(old, None, ng)
    dec.close()
    assert np.array_equal(new, old) and np.array_equal(new_stats, old_stats) and new_counters == old_counters
    assert np.array_equal(new, ref), np.nonzero((new != ref).reshape(ng * 32, code50.N).any(axis=1))[0][:8].tolist()
    assert np.array_equal(new_stats, ref_stats), (new_stats.tolist(), ref_stats.tolist())
    assert new_counters == oracle.count_errors(ref, None, ng)
    return new_stats


@pytest.mark.parametrize("method", [2, 1, 5])
@pytest.mark.parametrize("eb_n0", [3.0, 3.6, 4.2])
def test_one_group_equals_the_rotating_kernel_and_the_oracle(abi, code50, llrs, method, eb_n0):
    """At 3.6 dB some codewords of the group finish early and park while the others run on (the record of a parked codeword
    goes through HBM in the kernel's own edge order and comes back)."""
    _three_ways(abi, code50, method, llrs[(eb_n0, 1)], 1)


def test_three_groups(abi, code50, llrs):
    """more than one group status word live"""
    _three_ways(abi, code50, 2, llrs[(3.6, 3)], 3)


def test_selection(abi, lib, code50):
    import ctypes as C
    dec = abi.Decoder(code50, abi.default_cfg(2, 10), device=0, max_groups=1)
    assert dec.zero_shift_groups(12) == (True, ZG_50GPON)
    assert dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_OFF)
    assert dec.zero_shift_groups(12) == (False, [0] * 12)
    assert dec.kernel_residency() == (8, 8)
    dec.select_zero_shift(abi.ZERO_SHIFT_ON)
    assert dec.zero_shift_groups(12)[0]
    # outside the instance set: messages streamed through HBM, two waves per codeword, the two-rows kernel
    dec.select_message_store(abi.MSG_HBM)
    assert dec.zero_shift_groups(12) == (False, [0] * 12)
    dec.select_message_store(0)
    dec.select_zero_shift(0)
    dec.select_waves(2)
    assert not dec.zero_shift_groups(12)[0]
    dec.select_waves(0)
    dec.select_kernel(2)
    assert not dec.zero_shift_groups(12)[0]
    with pytest.raises(RuntimeError):
        dec.select_zero_shift(abi.ZERO_SHIFT_ON)
    dec.close()
    # DecodeMethod 0 (no messages in registers) and the erasing EF_ELIMINATION 2 stay on the rotating kernel
    dec = abi.Decoder(code50, abi.default_cfg(0, 10), device=0, max_groups=1)
    assert not dec.zero_shift_groups(12)[0]
    dec.close()
    cfg = abi.default_cfg(2, 10)
    assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), 2) == 0
    dec = abi.Decoder(code50, cfg, device=0, max_groups=1)
    assert dec.zero_shift_groups(12) == (False, [0] * 12)
    dec.close()
