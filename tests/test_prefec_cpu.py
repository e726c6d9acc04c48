"""CPU tests of the pre-FEC error counters (include/lnsfaid.h "pre-FEC error counters"):
lnsfaid_prefec_errors_host against the numpy restatement of prefec_ref.py on noisy symbols with values planted around the
decision threshold, against counts derived by hand, the argument rules, and the bit error rate theory predicts (no GPU needed)."""
import ctypes as C
import math

import numpy as np
import pytest

import demap_ref as dr
import oracle_abi as oa
import prefec_ref as pr
from test_gpu_demap import EB_N0

E_INVAL = -1
CASES = sorted(EB_N0)


def _sigma(mod, il):
    return oa.load().lnsfaid_frontend_sigma(EB_N0[(mod, il)], mod, oa.ReferenceChannel.RATE)


@pytest.mark.parametrize("mod,il", CASES, ids=["m%d_i%d" % k for k in CASES])
def test_host_equals_the_restatement(abi, lib, code50, mod, il):
    n_groups, N, M = 2, code50.N, code50.M
    rng = np.random.default_rng(500 + 10 * mod + il)
    frames = rng.integers(0, 2, (n_groups, 32, N), dtype=np.int8)
    rx = pr.plant(dr.noisy_symbols(rng, frames, mod, il, _sigma(mod, il)), n_groups, N, M, il, mod)
    sent = pr.sent_of_frames(frames, M)
    for scope in (pr.INFO, pr.CODEWORD):
        want = pr.count(rx, n_groups, N, M, il, mod, sent, scope)
        assert abi.prefec_errors_host(N, M, il, rx, n_groups, mod, sent, scope, lib) == want, (mod, il, scope)
        assert want[0] == 64 and 0 < want[2] < 0.5 * 64 * N and 0 < want[3] <= want[2] and want[1] == 64
        # against the all-zero codeword the same symbols are wrong wherever a 1 was sent
        zero = pr.count(rx, n_groups, N, M, il, mod, None, scope)
        assert abi.prefec_errors_host(N, M, il, rx, n_groups, mod, None, scope, lib) == zero
        assert zero[2] > 0.3 * 64 * (N - M)
    if mod == 1:  # every bit its own symbol, and no interleaver whatever the argument says
        assert want[3] == want[2]
        assert abi.prefec_errors_host(N, M, 3, rx, n_groups, mod, sent, pr.CODEWORD, lib) == want


def test_planted_values_decide_as_specified(abi, lib):
    """every threshold value alone against sent bits 0 and 1: only +Inf and the positive values decide 1"""
    n_var, n_check = 96, 24
    ones = np.ones(32 * n_var, dtype=np.int8)
    for v in pr.THRESHOLD_VALUES:
        rx = np.full(32 * n_var, v, dtype=np.float32)
        decides_one = bool(v > 0)
        for mod in (1, 2):
            got0 = abi.prefec_errors_host(n_var, n_check, 1, rx, 1, mod, None, pr.CODEWORD, lib)
            got1 = abi.prefec_errors_host(n_var, n_check, 1, rx, 1, mod, ones, pr.CODEWORD, lib)
            all_wrong = [32, 32, 32 * n_var, 32 * n_var // mod]
            assert got0 == (all_wrong if decides_one else [32, 0, 0, 0]), (v, mod)
            assert got1 == ([32, 0, 0, 0] if decides_one else all_wrong), (v, mod)


def _noiseless(mod, il, n_var, n_groups=1, seed=5):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 2, (n_groups, 32, n_var), dtype=np.int8)
    return frames, dr.noisy_symbols(rng, frames, mod, il, 0.0)


@pytest.mark.parametrize("mod,il,n_var,n_check", [(1, 1, 96, 24), (2, 1, 96, 24), (4, 1, 96, 24), (6, 3, 96, 24), (8, 8, 128, 32), (2, 2, 96, 24), (4, 4, 96, 24)])
def test_noiseless_symbols_have_no_errors(abi, lib, mod, il, n_var, n_check):
    frames, rx = _noiseless(mod, il, n_var, n_groups=3)
    sent = pr.sent_of_frames(frames, n_check)
    for scope in (pr.INFO, pr.CODEWORD):
        assert abi.prefec_errors_host(n_var, n_check, il, rx, 3, mod, sent, scope, lib) == [96, 0, 0, 0]
        assert pr.count(rx, 3, n_var, n_check, il, mod, sent, scope) == [96, 0, 0, 0]


def test_constructed_counts(abi, lib):
    """QPSK on n_var = 96, K = 72: float f of a group is stream position f, symbol f // 2; negating a float flips its decision"""
    n_var, n_check = 96, 24

    def run(il, negate, scope):
        frames, rx = _noiseless(2, il, n_var)
        rx[negate] = -rx[negate]
        return abi.prefec_errors_host(n_var, n_check, il, rx, 1, 2, pr.sent_of_frames(frames, n_check), scope, lib)

    for scope in (pr.INFO, pr.CODEWORD):
        # two bits of one symbol: 1 symbol, 2 bits
        assert run(1, [10, 11], scope) == [32, 1, 2, 1]
        # frame 0 position 3; frame 1 positions 5 and 6 (symbols 2 and 3 of that frame)
        assert run(1, [3, 96 + 5, 96 + 6], scope) == [32, 2, 3, 3]
        # frame 31, last information bit
        assert run(1, [31 * 96 + 71], scope) == [32, 1, 1, 1]
    # code bit 80 >= K of frame 0 and code bit 72 = K of frame 2: in the codeword scope only
    assert run(1, [80, 2 * 96 + 72], pr.INFO) == [32, 0, 0, 0]
    assert run(1, [80, 2 * 96 + 72], pr.CODEWORD) == [32, 2, 2, 2]
    # I = 2: position p carries code bit 48 (p % 2) + p // 2, so symbol 30 holds code bits 30 (in scope) and 78 (parity)
    assert run(2, [60, 61], pr.INFO) == [32, 1, 1, 1]
    assert run(2, [60, 61], pr.CODEWORD) == [32, 1, 2, 1]
    assert run(2, [61], pr.INFO) == [32, 0, 0, 0]
    assert run(2, [61], pr.CODEWORD) == [32, 1, 1, 1]
    # I = 2, symbol 10 holds code bits 10 and 58, both information bits
    assert run(2, [20, 21], pr.INFO) == [32, 1, 2, 1]


def test_out_is_added_to(abi, lib):
    n_var, n_check = 96, 24
    frames, rx = _noiseless(2, 1, n_var, n_groups=2)
    rx[[10, 11, 32 * 96 + 1]] *= -1
    sent = pr.sent_of_frames(frames, n_check)
    assert abi.prefec_errors_host(n_var, n_check, 1, rx, 2, 2, sent, pr.INFO, lib) == [64, 2, 3, 2]
    assert abi.prefec_errors_host(n_var, n_check, 1, rx, 2, 2, sent, pr.INFO, lib, out=[5, 6, 7, 1 << 40]) == [69, 8, 10, (1 << 40) + 2]


def test_argument_checks(lib):
    n_var, n_check = 96, 24
    rx = np.zeros(2 * 32 * 128, dtype=np.float32)
    sent = np.zeros(32 * 128, dtype=np.int8)
    out = (C.c_uint64 * 4)()

    def call(nv=n_var, nc=n_check, il=1, mod=2, scope=pr.INFO, n_groups=1, rxp=rx.ctypes.data, sentp=sent.ctypes.data, outp=out):
        return lib.lnsfaid_prefec_errors_host(nv, nc, il, rxp, n_groups, mod, sentp, scope, outp)

    for mod in (1, 2, 4, 6, 8):
        assert call(mod=mod) == 0 and call(mod=mod, scope=pr.CODEWORD) == 0
    for mod in (0, 3, 5, 7, 9, -2):
        assert call(mod=mod) == E_INVAL
    for il in (0, -1, 5, 7, 97):
        assert call(il=il) == E_INVAL
    assert call(il=96) == 0
    for scope in (0, 3, -1):
        assert call(scope=scope) == E_INVAL
    # a symbol must not straddle two frames: 32 * 100 is a multiple of 8 (the demapper takes it), 100 is not
    assert call(nv=100, nc=25, mod=4) == 0 and call(nv=100, nc=25, mod=8) == E_INVAL
    assert lib.lnsfaid_demap_host(100, 25, 1, rx.ctypes.data, 1, 8, 13.0, sent.ctypes.data) == 0
    assert call(nv=97, nc=25, mod=1) == 0 and call(nv=97, nc=25, mod=2) == E_INVAL
    assert call(nc=0) == E_INVAL and call(nc=n_var) == E_INVAL
    assert call(rxp=None) == E_INVAL and call(outp=None) == E_INVAL
    assert call(sentp=None) == 0  # the all-zero codeword
    before = list(out)
    assert call(n_groups=0, rxp=None, sentp=None, outp=None) == 0 and call(n_groups=0, rxp=None, sentp=None) == 0
    assert call(n_groups=0, scope=0) == E_INVAL  # the rules come first
    assert list(out) == before


def test_bit_error_rate_follows_theory(abi, lib, code50):
    """QPSK, no interleaver, whole codewords at the sigma of 3.6 dB: every bit sees N(0, (sigma / sqrt 2)^2) on an amplitude of
    0.707107, so it is wrong with probability Q(0.707107 sqrt 2 / sigma) = Q(1 / sigma); 5 binomial standard deviations"""
    n_groups, N, M = 2, code50.N, code50.M
    rng = np.random.default_rng(36)
    frames = rng.integers(0, 2, (n_groups, 32, N), dtype=np.int8)
    sigma = _sigma(2, 1)
    rx = dr.noisy_symbols(rng, frames, 2, 1, sigma)
    got = abi.prefec_errors_host(N, M, 1, rx, n_groups, 2, pr.sent_of_frames(frames, M), pr.CODEWORD, lib)
    n = n_groups * 32 * N
    p = 0.5 * math.erfc((1.0 / sigma) / math.sqrt(2))
    print("ModErrorBits %d of %d, expected %.1f +- %.1f" % (got[2], n, n * p, math.sqrt(n * p * (1 - p))))
    assert abs(got[2] - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert got[0] == 64 and got[1] == 64 and got[2] / 2 <= got[3] <= got[2]
