"""CPU tests of the demapper for received symbols (include/lnsfaid.h "demapper for received symbols"):
the restated channel and demapper of demap_ref.py against the oracle's chain, lnsfaid_demap_host / _packed_host against
both, the argument rules, and the compiled kernel's resource figures (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import demap_ref as dr
import oracle_abi as oa

E_INVAL = -1
SEED = 211


def _case(cfg):
    """(frames, rx of the restated channel, the oracle's fixInput) of one group"""
    mod, il, scale, eb, n_var, n_check = cfg
    olib = oa.load()
    frames = np.random.default_rng(1).integers(0, 2, (32, n_var), dtype=np.int8)
    sigma = olib.lnsfaid_frontend_sigma(eb, mod, oa.ReferenceChannel.RATE)
    fe = oa.Frontend()
    olib.lnsfaid_frontend_seed(C.byref(fe), SEED)
    want = np.empty(32 * n_var, dtype=np.int8)
    assert olib.lnsfaid_frontend_group(C.byref(fe), n_var, n_check, frames.ctypes.data, n_var, mod, il, sigma, scale, want.ctypes.data) == 0
    rx = dr.reference_channel_symbols(SEED, frames, mod, il, sigma)
    return frames, rx, want


@pytest.fixture(scope="module")
def cases():
    return [_case(cfg) for cfg in dr.SMALL_CONFIGS]


def _planted_rx(mod, n_var, n_check, il, scale):
    rng = np.random.default_rng(7)
    rx = (rng.standard_normal(dr.rx_floats(n_var, mod)) * 0.5).astype(np.float32)
    return dr.plant(rx, 1, n_var, n_check, il, mod, scale)


# one group of a small code for every mod_type: (mod_type, I, scale, n_var, n_check)
PLANTED = [(1, 1, 13.0, 96, 24), (2, 1, 13.0, 96, 24), (4, 1, 12.5, 96, 24), (6, 1, 12.5, 96, 24), (8, 1, 40.0, 128, 32),
           (2, 3, 13.0, 96, 24), (4, 4, 12.5, 96, 24), (6, 3, 12.5, 96, 24), (8, 8, 40.0, 128, 32)]


def test_restated_chain_equals_the_oracle(cases):
    """pins demap_ref.py: channel (a) + demapper (b) give the oracle's bytes; does not depend on the library"""
    levels, total = set(), 0
    for cfg, (_, rx, want) in zip(dr.SMALL_CONFIGS, cases):
        mod, il, scale, _, n_var, n_check = cfg
        got = dr.demap(rx, 1, n_var, n_check, il, mod, scale)
        assert np.array_equal(got, want), (cfg, int((got != want).sum()))
        total += want.size
        if scale < 1e6:
            levels |= set(np.unique(want).tolist())
        else:
            assert (want == -7).mean() > 0.98  # the out-of-range branch, but for the few levels within 2^31 / scale of zero
    assert total == 23552 and levels == set(range(-7, 8))


def test_host_demapper_equals_the_oracle(abi, lib, cases):
    for cfg, (_, rx, want) in zip(dr.SMALL_CONFIGS, cases):
        mod, il, scale, _, n_var, n_check = cfg
        got = abi.demap_host(n_var, n_check, il, rx, 1, mod, scale, lib)
        assert got.dtype == np.int8 and np.array_equal(got, want), (cfg, int((got != want).sum()))


@pytest.mark.parametrize("mod,il,scale,n_var,n_check", PLANTED)
def test_host_demapper_on_planted_values(abi, lib, mod, il, scale, n_var, n_check):
    rx = _planted_rx(mod, n_var, n_check, il, scale)
    want = dr.demap(rx, 1, n_var, n_check, il, mod, scale)
    got = abi.demap_host(n_var, n_check, il, rx, 1, mod, scale, lib)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert set(np.unique(got).tolist()) == set(range(-7, 8))
    # NaN, both infinities and |y| >= 2^31 of either sign end at -7 wherever they stand
    spec = np.resize(dr.special_values(scale), rx.size)
    only = abi.demap_host(n_var, n_check, il, spec, 1, mod, scale, lib)
    direct = np.ones(32 * n_var, dtype=bool) if mod == 1 else (np.arange(32 * n_var) % mod < 2)
    assert (only[dr.destination(n_var, n_check, 1 if mod == 1 else il)[direct]] == -7).all()


def test_packed_host_output(abi, lib, cases):
    inputs = [(cfg[0], cfg[1], cfg[2], cfg[4], cfg[5], rx) for cfg, (_, rx, _) in zip(dr.SMALL_CONFIGS, cases)]
    inputs += [(mod, il, scale, n_var, n_check, _planted_rx(mod, n_var, n_check, il, scale)) for mod, il, scale, n_var, n_check in PLANTED]
    for mod, il, scale, n_var, n_check, rx in inputs:
        fix = abi.demap_host(n_var, n_check, il, rx, 1, mod, scale, lib)
        out = np.full(16 * n_var + 32, 0x55, dtype=np.uint8)
        body = out[16:16 + 16 * n_var]
        assert lib.lnsfaid_demap_packed_host(n_var, n_check, il, rx.ctypes.data, 1, mod, scale, body.ctypes.data) == 0
        assert np.array_equal(body, abi.pack_llr4(fix, lib)) and np.array_equal(body, dr.pack(fix))
        assert (out[:16] == 0x55).all() and (out[16 + 16 * n_var:] == 0x55).all()
        # no byte keeps the fill: the same call over a buffer filled with another value gives the same bytes
        other = np.full(16 * n_var, 0xAA, dtype=np.uint8)
        assert lib.lnsfaid_demap_packed_host(n_var, n_check, il, rx.ctypes.data, 1, mod, scale, other.ctypes.data) == 0
        assert np.array_equal(other, body)


def test_mod_type_1_is_the_quantiser_regrouped(abi, lib):
    n_var, n_check, scale, groups = 96, 24, 13.0, 2
    K = n_var - n_check
    rng = np.random.default_rng(3)
    rx = (rng.standard_normal(groups * 32 * n_var) * 0.6).astype(np.float32)
    dr.plant(rx, groups, n_var, n_check, 1, 1, scale)
    q = dr.quantise(rx, scale).reshape(groups, 32, n_var)
    want = np.concatenate([np.concatenate([q[g, :, :K].reshape(-1), q[g, :, K:].reshape(-1)]) for g in range(groups)])
    got1 = abi.demap_host(n_var, n_check, 1, rx, groups, 1, scale, lib)
    got3 = abi.demap_host(n_var, n_check, 3, rx, groups, 1, scale, lib)
    assert np.array_equal(got1, want) and np.array_equal(got3, want)
    assert np.array_equal(abi.demap_packed_host(n_var, n_check, 3, rx, groups, 1, scale, lib), dr.pack(want))


def test_argument_checks(lib):
    n_var, n_check = 96, 24
    rx = np.zeros(2 * 32 * n_var, dtype=np.float32)
    fix = np.zeros(32 * 128, dtype=np.int8)  # (room for the cases with n_var = 97)
    llr4 = np.zeros(16 * 128, dtype=np.uint8)

    def both(nv, nc, il, mod, n_groups=1, rxp=rx.ctypes.data, fixp=fix.ctypes.data, llrp=llr4.ctypes.data):
        return (lib.lnsfaid_demap_host(nv, nc, il, rxp, n_groups, mod, 13.0, fixp),
                lib.lnsfaid_demap_packed_host(nv, nc, il, rxp, n_groups, mod, 13.0, llrp))

    for mod in (1, 2, 4, 6, 8):
        assert both(n_var, n_check, 1, mod) == (0, 0)
    for mod in (0, 3, 5, 7, 9, -2):
        assert both(n_var, n_check, 1, mod) == (E_INVAL, E_INVAL)
    for il in (0, -1, 5, 7, 97):  # 0, or not dividing n_var
        assert both(n_var, n_check, il, 2) == (E_INVAL, E_INVAL)
    assert both(n_var, n_check, 96, 2) == (0, 0)
    assert both(97, 25, 1, 2)[0] == 0 and both(97, 25, 1, 4)[0] == 0  # 32 * 97 is a multiple of 2 and 4 ...
    assert both(97, 25, 1, 6) == (E_INVAL, E_INVAL)                   # ... and not of 6
    # the packed form needs n_var and K even
    assert both(96, 23, 1, 2) == (0, E_INVAL) and both(97, 25, 1, 2) == (0, E_INVAL)
    assert both(n_var, 0, 1, 2) == (E_INVAL, E_INVAL) and both(n_var, n_var, 1, 2) == (E_INVAL, E_INVAL)
    # NULL buffers: an error with groups to do, a no-op without
    assert both(n_var, n_check, 1, 2, rxp=None) == (E_INVAL, E_INVAL)
    assert both(n_var, n_check, 1, 2, fixp=None, llrp=None) == (E_INVAL, E_INVAL)
    assert both(n_var, n_check, 1, 2, n_groups=0, rxp=None, fixp=None, llrp=None) == (0, 0)


def test_demap_kernels_have_no_scratch_and_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(oa.ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(oa.ROOT, "include"),
                          "-I" + csrc, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "lnsfaid_demap.hip"),
                          "-o", os.devnull], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    names = re.findall(r"Function Name: (\S+)", res.stderr)
    # mod_type 2 / 4 / 6 / 8 x int8 / packed x stream / gather / narrow
    assert len(names) == 24 and all("lnsfaid_demap_kernel" in n for n in names), names
    for what in (r"ScratchSize \[bytes/lane\]", "VGPRs Spill", "SGPRs Spill"):
        figures = [int(x) for x in re.findall(what + r": (\d+)", res.stderr)]
        assert len(figures) == 24 and all(f == 0 for f in figures), (what, figures)
