"""CPU tests of the device encoder's host side: the compact inverse of the parity part (lnsfaid_code_parity_inverse), the
message generator of lnsfaid_frontend_random_frames restated in numpy, and the compiled encoder kernel (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import encoder_ref as er
import oracle_abi as oa

E_INVAL, E_CODE = -1, -2
MB, Z = 12, 256
CIRC_BYTES = MB * MB * Z // 8  # 4608


def _parity_inverse(lib, code):
    circ = np.zeros(CIRC_BYTES, dtype=np.uint8)
    rc = lib.lnsfaid_code_parity_inverse(C.byref(code.code), circ.ctypes.data, circ.size)
    return rc, circ


@pytest.fixture(scope="module")
def binv_full(lib, code50):
    rc, circ = _parity_inverse(lib, code50)
    assert rc == 0
    return circ, er.unpack_parity_inverse(circ, MB)


def test_parity_inverse_equals_the_test_encoders(encoder, binv_full):
    circ, full = binv_full
    assert full.shape == (3072, 3072)
    assert np.array_equal(full, encoder.Binv)
    # dense, as DESIGN.md §3.8 says: every circulant weight in 109 .. 150
    w = np.unpackbits(circ.reshape(MB * MB, Z // 8), axis=1).sum(axis=1)
    assert w.min() >= 109 and w.max() <= 150


def test_parity_part_times_inverse_is_identity(code50, binv_full):
    _, full = binv_full
    H = er.parity_matrix(code50)
    B = H[:, code50.K:].astype(np.float32)
    prod = np.rint(B @ full.astype(np.float32)).astype(np.int64) & 1
    assert np.array_equal(prod, np.eye(3072, dtype=np.int64))


def test_singular_parity_part_and_short_buffer(abi, lib, code50):
    dc = er.derived_code(abi, lib, [68], 11)  # column 68 leaves block row 11: B loses rank
    rc, _ = _parity_inverse(lib, dc)
    assert rc == E_CODE
    circ = np.zeros(CIRC_BYTES, dtype=np.uint8)
    assert lib.lnsfaid_code_parity_inverse(C.byref(code50.code), circ.ctypes.data, CIRC_BYTES - 1) == E_INVAL
    assert not circ.any()
    assert lib.lnsfaid_code_parity_inverse(C.byref(code50.code), None, CIRC_BYTES) == E_INVAL
    broken = abi.Code50GPON(lib)  # not quasi-cyclic: the same rule as lnsfaid_create
    broken.pos_vn[5], broken.pos_vn[6] = broken.pos_vn[6], broken.pos_vn[5]
    assert lib.lnsfaid_code_parity_inverse(C.byref(broken.code), circ.ctypes.data, CIRC_BYTES) == E_CODE


def test_invertible_derived_code(abi, lib):
    """Row degrees 23 / 22 / 21 (columns 67 and 68 dropped from block rows 2 and up): B keeps full rank, and the compact
    inverse is its inverse."""
    dc = er.derived_code(abi, lib, [67, 68], 2)
    rc, circ = _parity_inverse(lib, dc)
    assert rc == 0
    H = er.parity_matrix(dc)
    full = er.unpack_parity_inverse(circ, MB)
    prod = np.rint(H[:, dc.K:].astype(np.float32) @ full.astype(np.float32)).astype(np.int64) & 1
    assert np.array_equal(prod, np.eye(3072, dtype=np.int64))


# (key, j) -> h = mix64(mix64(key) + (j + 1) * 0x9E3779B97F4A7C15); key 0, j 0 is splitmix64's first output from state 0
KNOWN = [(0, 0, 0xE220A8397B1DCDAF), (1, 0, 0xBFEF8030DDC2D772), (101 | 101 << 16 | 101 << 32, 0, 0x46AE5AF811C86F0D),
         (101 | 101 << 16 | 101 << 32, 14591, 0x59194A92E741C949), (0xFFFFFFFFFFFFFFFF, 7, 0xC62E5652A694833F)]


def test_message_generator_known_answers():
    assert er.mix64_int(0) == 0 and er.mix64_int(1) == 0x5692161D100B05E5
    for key, j, h in KNOWN:
        assert er.mix64_int(er.mix64_int(key) + (j + 1) * er.GOLDEN_GAMMA) == h
        assert int(er.message_words(key, j + 1)[j]) == h & 0xFFFFFFFF
    bits = er.messages([KNOWN[2][0]], 14592)
    assert bits.shape == (1, 32, 14592)
    for l in range(32):
        assert bits[0, l, 0] == (KNOWN[2][2] >> l) & 1 and bits[0, l, 14591] == (KNOWN[3][2] >> l) & 1
    # roughly balanced and different between streams
    two = er.messages([5, 6], 14592)
    assert abs(float(two.mean()) - 0.5) < 0.01 and (two[0] != two[1]).mean() > 0.45


def test_encoder_kernel_has_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(oa.ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(oa.ROOT, "include"), "-I" + csrc,
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "lnsfaid_encoder.hip"), "-o", os.devnull],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stderr)]
    assert len(scratch) == 2 and all(s == 0 for s in scratch), res.stderr
