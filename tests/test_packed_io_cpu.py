"""Packed decode I/O without a GPU (include/lnsfaid.h "packed decode I/O"): the new symbols, the host format helpers against a
numpy restatement of the formats, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

NEW_SYMBOLS = ["lnsfaid_decode_packed", "lnsfaid_decode_packed_device", "lnsfaid_decode_codewords_packed",
               "lnsfaid_decode_codewords_packed_device", "lnsfaid_count_errors_packed", "lnsfaid_count_errors_packed_device",
               "lnsfaid_pack_llr4", "lnsfaid_unpack_bits", "lnsfaid_pack_bits"]
E_INVAL = -1


def np_pack_llr4(fix):
    """element e: two's-complement nibble in byte e // 2, low nibble for even e"""
    u = fix.astype(np.int16) & 15
    return (u[0::2] | (u[1::2] << 4)).astype(np.uint8)


def np_unpack_llr4(llr4):
    lo = (llr4 & 15).astype(np.int16)
    hi = (llr4 >> 4).astype(np.int16)
    out = np.empty(2 * llr4.size, np.int16)
    out[0::2], out[1::2] = lo, hi
    return np.where(out >= 8, out - 16, out).astype(np.int8)


def test_new_symbols_resolve(lib):
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None


def test_pack_llr4_matches_the_format_and_keeps_minus_8(abi, lib):
    rng = np.random.default_rng(7)
    fix = rng.integers(-8, 8, size=32 * 17664, dtype=np.int8)
    fix[:16] = np.arange(-8, 8, dtype=np.int8)
    packed = abi.pack_llr4(fix, lib)
    assert np.array_equal(packed, np_pack_llr4(fix))
    assert packed[0] == 0x98  # -8 low, -7 high
    assert np.array_equal(np_unpack_llr4(packed), fix)


def test_unpack_bits_matches_numpy_packbits_little(abi, lib):
    rng = np.random.default_rng(11)
    dec = rng.integers(0, 2, size=32 * 17664, dtype=np.int8)
    words = np.packbits(dec.astype(np.uint8), bitorder="little").view("<u4")
    assert np.array_equal(abi.unpack_bits(words, lib), dec)
    w = np.array([0x80000001], dtype=np.uint32)
    got = abi.unpack_bits(w, lib)
    assert got[0] == 1 and got[31] == 1 and got[1:31].sum() == 0


def test_pack_bits_round_trips(abi, lib):
    rng = np.random.default_rng(13)
    msg = rng.integers(0, 2, size=32 * 14592, dtype=np.int8)
    packed = abi.pack_bits(msg, lib)
    assert np.array_equal(packed, np.packbits(msg.astype(np.uint8), bitorder="little"))
    assert np.array_equal(abi.unpack_bits(packed.view("<u4"), lib)[:msg.size], msg)


def test_helper_argument_errors(lib):
    fix = np.zeros(64, np.int8)
    out = np.zeros(64, np.uint8)
    assert lib.lnsfaid_pack_llr4(fix.ctypes.data, 63, out.ctypes.data) == E_INVAL  # odd count
    assert lib.lnsfaid_pack_llr4(None, 64, out.ctypes.data) == E_INVAL
    assert lib.lnsfaid_pack_llr4(fix.ctypes.data, 64, None) == E_INVAL
    assert lib.lnsfaid_pack_llr4(None, 0, None) == 0
    for bad in (8, -9, 127, -128):
        f = fix.copy()
        f[5] = bad
        assert lib.lnsfaid_pack_llr4(f.ctypes.data, 64, out.ctypes.data) == E_INVAL, bad
    words = np.zeros(2, np.uint32)
    dec = np.zeros(64, np.int8)
    assert lib.lnsfaid_unpack_bits(words.ctypes.data, 48, dec.ctypes.data) == E_INVAL  # not whole words
    assert lib.lnsfaid_unpack_bits(None, 64, dec.ctypes.data) == E_INVAL
    assert lib.lnsfaid_unpack_bits(words.ctypes.data, 64, None) == E_INVAL
    assert lib.lnsfaid_unpack_bits(None, 0, None) == 0
    msg = np.zeros(64, np.int8)
    assert lib.lnsfaid_pack_bits(msg.ctypes.data, 60, out.ctypes.data) == E_INVAL
    msg[3] = 2
    assert lib.lnsfaid_pack_bits(msg.ctypes.data, 64, out.ctypes.data) == E_INVAL
    assert lib.lnsfaid_pack_bits(None, 0, None) == 0


def test_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(1 << 20, np.uint8)
    p = buf.ctypes.data
    out = (C.c_uint64 * 4)()
    for name in ("lnsfaid_decode_packed", "lnsfaid_decode_packed_device", "lnsfaid_decode_codewords_packed",
                 "lnsfaid_decode_codewords_packed_device"):
        assert getattr(lib, name)(None, p, 1, p, None) == E_INVAL, name
        assert getattr(lib, name)(None, None, 0, None, None) == E_INVAL, name
    assert lib.lnsfaid_count_errors_packed(None, p, None, 1, out) == E_INVAL
    assert lib.lnsfaid_count_errors_packed_device(None, p, None, 1, out) == E_INVAL


@pytest.mark.parametrize("name", ["lnsfaid_pack_llr4", "lnsfaid_unpack_bits", "lnsfaid_pack_bits"])
def test_helpers_declared_in_the_header(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert ("int %s(" % name) in open(os.path.join(root, "include", "lnsfaid.h")).read()
