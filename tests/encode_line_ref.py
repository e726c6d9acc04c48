"""Helpers of the line-format encode tests (lnsfaid_encode_line*): the batches and their expected outputs from the independent numpy
encoder (tests/gf2_encoder.py) in the formats of tests/line_ref.py.  Shared by the CPU and the GPU test file; everything expensive is
computed once per session."""
import os

import numpy as np

import encoder_ref as er
import gf2_encoder
import line_ref as lr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNIT_VECTORS = 57

_cache = {}


def messages(n, K, seed):
    """[n, K] random information bits, a generator of its own for every codeword (seed + its index)"""
    msg = np.stack([np.random.default_rng(seed + c).integers(0, 2, K, dtype=np.uint8) for c in range(n)])
    assert msg.any(axis=1).all()
    return msg


def unit_vector_messages(K):
    """57 codewords, codeword cb carrying only information bit 256 cb + (97 cb + 5) mod 256: one bit in every block column of the
    built-in code, at a different place of each"""
    msg = np.zeros((UNIT_VECTORS, K), np.uint8)
    for cb in range(UNIT_VECTORS):
        msg[cb, 256 * cb + (97 * cb + 5) % 256] = 1
    return msg


def expected(encoder, msg, L):
    """(payload [n, K / 32], line [n, L / 32], bits [n, N / 32]) uint32 of the numpy encoder's codewords"""
    cw = encoder.encode(msg)
    n = cw.shape[0]
    line = lr.line_of(cw, L, lr.HARD).reshape(n, L // 32)
    bits = np.packbits(cw.astype(np.uint8), axis=1, bitorder="little").view("<u4").astype(np.uint32)
    return lr.payload_of(msg), line, bits


def batch(encoder, name, n=0, seed=0):
    """name "random" (n codewords from `seed`) or "unit": cached (payload, line, bits) of the built-in code"""
    key = (name, n, seed)
    if key not in _cache:
        msg = unit_vector_messages(encoder.K) if name == "unit" else messages(n, encoder.K, seed)
        _cache[key] = expected(encoder, msg, encoder.N - 384)
    return _cache[key]


def golden_codeword(N):
    """the reference's codeword as bits [N]"""
    return np.unpackbits(np.fromfile(os.path.join(GOLD, "codeword_50gpon.bin"), dtype=np.uint8))[:N]


def derived(abi, lib):
    """(code, its own numpy encoder) of the invertible derived code of test_encoder_tables.py: block columns 67 and 68 dropped from
    block rows 2 and up"""
    if "derived" not in _cache:
        dc = er.derived_code(abi, lib, [67, 68], 2)
        _cache["derived"] = (dc, gf2_encoder.Encoder(dc))
    return _cache["derived"]
