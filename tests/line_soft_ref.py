"""Independent numpy restatement of the line-format soft channel (include/lnsfaid.h "line-format soft channel"): the levels of
every position from the generator of line_link_ref.py (domain 3) and a table of fourteen thresholds, the nibble packing, and the
AWGN table from math.erfc.  Nothing here calls the library."""
import math

import numpy as np

from line_link_ref import codeword_numbers, draw

DEFAULT_SCALE = 13.0 / math.sqrt(2.0)


def ebn0_sigma(db, K, L):
    """noise deviation on a unit-amplitude axis at Eb/N0 `db` for the rate K / L on the line"""
    return 1.0 / math.sqrt(2.0 * (K / L) * 10.0 ** (db / 10.0))


def counts(key, first, n, L, table):
    """m + 7 = #{ i : u >= table[i] } for every position: int64 [n, L]; position 2 q is the low half of draw q, 2 q + 1 the high"""
    h = draw(key, codeword_numbers(first, n), 3, np.arange(L // 2))
    u = np.empty((n, L), dtype=np.uint64)
    u[:, 0::2] = h & np.uint64(0xFFFFFFFF)
    u[:, 1::2] = h >> np.uint64(32)
    c = np.zeros((n, L), dtype=np.int64)
    for t in table:
        c += u >= np.uint64(int(t))
    return c


def soft(line, key, first, table, L):
    """line uint32 [n, L / 32] -> (llr4 uint8 [n, L / 2], flips uint32 [n], total)"""
    n = line.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(line).view(np.uint8).reshape(n, -1), axis=1, bitorder="little").astype(np.int64)
    m = counts(key, first, n, L, table) - 7
    level = np.where(bits == 1, m, -m)
    nib = (level & 15).astype(np.uint8)
    out = nib[:, 0::2] | (nib[:, 1::2] << np.uint8(4))
    flips = ((level > 0) != (bits == 1)).sum(axis=1).astype(np.uint32)
    return np.ascontiguousarray(out), flips, int(flips.sum())


def levels(llr4):
    """uint8 [n, L / 2] -> int64 [n, L] in -8 .. 7"""
    n = llr4.shape[0]
    nib = np.empty((n, 2 * llr4.shape[1]), dtype=np.int64)
    nib[:, 0::2] = llr4 & 15
    nib[:, 1::2] = llr4 >> 4
    return np.where(nib >= 8, nib - 16, nib)


def awgn_table(sigma, scale):
    """the fourteen thresholds from math.erfc: a list of Python ints"""
    table = []
    for j in list(range(-7, 0)) + list(range(1, 8)):
        x = (j / scale - 1.0) / sigma
        table.append(min(math.floor(2.0 ** 32 * 0.5 * math.erfc(-x / math.sqrt(2.0))), 2 ** 32 - 1))
    return table
