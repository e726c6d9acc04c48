"""Helpers of the FEC status tests (lnsfaid_fec_status_*): the definition of include/lnsfaid.h "FEC status" restated in numpy from
pos_vn, row by row and with no quasi-cyclic shortcut, and the inputs the CPU and GPU tests share."""
import os

import numpy as np

import capture_ref as cr

RECORD = np.dtype([("unsatisfied", np.uint32), ("corrected", np.uint32)])
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tables(code):
    """(pos_vn, row index of every edge) of a Code struct"""
    deg = np.array([code.deg[i] for i in range(code.nb_degres)], dtype=np.int64)
    rows = np.array([code.deg_rows[i] for i in range(code.nb_degres)], dtype=np.int64)
    pos = np.ctypeslib.as_array(code.pos_vn, shape=(code.n_edges,)).astype(np.int64)
    return pos, np.repeat(np.arange(code.n_check), np.repeat(deg, rows))


def unsatisfied(code, bits):
    """bits [n, n_var] 0 / 1 -> checks with an odd number of ones among their variable nodes, per row of bits"""
    pos, row_of = tables(code)
    first_edge = np.nonzero(np.diff(row_of, prepend=-1))[0]  # every row has at least one edge
    assert first_edge.size == code.n_check
    out = np.zeros(bits.shape[0], dtype=np.int64)
    for i in range(0, bits.shape[0], 64):  # the sum of every row's bits, 64 codewords at a time
        ones = np.add.reduceat(bits[i:i + 64][:, pos].astype(np.int32), first_edge, axis=1)
        out[i:i + 64] = (ones & 1).sum(axis=1)
    return out


def status(code, fix, decoded, sent, n_groups, with_sent=False):
    """(records, out, vs_sent or None) by the definition.  fix / sent: int8 in the group layout or None; decoded: int8
    [n_groups * 32 * n_var]; with_sent: vs_sent is asked for (sent None: the all-zero codeword)"""
    N, M = code.n_var, code.n_check
    K, n_cw = N - M, 32 * n_groups
    dec = np.asarray(decoded, dtype=np.int8).reshape(n_cw, N)
    bits = (dec != 0).astype(np.int8)
    rec = np.zeros(n_cw, dtype=RECORD)
    rec["unsatisfied"] = unsatisfied(code, bits)
    if fix is not None:
        channel = (cr.frames_of(fix, n_groups, N, M) > 0).astype(np.int8)
        rec["corrected"] = (bits != channel)[:, :N - code.puncture_tail].sum(axis=1)
    ok = rec["unsatisfied"] == 0
    out = [n_cw, int((~ok).sum()), int((ok & (rec["corrected"] > 0)).sum()), int(rec["corrected"][ok].sum())]
    vs = None
    if with_sent:
        snt = np.zeros((n_cw, N), dtype=np.int8) if sent is None else cr.frames_of(sent, n_groups, N, M)
        wrong = (dec[:, :K] != snt[:, :K]).any(axis=1)
        vs = [n_cw, int(wrong.sum()), int((wrong & ok).sum()), int((~wrong & ~ok).sum())]
    return rec, out, vs


def golden_codeword(n_var):
    return np.unpackbits(np.fromfile(os.path.join(GOLD, "codeword_50gpon.bin"), dtype=np.uint8))[:n_var].astype(np.int8)


def golden_group(name, n_var):
    """(npz, fixInput, decodedBits) of a golden group of tests/golden"""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    fix = np.empty(z["fix_packed"].size * 2, dtype=np.int8)
    fix[0::2] = (z["fix_packed"] & 15).astype(np.int8) - 8
    fix[1::2] = (z["fix_packed"] >> 4).astype(np.int8) - 8
    return z, fix, np.unpackbits(z["decoded_packed"])[:32 * n_var].astype(np.int8)


def pair_rows(code):
    """rows 256 br + {0, 37, 255} of every layer"""
    return [256 * br + i for br in range(code.n_check // 256) for i in (0, 37, 255)]


def planted_pairs(code, codeword):
    """[n, n_var] decisions: the codeword with two adjacent variable nodes of one check flipped - for every row of pair_rows and
    every adjacent pair of the row's nodes, one codeword per pair.  The two nodes share that check, so a wrong rotation of either
    circulant changes the count, which a single flip (always the column's weight) cannot show."""
    pos, row_of = tables(code)
    out = []
    for r in pair_rows(code):
        vn = pos[row_of == r]
        for a, b in zip(vn[:-1], vn[1:]):
            w = codeword.copy()
            w[[a, b]] ^= 1
            out.append(w)
    return np.array(out, dtype=np.int8)


def pair_batch(code, seed, n_groups):
    """(fixInput, decodedBits, sent) of n_groups groups: the planted pairs on the golden codeword, then random decision bytes (a dense
    syndrome) up to n_groups groups; LLRs random over -8 .. 7; sent = the codeword in every frame"""
    N, M = code.n_var, code.n_check
    rng = np.random.default_rng(seed)
    cw = golden_codeword(N)
    pairs = planted_pairs(code, cw)
    n_cw = 32 * n_groups
    assert pairs.shape[0] <= n_cw, pairs.shape
    dec = np.concatenate([pairs, rng.integers(0, 2, (n_cw - pairs.shape[0], N), dtype=np.int8)])
    fix = rng.integers(-8, 8, (n_cw, N), dtype=np.int8)
    sent = np.tile(cw, (n_cw, 1))
    return cr.layout_of(fix, n_groups, N, M), np.ascontiguousarray(dec.reshape(-1)), cr.layout_of(sent, n_groups, N, M)


def random_batch(code, seed, n_groups, dirty=0.5):
    """(fixInput over -8 .. 7, decodedBits, sent) for the built-in code: every sent frame is the golden codeword or the all-zero one;
    a fraction `dirty` of the frames random decision bytes (any value: the bit is `!= 0`), the others their sent frame, half of
    those with one wrong information bit"""
    N, M = code.n_var, code.n_check
    rng = np.random.default_rng(seed)
    n_cw = 32 * n_groups
    sent = golden_codeword(N)[None, :] * rng.integers(0, 2, (n_cw, 1), dtype=np.int8)
    dec = sent.copy()
    for c in range(n_cw):
        if rng.random() < dirty:
            dec[c] = rng.integers(-128, 128, N, dtype=np.int8) * rng.integers(0, 2, N, dtype=np.int8)
        elif c % 2:
            dec[c, int(rng.integers(0, N - M))] ^= 1
    fix = rng.integers(-8, 8, (n_cw, N), dtype=np.int8)
    return cr.layout_of(fix, n_groups, N, M), np.ascontiguousarray(dec.reshape(-1)), cr.layout_of(sent, n_groups, N, M)


def pack_decisions(decoded):
    """int8 decisions -> the packed form's words: bit b of word w is decision 32 w + b != 0"""
    return np.packbits((np.asarray(decoded) != 0).astype(np.uint8), bitorder="little").view(np.uint32)
