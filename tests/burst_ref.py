"""Helpers of the burst-format tests (lnsfaid_decode_burst*, lnsfaid_encode_burst*, lnsfaid_burst_*): the formats of
include/lnsfaid.h "burst-format line calls" restated in numpy on frame-major arrays [n_codewords, n_var], and the batches the tests
use.  Codeword c is shortened by S_c bits; its known range is [k0, k0 + S_c) of the information part, k0 = 0 (HEAD) or K - S_c
(TAIL); a burst line / payload is what is left of every codeword, back to back."""
import numpy as np

import line_ref as lr

HARD, LLR4 = lr.HARD, lr.LLR4
TAIL, HEAD = 0, 1
# in bits: 224 and 288 beside the edge of a block column (256), 5760 = 22.5 block columns, 14560 = K - 32 the maximum; the odd word
# counts put the next codeword off 16-byte alignment
SHORT = (0, 32, 224, 256, 288, 5760, 8288, 14560)


def cycle_batch(n):
    """n codewords cycling through SHORT"""
    return np.array([SHORT[i % len(SHORT)] for i in range(n)], dtype=np.uint32)


def burst_shaped_batch(n=33):
    """S = 0 everywhere except codewords 7, 8 and 32: bursts that end there"""
    s = np.zeros(n, dtype=np.uint32)
    for c, v in ((7, 5760), (8, 288), (32, 14560)):
        if c < n:
            s[c] = v
    return s


def batch(name, n):
    if n == 1:
        return np.array([14560], dtype=np.uint32)
    return cycle_batch(n) if name == "cycle" else burst_shaped_batch(n)


def known_range(K, S, where):
    k0 = 0 if where == HEAD else K - int(S)
    return k0, k0 + int(S)


def kept(X, K, S, where):
    """mask over positions 0 .. X - 1 (X = K, L or N): False inside the known range"""
    k0, k1 = known_range(K, S, where)
    m = np.ones(X, dtype=bool)
    m[k0:k1] = False
    return m


def zero_known(msg, shortened, where):
    """messages [n, K] with zeros in every codeword's known range"""
    msg = msg.copy()
    for c, S in enumerate(shortened):
        k0, k1 = known_range(msg.shape[1], S, where)
        msg[c, k0:k1] = 0
    return msg


def burst_words(n, K, L, shortened):
    s = int(np.asarray(shortened, dtype=np.int64).sum())
    return n * L - s, n * K - s


def pack_words(bits):
    """flat 0 / 1 array, a multiple of 32 long -> uint32 words, bit b of word w = element 32 w + b"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").view("<u4").astype(np.uint32)


def burst_payload_of(msg, shortened, where):
    """[n, K] bits -> the burst payload: every codeword's information bits without the known range, one bit stream"""
    K = msg.shape[1]
    return pack_words(np.concatenate([msg[c, kept(K, K, S, where)] for c, S in enumerate(shortened)]))


def burst_line_of(frames, K, L, fmt, shortened, where):
    """frame-major LLRs [n, N] -> burst line: positions 0 .. L - 1 of every codeword without the known range, back to back"""
    vals = np.concatenate([frames[c, :L][kept(L, K, S, where)] for c, S in enumerate(shortened)])
    if fmt == HARD:
        return pack_words(vals > 0)
    return lr.pack_nibbles(vals)


def frames_of_burst(line, n, N, K, L, fmt, magnitude, shortened, where):
    """what the decoder is given: [n, N] int8, -7 in the known range, 0 in the punctured tail, the line's levels elsewhere"""
    if fmt == HARD:
        bits = np.unpackbits(np.ascontiguousarray(line).view(np.uint8), bitorder="little")
        vals = np.where(bits > 0, magnitude, -magnitude).astype(np.int8)
    else:
        vals = lr.unpack_nibbles(np.ascontiguousarray(line))
    out = np.zeros((n, N), np.int8)
    at = 0
    for c, S in enumerate(shortened):
        m = kept(L, K, S, where)
        out[c, :L][~m] = -7
        out[c, :L][m] = vals[at:at + L - int(S)]
        at += L - int(S)
    assert at == vals.size
    return out


def llr4_of_burst(line, n, N, K, L, fmt, magnitude, shortened, where):
    """lnsfaid_burst_to_llr4 restated: the llr4 group layout of ceil(n / 32) groups, padding codewords all 0"""
    return lr.pack_nibbles(lr.group_layout(lr.pad_to_groups(frames_of_burst(line, n, N, K, L, fmt, magnitude, shortened, where)), K))


def channel_decisions(line, n, N, K, L, fmt, shortened, where):
    """[n, L] 0 / 1: the channel's own decision at every transmitted position (the line bit, nibble > 0); 0 in the known range"""
    f = frames_of_burst(line, n, N, K, L, fmt, 1, shortened, where)[:, :L]
    return (f > 0).astype(np.uint8)


def counts(bits, line, N, K, L, fmt, shortened, where):
    """(corrected, short_ones) per codeword of packed decisions [n, N / 32]: decisions that differ from the channel's at the
    transmitted positions, and ones decided inside the known range"""
    n = bits.shape[0]
    dec = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(n, N // 8), axis=1, bitorder="little")[:, :L]
    ch = channel_decisions(line, n, N, K, L, fmt, shortened, where)
    corrected, ones = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for c, S in enumerate(shortened):
        m = kept(L, K, S, where)
        corrected[c] = (dec[c, m] != ch[c, m]).sum()
        ones[c] = dec[c, ~m].sum()
    return corrected, ones


def payload_of_bits(bits, K, shortened, where):
    """packed decisions [n, N / 32] -> the burst payload: the information words minus the known ones"""
    out = []
    for c, S in enumerate(shortened):
        k0, k1 = known_range(K, S, where)
        out.append(np.concatenate([bits[c, :k0 // 32], bits[c, k1 // 32:K // 32]]))
    return np.concatenate(out).astype(np.uint32)


def planted_burst(encoder, n, L, fmt, seed, shortened, where, p_flip=0.005, eb_n0=3.6):
    """lr.planted_batch for a burst: n random messages with zeros in the known range, encoded.  From 33 codewords on codewords 0
    and 1 are received as sent, 2 and 3 are random bits (HARD) or random nibbles (LLR4), the rest go through the channel - HARD:
    every transmitted position flipped with probability p_flip; LLR4: QPSK + AWGN at eb_n0 and the 4-bit quantiser.  The known
    positions are then dropped.  Returns (burst line, messages [n, K], kind [n], flips per codeword over the transmitted positions,
    codewords [n, N])."""
    import gf2_encoder
    rng = np.random.default_rng(seed)
    N, K = encoder.N, encoder.K
    msg = zero_known(rng.integers(0, 2, (n, K), dtype=np.uint8), shortened, where)
    cw = encoder.encode(msg)
    assert cw[:, :K].any() and cw[:, K:].any()
    kind = np.full(n, 2)
    if n >= 33:
        kind[:2], kind[2:4] = 0, 1
    sent = np.stack([kept(L, K, S, where) for S in shortened])
    flips = np.zeros(n, np.int64)
    if fmt == HARD:
        rx = cw[:, :L].astype(np.uint8).copy()
        noise = (rng.random((n, L)) < p_flip).astype(np.uint8)
        noise[kind != 2] = 0
        noise[~sent] = 0
        rx ^= noise
        flips = noise.sum(axis=1)
        rx[kind == 1] = rng.integers(0, 2, (int((kind == 1).sum()), L), dtype=np.uint8)
        frames = np.where(rx > 0, 1, -1).astype(np.int8)
    else:
        padded = lr.pad_to_groups(cw)
        frames = lr.frames_of(gf2_encoder.qpsk_llr(padded, eb_n0, seed), N, K)[:n, :L].copy()
        frames[kind == 0] = np.where(cw[kind == 0, :L] > 0, 7, -7)
        frames[kind == 1] = rng.integers(-8, 8, (int((kind == 1).sum()), L), dtype=np.int8)
    full = np.zeros((n, N), np.int8)
    full[:, :L] = frames
    return burst_line_of(full, K, L, fmt, shortened, where), msg, kind, flips, cw


def expand_payload(payload, n, K, shortened, where):
    """burst payload -> [n, K] bits with zeros in the known range"""
    bits = np.unpackbits(np.ascontiguousarray(payload).view(np.uint8), bitorder="little")
    out = np.zeros((n, K), np.uint8)
    at = 0
    for c, S in enumerate(shortened):
        m = kept(K, K, S, where)
        out[c, m] = bits[at:at + K - int(S)]
        at += K - int(S)
    assert at == bits.size
    return out


def burst_line_of_codewords(cw, K, L, shortened, where):
    """codewords [n, N] bits -> the burst line in the HARD format"""
    return pack_words(np.concatenate([cw[c, :L][kept(L, K, S, where)] for c, S in enumerate(shortened)]) > 0)
