"""Helpers of the line-format tests (lnsfaid_decode_line*, lnsfaid_line_*): the formats of include/lnsfaid.h "line-format decode"
restated in numpy on frame-major arrays [n_codewords, n_var], and the batches the GPU tests decode."""
import numpy as np

HARD, LLR4 = 0, 1
GROUP = 32


def group_layout(frames, K):
    """[n, N] frame-major values, n a multiple of 32 -> flat groups, each [32][K] followed by [32][M]"""
    n, N = frames.shape
    assert n % GROUP == 0
    g = frames.reshape(n // GROUP, GROUP, N)
    return np.ascontiguousarray(np.concatenate([g[:, :, :K].reshape(n // GROUP, -1), g[:, :, K:].reshape(n // GROUP, -1)], axis=1).reshape(-1))


def frames_of(flat, N, K):
    """the inverse of group_layout"""
    g = flat.reshape(-1, GROUP * N)
    return np.ascontiguousarray(np.concatenate([g[:, :GROUP * K].reshape(-1, GROUP, K), g[:, GROUP * K:].reshape(-1, GROUP, N - K)], axis=2)
                                .reshape(-1, N))


def pad_to_groups(frames):
    n, N = frames.shape
    out = np.zeros(((n + GROUP - 1) // GROUP * GROUP, N), dtype=frames.dtype)
    out[:n] = frames
    return out


def pack_nibbles(values):
    """[..., even] int8 in -8 .. 7 -> uint8, element e in byte e // 2, the low nibble when e is even"""
    u = values.astype(np.int16) & 15
    return (u[..., 0::2] | (u[..., 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(b):
    out = np.empty(b.shape[:-1] + (2 * b.shape[-1],), np.int16)
    out[..., 0::2], out[..., 1::2] = b & 15, b >> 4
    return np.where(out >= 8, out - 16, out).astype(np.int8)


def line_of(frames, L, fmt):
    """frame-major LLRs [n, N] -> line: the first L positions of every codeword, back to back.  HARD: bit b of word w of a codeword
    is (LLR of position 32 w + b) > 0, as uint32 words; LLR4: nibbles, as uint8"""
    if fmt == HARD:
        return np.packbits((frames[:, :L] > 0).astype(np.uint8), axis=1, bitorder="little").reshape(-1).view("<u4").astype(np.uint32)
    return pack_nibbles(frames[:, :L]).reshape(-1)


def frames_of_line(line, n, N, L, fmt, magnitude):
    """what the decoder is given for a line: [n, N] int8, +-magnitude (HARD) or the nibbles (LLR4) below L, 0 in the punctured tail"""
    out = np.zeros((n, N), np.int8)
    if fmt == HARD:
        bits = np.unpackbits(np.ascontiguousarray(line).view(np.uint8).reshape(n, L // 8), axis=1, bitorder="little")
        out[:, :L] = np.where(bits > 0, magnitude, -magnitude)
    else:
        out[:, :L] = unpack_nibbles(line.reshape(n, L // 2))
    return out


def llr4_of_line(line, n, N, K, L, fmt, magnitude):
    """lnsfaid_line_to_llr4 restated: the llr4 group layout of ceil(n / 32) groups, padding codewords all 0"""
    return pack_nibbles(group_layout(pad_to_groups(frames_of_line(line, n, N, L, fmt, magnitude)), K))


def payload_of(messages):
    """[n, K] bits -> [n, K / 32] uint32 words, bit b of word w = bit 32 w + b"""
    return np.packbits(np.asarray(messages, dtype=np.uint8), axis=1, bitorder="little").view("<u4").astype(np.uint32)


def channel_decisions(line, n, L, fmt):
    """[n, L] 0 / 1: the line bit (HARD), nibble > 0 (LLR4)"""
    if fmt == HARD:
        return np.unpackbits(np.ascontiguousarray(line).view(np.uint8).reshape(n, L // 8), axis=1, bitorder="little")
    return (unpack_nibbles(line.reshape(n, L // 2)) > 0).astype(np.uint8)


def planted_batch(encoder, n, L, fmt, seed, p_flip=0.005, eb_n0=3.6):
    """n random encoded codewords as a line.  From 33 codewords on: codewords 0 and 1 received as sent, 2 and 3 random bits
    (HARD) or random nibbles (LLR4), the rest through the channel - HARD: every position below L flipped with probability
    p_flip; LLR4: QPSK + AWGN at eb_n0 and the 4-bit quantiser (gf2_encoder.qpsk_llr).  A batch of fewer codewords goes through
    the channel whole.  Returns (line, messages [n, K], kind [n]: 0 noiseless / 1 random / 2 channel, flips per codeword)."""
    import gf2_encoder
    rng = np.random.default_rng(seed)
    N, K = encoder.N, encoder.K
    msg = rng.integers(0, 2, (n, K), dtype=np.uint8)
    cw = encoder.encode(msg)
    assert cw[:, :K].any() and cw[:, K:].any()
    kind = np.full(n, 2)
    if n >= 33:
        kind[:2], kind[2:4] = 0, 1
    flips = np.zeros(n, np.int64)
    if fmt == HARD:
        rx = cw[:, :L].astype(np.uint8).copy()
        noise = (rng.random((n, L)) < p_flip).astype(np.uint8)
        noise[kind != 2] = 0
        rx ^= noise
        flips = noise.sum(axis=1)
        rx[kind == 1] = rng.integers(0, 2, (int((kind == 1).sum()), L), dtype=np.uint8)
        frames = np.where(rx > 0, 1, -1).astype(np.int8)
    else:
        padded = pad_to_groups(cw)
        frames = frames_of(gf2_encoder.qpsk_llr(padded, eb_n0, seed), N, K)[:n, :L].copy()
        frames[kind == 0] = np.where(cw[kind == 0, :L] > 0, 7, -7)
        frames[kind == 1] = rng.integers(-8, 8, (int((kind == 1).sum()), L), dtype=np.int8)
    full = np.zeros((n, N), np.int8)
    full[:, :L] = frames
    return line_of(full, L, fmt), msg, kind, flips
