"""Test-side restatements for the device encoder (include/lnsfaid.h: lnsfaid_code_parity_inverse, lnsfaid_encode*,
lnsfaid_frontend_random_frames): the message generator in numpy, the unpacking of the compact B^-1, GF(2) rank and
syndrome helpers, and the derived quasi-cyclic codes of test_gpu_more.py."""
import ctypes as C

import numpy as np

GOLDEN_GAMMA = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def mix64_int(x):
    """splitmix64 finaliser on a Python int (the header's definition, one value at a time)."""
    x &= MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def mix64(x):
    """the same on a numpy uint64 array (multiplication wraps modulo 2^64)"""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def message_words(key, K):
    """the 32-bit word of every information position j < K of one stream: bit l = frame l's bit j"""
    hk = mix64(np.uint64(key & MASK64))
    j = np.arange(1, K + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(hk + j * np.uint64(GOLDEN_GAMMA))
    return (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def messages(keys, K):
    """[n_streams, 32, K] int8 information bits of lnsfaid_frontend_random_frames"""
    out = np.empty((len(keys), 32, K), dtype=np.int8)
    for s, key in enumerate(keys):
        w = message_words(int(key), K)
        out[s] = ((w[None, :] >> np.arange(32, dtype=np.uint32)[:, None]) & 1).astype(np.int8)
    return out


def unpack_parity_inverse(circ, mb, z=256):
    """compact B^-1 (first row of every z x z block) -> the full [mb z, mb z] matrix of 0/1"""
    first = np.unpackbits(np.asarray(circ, dtype=np.uint8).reshape(mb, mb, z // 8), axis=2, bitorder="little")  # [a, b, c]
    t = np.arange(z)
    cols = (t[None, :] - t[:, None]) % z  # entry (t, c) of a block = first row at (c - t) mod z
    full = first[:, :, cols]  # [a, b, t, c]
    return np.ascontiguousarray(full.transpose(0, 2, 1, 3).reshape(mb * z, mb * z))


def parity_matrix(code):
    """H as a dense [M, N] uint8 matrix"""
    N, M = code.code.n_var, code.code.n_check
    pos = np.ctypeslib.as_array(code.pos_vn, shape=(code.code.n_edges,)).astype(np.int64)
    deg = [code.deg[i] for i in range(code.code.nb_degres)]
    rows = [code.deg_rows[i] for i in range(code.code.nb_degres)]
    row_deg = np.repeat(np.array(deg), np.array(rows))
    H = np.zeros((M, N), dtype=np.uint8)
    H[np.repeat(np.arange(M), row_deg), pos] = 1
    return H


def gf2_rank(mat):
    """rank over GF(2) of a 0/1 matrix (bit-packed elimination)"""
    packed = np.packbits(np.asarray(mat, dtype=np.uint8), axis=1)
    rank, n_rows = 0, packed.shape[0]
    for col in range(mat.shape[1]):
        byte, bit = col >> 3, 7 - (col & 7)
        piv = np.nonzero((packed[rank:, byte] >> bit) & 1)[0]
        if piv.size == 0:
            continue
        p = rank + int(piv[0])
        if p != rank:
            packed[[rank, p]] = packed[[p, rank]]
        mask = ((packed[:, byte] >> bit) & 1).astype(bool)
        mask[rank] = False
        packed[mask] ^= packed[rank]
        rank += 1
        if rank == n_rows:
            break
    return rank


def syndromes(H, codewords):
    """H c over GF(2) for frame-major codewords [n, N]: [n, M] (float32 products are exact below 2^24)"""
    return (np.rint(np.asarray(codewords, dtype=np.float32) @ H.T.astype(np.float32)).astype(np.int64) & 1)


def frames_of_group(group, K, M):
    """one group in the encoder output layout ([32][K] then [32][M]) -> [32, N] frame-major"""
    g = np.asarray(group).reshape(-1)
    return np.concatenate([g[:32 * K].reshape(32, K), g[32 * K:].reshape(32, M)], axis=1)


def derived_code(abi, lib, drop_cols, from_block_row, keep_edges=None):
    """A second quasi-cyclic code (the helper _derived_code of test_gpu_more.py): the 50G-PON table with the circulants of the
    block columns `drop_cols` removed from block rows >= from_block_row (degree 23 -> 23 - len(drop_cols)); `keep_edges`
    {block row: n} keeps only the first n circulants of a block row."""
    base = abi.Code50GPON(lib)
    pos = np.ctypeslib.as_array(base.pos_vn)
    out, e = [], 0
    degs = []
    for r in range(3072):
        d = 22 if 256 <= r < 512 else 23
        row = pos[e:e + d]
        e += d
        if r // 256 >= from_block_row:
            row = row[~np.isin(row // 256, drop_cols)]
        if keep_edges and r // 256 in keep_edges:
            row = row[:keep_edges[r // 256]]
        out.append(row)
        degs.append(len(row))
    classes, rows = [], []
    for d in degs:
        if classes and classes[-1] == d:
            rows[-1] += 1
        else:
            classes.append(d)
            rows.append(1)
    flat = np.concatenate(out).astype(np.uint16)

    class Derived:
        pass
    dc = Derived()
    dc.pos_vn = (C.c_uint16 * flat.size)(*flat.tolist())
    dc.deg = (C.c_int32 * len(classes))(*classes)
    dc.deg_rows = (C.c_int32 * len(rows))(*rows)
    dc.code = abi.Code()
    dc.code.n_var, dc.code.n_check, dc.code.n_edges, dc.code.z = 17664, 3072, int(flat.size), 256
    dc.code.puncture_tail, dc.code.nb_degres = 384, len(classes)
    dc.code.deg, dc.code.deg_rows, dc.code.pos_vn = dc.deg, dc.deg_rows, dc.pos_vn
    dc.N, dc.M, dc.K = 17664, 3072, 17664 - 3072
    return dc
