"""Host-side references of the per-codeword early stop (lnsfaid_decode_codewords): the parity checks a decision leaves unsatisfied
(numpy H x) and the 32-copy restatement through the unmodified oracle (a codeword under the per-codeword rule decodes as a group of
32 copies of itself, read from lane 0)."""
import ctypes as C

import numpy as np

import oracle_abi as oa


def check_rows(code):
    """(pos_vn, row start offsets) of the Constants_SSE.h table of `code` (a pyabi.Code50GPON or a derived code)"""
    c = code.code
    pos = np.ctypeslib.as_array(C.cast(c.pos_vn, C.POINTER(C.c_uint16)), shape=(c.n_edges,)).astype(np.int64)
    degs = np.concatenate([np.full(c.deg_rows[k], c.deg[k], dtype=np.int64) for k in range(c.nb_degres)])
    assert degs.size == c.n_check and degs.sum() == c.n_edges
    starts = np.concatenate([[0], np.cumsum(degs)[:-1]])
    return pos, starts


def unsatisfied(code, bits, chunk=512):
    """bits: [n, N] 0/1 -> [n] number of parity checks H x leaves unsatisfied"""
    pos, starts = check_rows(code)
    bits = np.asarray(bits).reshape(-1, code.code.n_var)
    out = np.empty(bits.shape[0], dtype=np.int64)
    for i in range(0, bits.shape[0], chunk):
        x = bits[i:i + chunk][:, pos] & 1
        out[i:i + chunk] = (np.bitwise_xor.reduceat(x, starts, axis=1) != 0).sum(axis=1)
    return out


def replicate(code, fix, n_groups, cws=None):
    """fixInput of one group per codeword: row c of the [32][K] block and row c of the [32][M] block, 32 times"""
    N, K, M = code.N, code.K, code.M
    f = np.asarray(fix).reshape(n_groups, 32 * N)
    info = f[:, :32 * K].reshape(n_groups * 32, K)
    par = f[:, 32 * K:].reshape(n_groups * 32, M)
    if cws is not None:
        info, par = info[cws], par[cws]
    n = info.shape[0]
    out = np.empty((n, 32 * N), dtype=np.int8)
    out[:, :32 * K] = np.repeat(info[:, None, :], 32, axis=1).reshape(n, 32 * K)
    out[:, 32 * K:] = np.repeat(par[:, None, :], 32, axis=1).reshape(n, 32 * M)
    return out.reshape(-1)


def per_codeword_oracle(code, cfg, fix, n_groups, kind="avx2", cws=None):
    """(decodedBits [n, N], [n, 2] I / J) of every codeword (or of the codewords `cws`) under the per-codeword rule"""
    rep = replicate(code, fix, n_groups, cws)
    n = rep.size // (32 * code.N)
    if kind == "oracle":
        outs, stats = [], []
        for lo in range(0, n, 64):
            hi = min(n, lo + 64)
            o, s = oa.decode_mt(code, cfg, rep[lo * 32 * code.N:hi * 32 * code.N], hi - lo)
            outs.append(o)
            stats.append(s)
        out, st = np.concatenate(outs), np.concatenate(stats)
    else:
        out, st = oa.decode_mt(code, cfg, rep, n, kind=kind)
    out = out.reshape(n, 32, code.N)
    assert (out == out[:, :1]).all(), "the 32 copies of a codeword decoded differently"
    return out[:, 0], st
