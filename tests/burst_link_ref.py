"""Independent numpy restatement of the burst-format link (include/lnsfaid.h "burst-format link"): every draw is indexed by the mother
position, so each function computes the line link's quantity for whole mother codewords (line_link_ref.draw, line_soft_ref) and keeps
the positions outside the known range (burst_ref.kept).  Nothing here calls the library."""
import numpy as np

import burst_ref as br
import line_link_ref as ll
import line_soft_ref as ls

TAIL, HEAD = br.TAIL, br.HEAD


def kept_words(X, K, S, where):
    """mask over the X / 32 words of a mother codeword (X = K or L): False for the known words"""
    return br.kept(X, K, S, where)[::32]


def payload(key, first, shortened, where, K):
    """flat uint32: the line payload of every codeword without its known words"""
    full = ll.payload(key, first, len(shortened), K)
    return np.concatenate([full[c, kept_words(K, K, S, where)] for c, S in enumerate(shortened)]).astype(np.uint32)


def split(flat, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(flat[at:at + s])
        at += s
    assert at == flat.size
    return out


def bits_of(line, shortened, L):
    """flat uint32 burst line -> list of 0 / 1 arrays, one per codeword, L - S_c long"""
    bits = np.unpackbits(np.ascontiguousarray(line).view(np.uint8), bitorder="little")
    return split(bits, [L - int(S) for S in shortened])


def bsc(line, shortened, where, key, first, threshold, K, L):
    """flat uint32 burst line -> (burst line out, flips per codeword uint32, total)"""
    n = len(shortened)
    f = ll.flip_bits(key, first, n, L, threshold)
    out, flips = [], np.zeros(n, np.uint32)
    for c, (S, b) in enumerate(zip(shortened, bits_of(line, shortened, L))):
        m = br.kept(L, K, S, where)
        out.append(b ^ f[c, m])
        flips[c] = f[c, m].sum()
    return br.pack_words(np.concatenate(out)), flips, int(flips.sum())


def soft(line, shortened, where, key, first, table, K, L):
    """flat uint32 burst line -> (flat uint8 LLR4 burst line, flips per codeword uint32, total)"""
    n = len(shortened)
    m7 = ls.counts(key, first, n, L, table) - 7
    out, flips = [], np.zeros(n, np.uint32)
    for c, (S, b) in enumerate(zip(shortened, bits_of(line, shortened, L))):
        m = m7[c, br.kept(L, K, S, where)]
        level = np.where(b == 1, m, -m)
        nib = (level & 15).astype(np.uint8)
        out.append(nib[0::2] | (nib[1::2] << np.uint8(4)))
        flips[c] = ((level > 0) != (b == 1)).sum()
    return np.concatenate(out), flips, int(flips.sum())


def count(got, sent, stats, short_ones, shortened, K):
    """(errors, fec, vs_sent) as lists of four; fec and vs_sent None without stats.  got / sent flat uint32 burst payloads;
    failed = unsatisfied > 0 or short_ones > 0"""
    sizes = [(K - int(S)) // 32 for S in shortened]
    g = split(np.asarray(got), sizes)
    s = split(np.asarray(sent), sizes) if sent is not None else None
    errors, fec, vs = [0] * 4, [0] * 4, [0] * 4
    for i in range(len(shortened)):
        x = g[i] ^ s[i] if s is not None else g[i]
        w = int(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum())
        errors[0] += 1
        errors[1] += w > 0
        errors[2] += w
        errors[3] += w in (1, 2)
        if stats is not None:
            unsat, corr = int(stats["unsatisfied"][i]), int(stats["corrected"][i])
            failed = unsat > 0 or (short_ones is not None and int(short_ones[i]) > 0)
            fec[0] += 1
            fec[1] += failed
            fec[2] += (not failed) and corr > 0
            fec[3] += 0 if failed else corr
            vs[0] += 1
            vs[1] += w > 0
            vs[2] += w > 0 and not failed
            vs[3] += w == 0 and failed
    return errors, (fec if stats is not None else None), (vs if stats is not None else None)


def planted(shortened, K, seed, stats_dtype):
    """line_link_ref.planted on burst payloads: sent random, got = sent with 0, 1, 2, 3 and many wrong bits planted in turn (in the
    codeword's first or last transmitted word), stats as there (period 4), and short_ones of period 3 (0, 0, 2), so that over 60
    codewords every pairing occurs - among them unsatisfied == 0 with short_ones > 0, right and wrong payloads."""
    n = len(shortened)
    rng = np.random.default_rng(seed)
    sizes = [(K - int(S)) // 32 for S in shortened]
    sent = rng.integers(0, 2 ** 32, size=sum(sizes), dtype=np.uint64).astype(np.uint32)
    got = sent.copy()
    plans = [0, 1, 2, 3, 40]
    at = 0
    for i, kw in enumerate(sizes):
        w = plans[i % 5] if i != n - 1 else 3
        if kw < 3:
            w = min(w, 20)
        word = at if (i // 5) % 2 == 0 else at + kw - 1
        for b in rng.choice(32, size=min(w, 32), replace=False):
            got[word] ^= np.uint32(1) << np.uint32(b)
        if w > 32:
            got[at + kw // 2] ^= np.uint32((1 << (w - 32)) - 1)
        at += kw
    stats = np.zeros(n, dtype=stats_dtype)
    stats["iterations"] = 3
    stats["unsatisfied"] = [(0, 7, 0, 2)[i % 4] for i in range(n)]
    stats["corrected"] = [(0, 0, 5, 9)[i % 4] for i in range(n)]
    ones = np.array([(0, 0, 2)[i % 3] for i in range(n)], dtype=np.uint32)
    return got, sent, stats, ones


def expand_line(line, shortened, where, K, L, fill):
    """flat uint32 burst line -> uint32 [n, L / 32] mother lines with `fill` in the known words"""
    out = np.full((len(shortened), L // 32), fill, dtype=np.uint32)
    for c, (S, w) in enumerate(zip(shortened, split(np.asarray(line), [(L - int(S)) // 32 for S in shortened]))):
        out[c, kept_words(L, K, S, where)] = w
    return out


def drop_words(full, shortened, where, K, X, per_word=1):
    """[n, per_word * X / 32] mother rows -> flat: the known words' elements dropped (per_word = 16 for LLR4 bytes)"""
    return np.concatenate([full[c, np.repeat(kept_words(X, K, S, where), per_word)] for c, S in enumerate(shortened)])


def sim_shortened(first, n, burst_length, shorten):
    """the driver's rule: the last codeword of burst j is shortened by shorten[j % len], all others by 0; a function of the global
    codeword number alone"""
    out = np.zeros(n, np.uint32)
    for i in range(n):
        g = first + i
        if g % burst_length == burst_length - 1:
            out[i] = shorten[(g // burst_length) % len(shorten)]
    return out
