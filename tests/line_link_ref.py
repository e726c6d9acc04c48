"""Independent numpy restatement of the line-format link (include/lnsfaid.h "line-format link"): the generator in uint64 arithmetic,
the payload source, the binary symmetric channel, and a counter that walks the bits one by one.  Nothing here calls the library."""
import numpy as np

M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
GOLD = np.uint64(0x9E3779B97F4A7C15)
CWMUL = np.uint64(0xD1B54A32D192ED03)
MASK = (1 << 64) - 1


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix64(x):
    """the splitmix64 finaliser, elementwise on uint64 (numpy wraps mod 2^64)"""
    x = _u64(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= M1
        x ^= x >> np.uint64(27)
        x *= M2
        x ^= x >> np.uint64(31)
    return x


def cwkey(key, C, d):
    """key and d Python ints, C an array of global codeword numbers (uint64, already wrapped)"""
    with np.errstate(over="ignore"):
        return mix64(mix64(np.uint64((key + d) & MASK)) + (_u64(C) + np.uint64(1)) * CWMUL)


def draw(key, C, d, q):
    """draw(key, C, d, q) for every codeword of C and every q: uint64 [len(C), len(q)]"""
    with np.errstate(over="ignore"):
        return mix64(cwkey(key, C, d)[:, None] + (_u64(q)[None, :] + np.uint64(1)) * GOLD)


def codeword_numbers(first, n):
    return np.array([(first + i) & MASK for i in range(n)], dtype=np.uint64)


def payload(key, first, n, K):
    """uint32 [n, K / 32]: word 2 q the low half of draw q, word 2 q + 1 the high half; an odd K / 32 drops the last high half"""
    kw = K // 32
    h = draw(key, codeword_numbers(first, n), 1, np.arange((kw + 1) // 2))
    words = np.empty((n, 2 * ((kw + 1) // 2)), dtype=np.uint32)
    words[:, 0::2] = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words[:, 1::2] = (h >> np.uint64(32)).astype(np.uint32)
    return np.ascontiguousarray(words[:, :kw])


def flip_bits(key, first, n, L, threshold):
    """uint8 0 / 1 [n, L]: position 2 q inverted iff the low half of draw q is below threshold, 2 q + 1 iff the high half is"""
    h = draw(key, codeword_numbers(first, n), 2, np.arange(L // 2))
    f = np.empty((n, L), dtype=np.uint8)
    f[:, 0::2] = (h & np.uint64(0xFFFFFFFF)) < np.uint64(threshold)
    f[:, 1::2] = (h >> np.uint64(32)) < np.uint64(threshold)
    return f


def bsc(line, key, first, threshold, L):
    """line uint32 [n, L / 32] -> (line out, flips per codeword uint32 [n], total)"""
    n = line.shape[0]
    f = flip_bits(key, first, n, L, threshold)
    mask = np.packbits(f, axis=1, bitorder="little").view(np.uint32).reshape(n, L // 32)
    flips = f.sum(axis=1).astype(np.uint32)
    return line ^ mask, flips, int(flips.sum())


def count(got, sent, stats, K):
    """bit loop: (errors, fec, vs_sent) as lists of four; fec and vs_sent None without stats.  got / sent uint32 [n, K / 32]"""
    n = got.shape[0]
    errors, fec, vs = [0] * 4, [0] * 4, [0] * 4
    for i in range(n):
        w = 0
        for word in range(K // 32):
            x = int(got[i, word]) ^ (int(sent[i, word]) if sent is not None else 0)
            for b in range(32):
                w += (x >> b) & 1
        errors[0] += 1
        errors[1] += w > 0
        errors[2] += w
        errors[3] += w in (1, 2)
        if stats is not None:
            unsat, corr = int(stats["unsatisfied"][i]), int(stats["corrected"][i])
            fec[0] += 1
            fec[1] += unsat > 0
            fec[2] += unsat == 0 and corr > 0
            fec[3] += corr if unsat == 0 else 0
            vs[0] += 1
            vs[1] += w > 0
            vs[2] += w > 0 and unsat == 0
            vs[3] += w == 0 and unsat > 0
    return errors, (fec if stats is not None else None), (vs if stats is not None else None)


def planted(n, K, seed, stats_dtype):
    """A batch for the counters: sent random, got = sent with 0, 1, 2, 3 and many wrong bits planted in turn - in the first and in the
    last payload word, the last codeword always hit - and stats rows that run through every combination of unsatisfied 0 / > 0 and
    corrected 0 / > 0 against wrong and right payloads."""
    rng = np.random.default_rng(seed)
    kw = K // 32
    sent = rng.integers(0, 2 ** 32, size=(n, kw), dtype=np.uint64).astype(np.uint32)
    got = sent.copy()
    plans = [0, 1, 2, 3, 40 if kw > 2 else 20]  # many: a whole word and more where there is room
    for i in range(n):
        w = plans[i % 5] if i != n - 1 else 3
        word = 0 if (i // 5) % 2 == 0 else kw - 1
        bits = rng.choice(32, size=min(w, 32), replace=False)
        for b in bits:
            got[i, word] ^= np.uint32(1) << np.uint32(b)
        if w > 32:
            got[i, kw // 2] ^= np.uint32((1 << (w - 32)) - 1)
    stats = np.zeros(n, dtype=stats_dtype)
    stats["iterations"] = 3
    # period 4 against the period 5 of the plans: over 20 codewords every pairing occurs
    stats["unsatisfied"] = [(0, 7, 0, 2)[i % 4] for i in range(n)]
    stats["corrected"] = [(0, 0, 5, 9)[i % 4] for i in range(n)]
    return got, sent, stats
