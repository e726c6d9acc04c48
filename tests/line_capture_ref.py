"""numpy restatement of the line-format failure capture (include/lnsfaid.h "line-format failure capture") and the
planted batches its tests share.  H comes straight from pos_vn, deg and deg_rows: nothing of the quasi-cyclic view is used."""
import numpy as np

HARD, LLR4 = 0, 1
UNCORRECTABLE, WRONG = 1, 2
RECORD = np.dtype([("codeword", np.uint64), ("index", np.uint32), ("flags", np.uint32), ("unsatisfied", np.uint32),
                   ("wrong_payload", np.uint32), ("wrong_parity", np.uint32), ("channel_errors", np.uint32)])
KINDS = ("clean", "payload", "parity", "tail", "other", "alarm")


def dims(code):
    return code.n_var, code.n_var - code.n_check, code.n_var - code.puncture_tail


def line_words(code, fmt):
    N, K, L = dims(code)
    return L // 8 if fmt == LLR4 else L // 32


def words(code, fmt):
    return line_words(code, fmt) + 2 * (code.n_var // 32) + code.n_check // 32


def unpack(w):
    """uint32 [n, words] -> uint8 0 / 1 [n, 32 words], bit b of word w at position 32 w + b"""
    w = np.ascontiguousarray(w, dtype="<u4")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], 4 * w.shape[1]), axis=1, bitorder="little")  # (no -1: n may be 0)


def pack(b):
    """the inverse of unpack"""
    return np.packbits(np.ascontiguousarray(b, dtype=np.uint8), axis=1, bitorder="little").view("<u4")


def rows(code):
    """the rows of H: one index array [rows of the class, degree] per degree class, in the table's own row order"""
    pos = np.ctypeslib.as_array(code.pos_vn, shape=(code.n_edges,)).astype(np.int64)
    out, e = [], 0
    for d in range(code.nb_degres):
        deg, cnt = code.deg[d], code.deg_rows[d]
        out.append(pos[e:e + deg * cnt].reshape(cnt, deg))
        e += deg * cnt
    assert e == code.n_edges and sum(r.shape[0] for r in out) == code.n_check
    return out


def syndrome(code, bit):
    """bit uint8 [n, N] -> uint8 [n, M]: 1 where the row of H is unsatisfied"""
    return np.concatenate([bit[:, idx].sum(axis=2) & 1 for idx in rows(code)], axis=1).astype(np.uint8)


def channel_decisions(code, line, fmt):
    """the channel's own decision at the L transmitted positions: the line bit (HARD), nibble > 0 (LLR4)"""
    N, K, L = dims(code)
    if fmt == HARD:
        return unpack(np.ascontiguousarray(line, dtype=np.uint32).reshape(-1, L // 32))
    b = np.ascontiguousarray(line, dtype=np.uint8).reshape(-1, L // 2)
    nib = np.stack([b & 15, b >> 4], axis=2).reshape(b.shape[0], L)
    return ((nib >= 1) & (nib <= 7)).astype(np.uint8)


def capture(code, line, fmt, bits, sent, n, first=0, select=1, skip=0, capacity=256):
    """(found, records, payload uint32 [stored, W]) as lnsfaid_line_capture_host defines them"""
    N, K, L = dims(code)
    lw, W = line_words(code, fmt), words(code, fmt)
    bits = np.ascontiguousarray(bits, dtype=np.uint32).reshape(n, N // 32)
    bit = unpack(bits)
    syn = syndrome(code, bit)
    unsat = syn.sum(axis=1).astype(np.uint32)
    if sent is not None:
        sent = np.ascontiguousarray(sent, dtype=np.uint32).reshape(n, N // 32)
        diff = bit ^ unpack(sent)
        wp, wq = diff[:, :K].sum(axis=1).astype(np.uint32), diff[:, K:].sum(axis=1).astype(np.uint32)
    else:
        wp = wq = np.zeros(n, np.uint32)
    flags = (unsat > 0) * np.uint32(UNCORRECTABLE) | (wp > 0) * np.uint32(WRONG)
    chosen = np.flatnonzero(flags & np.uint32(select))
    kept = chosen[skip:skip + capacity]
    rec = np.zeros(len(kept), RECORD)
    pay = np.zeros((len(kept), W), np.uint32)
    rec["codeword"] = (np.uint64(first % 2 ** 64) + kept.astype(np.uint64))  # wraps
    rec["index"], rec["flags"], rec["unsatisfied"], rec["wrong_payload"], rec["wrong_parity"] = kept, flags[kept], unsat[kept], wp[kept], wq[kept]
    if line is not None:
        img = np.ascontiguousarray(line).reshape(n, -1).view(np.uint8).reshape(n, 4 * lw)
        pay[:, :lw] = np.ascontiguousarray(img[kept]).view("<u4")
        if sent is not None:
            rec["channel_errors"] = (channel_decisions(code, line, fmt)[kept] ^ unpack(sent[kept])[:, :L]).sum(axis=1)
    pay[:, lw:lw + N // 32] = bits[kept]
    if sent is not None:
        pay[:, lw + N // 32:lw + 2 * (N // 32)] = bits[kept] ^ sent[kept]
    pay[:, lw + 2 * (N // 32):] = pack(syn[kept])
    return len(chosen), rec, pay


def planted(abi, lib, code, circ, kinds, fmt, seed, key=0x5EED0F50C0DE2025, first=0):
    """(line, bits, sent) for one codeword per entry of `kinds`:
         clean    the sent word
         payload  a few flipped bits in the payload only      parity  in the transmitted parity only      tail  in the punctured tail only
         other    another valid codeword: unsatisfied 0 and wrong > 0, the undetected case
         alarm    flips in parity and tail that leave the payload right but checks unsatisfied, the false-alarm case
    sent: encode_line_host on payloads of line_payload_random_host.  line: the sent words with planted channel flips (HARD) or levels
    over -8 .. 7 whose sign mostly follows the sent bit (LLR4), level 0 and nibble -8 included."""
    n = len(kinds)
    N, K, L = dims(code)
    rng = np.random.default_rng(seed)
    payload = abi.line_payload_random_host(code, key, first, n + 1, lib)
    _, sent = abi.encode_line_host(code, payload, n + 1, True, lib, circ)
    other, sent = sent[1:], sent[:n]
    bit = unpack(sent)
    spans = {"payload": [(0, K)], "parity": [(K, L)], "tail": [(L, N)], "alarm": [(K, L), (L, N)]}
    for i, kind in enumerate(kinds):
        if kind == "other":
            bit[i] = unpack(other[i:i + 1])[0]
        for lo, hi in spans.get(kind, []):
            at = rng.choice(hi - lo - 2, size=int(rng.integers(0, 5)), replace=False) + lo + 1  # strictly inside the span
            bit[i, at] ^= 1
            bit[i, [lo, hi - 1][i % 2]] ^= 1  # and its first or last position
    bits = pack(bit)
    tx = unpack(sent)[:, :L].copy()
    for i in range(n):
        at = rng.choice(L, size=int(rng.integers(0, 40)), replace=False)
        tx[i, at] ^= 1
    if fmt == HARD:
        return pack(tx), bits, sent
    mag = rng.integers(0, 8, size=(n, L))
    lev = np.where(tx == 1, mag, -mag - (rng.integers(0, 8, size=(n, L)) == 0))  # 0 .. 7 for a 1, -8 .. 0 for a 0
    lev[:, 0], lev[:, 1], lev[:, L - 1] = 0, -8, 7
    nib = (lev & 15).astype(np.uint8)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), bits, sent
