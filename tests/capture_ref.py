"""Helpers of the error-frame capture tests (lnsfaid_capture_errors_*): the definition of include/lnsfaid.h "error-frame capture"
restated in numpy, the synthetic batches the CPU and GPU tests share, and the calls with guard bytes around the outputs."""
import ctypes as C

import numpy as np

RECORD = np.dtype([("codeword", np.uint32), ("info_errors", np.uint32), ("parity_errors", np.uint32), ("reserved", np.uint32)])
GUARD = 64  # bytes in front of and behind records and payload
GUARD_BYTE = 0x5A


def frames_of(buf, n_groups, n_var, n_check):
    """[32][K] then [32][M] per group (fixInput, sent) -> [n_groups * 32, n_var] in code-bit order"""
    K = n_var - n_check
    b = np.asarray(buf, dtype=np.int8).reshape(n_groups, 32 * n_var)
    return np.concatenate([b[:, :32 * K].reshape(n_groups, 32, K), b[:, 32 * K:].reshape(n_groups, 32, n_check)], axis=2).reshape(-1, n_var)


def layout_of(frames, n_groups, n_var, n_check):
    """the inverse of frames_of"""
    K = n_var - n_check
    f = np.asarray(frames, dtype=np.int8).reshape(n_groups, 32, n_var)
    return np.ascontiguousarray(np.concatenate([f[:, :, :K].reshape(n_groups, -1), f[:, :, K:].reshape(n_groups, -1)], axis=1).reshape(-1))


def capture(n_var, n_check, fix, decoded, sent, n_groups, skip, capacity):
    """(found, records, payload [stored, 3, n_var], counters the call adds) by the definition"""
    K = n_var - n_check
    n_cw = 32 * n_groups
    zero = np.zeros((n_cw, n_var), dtype=np.int8)
    dec = np.asarray(decoded, dtype=np.int8).reshape(n_cw, n_var)
    snt = zero if sent is None else frames_of(sent, n_groups, n_var, n_check)
    llr = zero if fix is None else frames_of(fix, n_groups, n_var, n_check)
    wrong = dec != snt
    info, parity = wrong[:, :K].sum(axis=1), wrong[:, K:].sum(axis=1)
    order = np.nonzero(info > 0)[0]  # ascending codeword index
    counters = [n_cw, int(order.size), int(info.sum()), int(((info > 0) & (info < 3)).sum())]
    take = order[skip:skip + capacity] if capacity > 0 else order[:0]
    records = np.zeros(take.size, dtype=RECORD)
    records["codeword"], records["info_errors"], records["parity_errors"] = take, info[take], parity[take]
    payload = np.stack([llr[take], dec[take], snt[take]], axis=1).reshape(take.size, 3, n_var)
    return int(order.size), records, payload, counters


def batch(n_var, n_check, n_groups, seed, error_frames, parity_only=(), k_edge=()):
    """(fixInput, decodedBits, sent): random LLRs in [-7, 7], random sent bits, decisions = sent bits with flips planted:
    error_frames: codewords that get 1 + cw % 5 wrong information bits (bit 0, bit K - 1 and random ones in turn) and cw % 3 wrong
    parity bits; parity_only: codewords with wrong parity bits only; k_edge: codewords whose only wrong bits are K - 1 and K"""
    K = n_var - n_check
    rng = np.random.default_rng(seed)
    n_cw = 32 * n_groups
    sent = rng.integers(0, 2, (n_cw, n_var), dtype=np.int8)
    fix = rng.integers(-7, 8, (n_cw, n_var), dtype=np.int8)
    dec = sent.copy()
    for cw in error_frames:
        n = 1 + cw % 5
        bits = {0, K - 1} if n >= 2 else {(0, K - 1, int(rng.integers(0, K)))[cw % 3]}
        while len(bits) < n:
            bits.add(int(rng.integers(0, K)))
        par = [K, n_var - 1][:cw % 3]
        dec[cw, sorted(bits) + par] ^= 1
    for cw in parity_only:
        dec[cw, [K, K + 1, n_var - 1]] ^= 1
    for cw in k_edge:
        dec[cw, [K - 1, K]] ^= 1
    return layout_of(fix, n_groups, n_var, n_check), np.ascontiguousarray(dec.reshape(-1)), layout_of(sent, n_groups, n_var, n_check)


# name -> (error frames, parity-only frames, K-edge frames) at 3 groups (96 codewords)
CASES = {
    "none": ([], [], []),
    "all": (list(range(96)), [], []),
    "group_edges": ([0, 31, 32, 63, 95], [], []),
    "adjacent_pairs": ([0, 1, 31, 32, 62, 63, 64, 94, 95], [], []),
    "parity_only": ([7, 40], [5, 33, 95], []),
    "k_edge": ([12], [], [50]),
    "only_parity_only": ([], [0, 64], []),
}


def guarded_call(fn, n_var, slots, out=None):
    """fn(records pointer, payload pointer, found, stored, out) with guard bytes around both output buffers.  Returns (rc, found,
    stored, records, payload [slots, 3, n_var], counters or None, guards intact); the buffers are pre-filled with GUARD_BYTE, so
    slots the call did not write show it"""
    rec = np.full(2 * GUARD + slots * RECORD.itemsize, GUARD_BYTE, dtype=np.uint8)
    pay = np.full(2 * GUARD + slots * 3 * n_var, GUARD_BYTE, dtype=np.uint8)
    found, stored = C.c_uint64(12345), C.c_uint64(54321)
    counters = None if out is None else (C.c_uint64 * 4)(*[int(x) for x in out])
    rc = fn(rec.ctypes.data + GUARD, pay.ctypes.data + GUARD, C.byref(found), C.byref(stored), counters)
    records = rec[GUARD:GUARD + slots * RECORD.itemsize].view(RECORD)
    payload = pay[GUARD:GUARD + slots * 3 * n_var].view(np.int8).reshape(slots, 3, n_var)
    intact = all((b[:GUARD] == GUARD_BYTE).all() and (b[b.size - GUARD:] == GUARD_BYTE).all() for b in (rec, pay))
    return rc, found.value, stored.value, records, payload, None if counters is None else list(counters), intact


def check_against_ref(fn, n_var, n_check, fix, dec, sent, n_groups, skip, capacity, slots=None, out=(3, 5, 7, 1 << 40)):
    """One guarded call against capture(): records, payload, found, stored, counters (ADDED to `out`), and nothing written beyond
    `stored` slots.  fn(skip, capacity, records, payload, found, stored, out)"""
    slots = min(capacity, 32 * n_groups) if slots is None else slots
    want_found, want_rec, want_pay, want_cnt = capture(n_var, n_check, fix, dec, sent, n_groups, skip, capacity)
    rc, found, stored, rec, pay, cnt, intact = guarded_call(lambda r, p, f, s, o: fn(skip, capacity, r, p, f, s, o), n_var, slots, out)
    assert rc == 0, rc
    assert found == want_found and stored == want_rec.size == min(capacity, max(want_found - skip, 0)), (found, stored, want_found)
    assert rec[:stored].tobytes() == want_rec.tobytes()
    assert pay[:stored].tobytes() == want_pay.tobytes()
    assert intact
    assert (rec[stored:].view(np.uint8) == GUARD_BYTE).all() and (pay[stored:].view(np.uint8) == GUARD_BYTE).all()
    assert cnt == [a + b for a, b in zip(out, want_cnt)], (cnt, want_cnt)
    return found, rec[:stored].copy(), pay[:stored].copy()
