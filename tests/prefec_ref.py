"""Helpers of the pre-FEC counter tests (lnsfaid_prefec_errors_*, lnsfaid_frontend_set_prefec): the definition of
include/lnsfaid.h "pre-FEC error counters" restated in numpy on top of demap_ref's levels and de-interleaver, the values the
CPU and GPU tests plant around the decision threshold, and a recount from the bytes the device front-end wrote."""
import numpy as np

import demap_ref as dr

INFO, CODEWORD = 1, 2
FLT_MIN = np.float32(1.17549435e-38)
# what the decision `level > 0` must get right: both zeros and NaN decide 0, +Inf decides 1, the smallest normal floats and
# values far below every quantiser step have their sign
THRESHOLD_VALUES = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, FLT_MIN, -FLT_MIN, 1e-30, -1e-30], dtype=np.float32)


def in_scope(n_var, n_check, interleave, mod_type, scope):
    """(frame, code bit, takes part) of every stream position of a group"""
    m, k = dr.code_bit(np.arange(32 * n_var), n_var, 1 if mod_type == 1 else interleave)
    return m, k, k < (n_var - n_check if scope == INFO else n_var)


def count(rx, n_groups, n_var, n_check, interleave, mod_type, sent, scope):
    """[TestFrame, ModErrorFrame, ModErrorBits, ModErrorSymbol] of received symbols rx against the sent bits (int8, the encoder's
    output layout per group; None = the all-zero codeword)"""
    assert n_var % mod_type == 0 and scope in (INFO, CODEWORD)
    il = 1 if mod_type == 1 else interleave
    levels = dr.stream_levels(rx, n_groups, n_var, mod_type)
    with np.errstate(invalid="ignore"):
        d = (levels > 0).astype(np.int8)  # NaN > 0 is False
    _, _, take = in_scope(n_var, n_check, il, mod_type, scope)
    b = 0 if sent is None else np.asarray(sent, dtype=np.int8).reshape(n_groups, 32 * n_var)[:, dr.destination(n_var, n_check, il)]
    wrong = (d != b) & take
    return counters_of(wrong, n_var, mod_type)


def counters_of(wrong, n_var, mod_type):
    """wrong: bool [n_groups, 32 * n_var] by stream position (frame m holds positions m n_var .. (m + 1) n_var - 1)"""
    n_groups = wrong.shape[0]
    frames = int((wrong.reshape(n_groups, 32, n_var).sum(axis=2) > 0).sum())
    symbols = int(wrong.reshape(n_groups, -1, mod_type).any(axis=2).sum())
    return [32 * n_groups, frames, int(wrong.sum()), symbols]


def sent_of_frames(frames, n_check):
    """frames [n_groups, 32, n_var] bits -> the encoder's output layout: [32][K] then [32][M] per group, int8"""
    frames = np.asarray(frames, dtype=np.int8)
    K = frames.shape[2] - n_check
    return np.concatenate([np.concatenate([fr[:, :K].reshape(-1), fr[:, K:].reshape(-1)]) for fr in frames])


def special_symbols(n_var, n_check, interleave, mod_type):
    """symbols of a group where an addressing mistake would show: the first and the last symbol of frames 0, 1 and 31 and the
    symbols on both sides of their K boundary - by stream position and by code bit"""
    il = 1 if mod_type == 1 else interleave
    K, stride = n_var - n_check, n_var // il
    pos = set()
    for m in (0, 1, 31):
        pos |= {m * n_var, (m + 1) * n_var - 1}
        for k in (K - 1, K):
            pos.add(m * n_var + k)
            pos.add(m * n_var + (k % stride) * il + k // stride)  # the position that carries code bit k
    return sorted({p // mod_type for p in pos})


def plant(rx, n_groups, n_var, n_check, interleave, mod_type):
    """Overwrite, in place, the floats of every special symbol of every group with THRESHOLD_VALUES (rotating, so that each value
    meets each place over the groups and symbols)"""
    per = dr.rx_floats(n_var, mod_type)
    floats = 1 if mod_type == 1 else 2
    j = 0
    for g in range(n_groups):
        for s in special_symbols(n_var, n_check, interleave, mod_type):
            for f in range(floats):
                rx[g * per + floats * s + f] = THRESHOLD_VALUES[j % len(THRESHOLD_VALUES)]
                j += 1
        j += 1  # another phase in the next group
    return rx


def bounds_from_fix_input(fix, n_streams, n_var, n_check, interleave, mod_type, sent, scope):
    """What the bytes a front-end wrote say about its decisions.  A non-zero quantised value has its level's sign (the quantiser
    truncates toward zero, and scale > 0), so it fixes the decision; a zero leaves it open.  Returns (lower, upper) counters:
    lower counts the wrong bits among the non-zero values, upper adds every in-scope zero as wrong."""
    fix = np.asarray(fix, dtype=np.int8).reshape(n_streams, 32 * n_var)
    dest = dr.destination(n_var, n_check, interleave)
    q = fix[:, dest]  # by stream position
    _, _, take = in_scope(n_var, n_check, interleave, mod_type, scope)
    b = 0 if sent is None else np.asarray(sent, dtype=np.int8).reshape(n_streams, 32 * n_var)[:, dest]
    sure = ((q > 0).astype(np.int8) != b) & (q != 0) & take
    maybe = sure | ((q == 0) & take)
    return counters_of(sure, n_var, mod_type), counters_of(maybe, n_var, mod_type)
