"""Independent numpy restatement of the line-format error-propagation channel (include/lnsfaid.h "line-format error-propagation
channel"): the generator of line_link_ref.py, the BSC's domain, and a walk over the positions one by one (all codewords of the call
side by side), the previous decision choosing the threshold.  Nothing here calls the library."""
import math

import numpy as np

import line_link_ref as ll

LOW = np.uint64(0xFFFFFFFF)


def thresholds(ber, propagation):
    """{ t_idle, t_after, t_start } of the stationary chain, in double in the order the header states"""
    p, a = float(ber), float(propagation)
    if not 0.0 <= p <= a < 1.0:
        raise ValueError((ber, propagation))
    t_after, t_start = int(a * 4294967296.0), int(p * 4294967296.0)
    t_idle = t_start if a == p else min(int(math.floor(4294967296.0 * p * (1.0 - a) / (1.0 - p))), t_after)
    return [t_idle, t_after, t_start]


def error_bits(key, first, n, L, t):
    """uint8 0 / 1 [n, L]: e of every position of codewords first .. first + n - 1"""
    t_idle, t_after, t_start = (np.uint64(int(x)) for x in t)
    assert t_idle <= t_after
    h = ll.draw(key, ll.codeword_numbers(first, n), 2, np.arange(L // 2 + 1))
    u = np.empty((n, L), dtype=np.uint64)
    u[:, 0::2] = h[:, :L // 2] & LOW
    u[:, 1::2] = h[:, :L // 2] >> np.uint64(32)
    e = (h[:, L // 2] & LOW) < t_start  # position -1: the low half of the draw after the BSC's last
    out = np.empty((n, L), dtype=np.uint8)
    for k in range(L):
        e = u[:, k] < np.where(e, t_after, t_idle)
        out[:, k] = e
    return out


def count_runs(e):
    """the maximal runs of ones in each row of a 0 / 1 array; a run at position 0 counts whatever came before the row"""
    e = e.astype(np.int64)
    return (e[:, 0] + ((e[:, 1:] == 1) & (e[:, :-1] == 0)).sum(axis=1)).astype(np.uint32)


def markov(line, key, first, t, L):
    """line uint32 [n, L / 32] -> (line out, flips uint32 [n], runs uint32 [n], total flips, total runs)"""
    n = line.shape[0]
    e = error_bits(key, first, n, L, t)
    mask = np.packbits(e, axis=1, bitorder="little").view(np.uint32).reshape(n, L // 32)
    flips = e.sum(axis=1).astype(np.uint32)
    runs = count_runs(e)
    return line ^ mask, flips, runs, int(flips.sum()), int(runs.sum())


def runs_crossing(e, every, but_not=None):
    """how many runs of the 0 / 1 rows of e cross a position that is a multiple of `every` (both that position and the one before it
    inverted), multiples of `but_not` left out"""
    L = e.shape[1]
    ks = [k for k in range(every, L, every) if but_not is None or k % but_not != 0]
    return int(sum(((e[:, k] == 1) & (e[:, k - 1] == 1)).sum() for k in ks))
