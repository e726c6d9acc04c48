"""Helpers of the demapper tests (lnsfaid_demap_*): (a) the reference's channel restated in Python, which produces the very
symbols the oracle's chain (oracle/frontend_oracle.c) saw between AWGNChannel and Demodulation, (b) the demapper of
include/lnsfaid.h "demapper for received symbols" restated in numpy, (c) a vectorised modulator and the planted values the
CPU and GPU tests share."""
import math

import numpy as np

f32 = np.float32

# CModulate.cpp:4-7 (oracle/frontend_oracle.c:144-148)
TABLES = {
    2: [-0.707107, 0.707107],
    4: [-0.316228, -0.948683, 0.316228, 0.948683],
    6: [-0.462910, -0.154303, -0.771517, -1.08012, 0.462910, 0.154303, 0.771517, 1.08012],
    8: [-0.383482, -0.536875, -0.230089, -0.076696, -0.843661, -0.690268, -0.997054, -1.150447,
        0.383482, 0.536875, 0.230089, 0.076696, 0.843661, 0.690268, 0.997054, 1.150447],
}
FOLD = {2: [], 4: [0.6324555], 6: [0.6172134, 0.3086067], 8: [0.613568, 0.306784, 0.153392]}
# (mod_type, InterleaveModType, scale, Eb/N0, n_var, n_check); the last one drives every LLR through the out-of-range branch
SMALL_CONFIGS = [(2, 1, 13.0, 3.6, 96, 24), (4, 1, 12.5, 8.1, 96, 24), (6, 3, 12.5, 14.0, 96, 24), (8, 8, 40.0, 19.0, 128, 32),
                 (2, 2, 13.0, 3.8, 96, 24), (4, 4, 12.5, 8.6, 96, 24), (8, 1, 1e12, 19.0, 128, 32)]


# ---- (a) the reference's channel -----------------------------------------------------------------------------------
class WichmannHill:
    """CChannel::Random_Uniform / Random_Norm (CChannel.cpp:71-89) with np.float32 scalars and Python's math (the libm the
    oracle calls; numpy's vectorised cos / log may round differently)."""

    def __init__(self, seed):
        self.ix = self.iy = self.iz = int(seed)

    def uniform(self):
        self.ix = self.ix * 249 % 61967
        self.iy = self.iy * 251 % 63443
        self.iz = self.iz * 252 % 63599
        t = f32(f32(f32(self.ix) / f32(61967) + f32(self.iy) / f32(63443)) + f32(self.iz) / f32(63599))
        return f32(t - f32(int(t)))

    def normal(self, sig):
        u1 = float(self.uniform())
        u2 = float(self.uniform())
        return f32(sig * math.cos(2 * 3.1415926535897932384626433832795 * u2) * math.sqrt(-2.0 * math.log(1.0 - u1)))


def code_bit(pos, n_var, interleave):
    """frame and code bit of a stream position (array or scalar)"""
    m, p = pos // n_var, pos % n_var
    return m, (n_var // interleave) * (p % interleave) + p // interleave


def symbol_indices(frames, mod_type, interleave):
    """frames [32, n_var] bits -> (in-phase, quadrature) table index of every symbol of the group (Modulation, CModulate.cpp:216-264)"""
    n_var = frames.shape[1]
    half = mod_type // 2
    m, k = code_bit(np.arange(32 * n_var), n_var, interleave)
    b = frames[m, k].astype(np.int64).reshape(-1, mod_type)
    idx_i = sum(b[:, u] << (half - u // 2 - 1) for u in range(0, mod_type, 2))
    idx_q = sum(b[:, u] << (half - u // 2 - 1) for u in range(1, mod_type, 2))
    return idx_i, idx_q


def reference_channel_symbols(seed, frames, mod_type, interleave, sigma):
    """One group through Modulation + AWGNChannel of the reference: float32 [symbols * 2], real before imaginary.
    sigma: CSimulate::Configure's (a float); the channel gets float(sigma / sqrt 2)."""
    gen = WichmannHill(seed)
    sig = float(f32(float(sigma) / math.sqrt(2)))
    table = [f32(t) for t in TABLES[mod_type]]
    idx_i, idx_q = symbol_indices(np.asarray(frames), mod_type, interleave)
    rx = np.empty(2 * idx_i.size, dtype=np.float32)
    for s in range(idx_i.size):
        rx[2 * s] = f32(gen.normal(sig) + table[idx_i[s]])
        rx[2 * s + 1] = f32(gen.normal(sig) + table[idx_q[s]])
    return rx


# ---- (b) the demapper ----------------------------------------------------------------------------------------------
def quantise(levels, scale):
    """float2LimitChar_4bit: one float multiply, truncation, integer indefinite -> -7, clamp to [-7, 7]"""
    with np.errstate(all="ignore"):
        y = np.asarray(levels, dtype=np.float32) * f32(scale)
        ok = (y > f32(-2147483648.0)) & (y < f32(2147483648.0))
        q = np.where(ok, np.trunc(np.where(ok, y, f32(0))), -2147483648.0)
    return np.clip(q, -7, 7).astype(np.int8)


def stream_levels(rx, n_groups, n_var, mod_type):
    """LLR (before the quantiser) of every stream position: float32 [n_groups, 32 * n_var]"""
    rx = np.asarray(rx, dtype=np.float32)
    if mod_type == 1:
        return rx.reshape(n_groups, 32 * n_var)
    sym = rx.reshape(-1, 2)
    lv = np.empty((sym.shape[0], mod_type), dtype=np.float32)
    lv[:, 0], lv[:, 1] = sym[:, 0], sym[:, 1]
    for n in range(1, mod_type // 2):
        c = FOLD[mod_type][n - 1]  # in double, stored as float before it feeds the next level
        lv[:, 2 * n] = (np.abs(lv[:, 2 * n - 2].astype(np.float64)) - c).astype(np.float32)
        lv[:, 2 * n + 1] = (np.abs(lv[:, 2 * n - 1].astype(np.float64)) - c).astype(np.float32)
    return lv.reshape(n_groups, 32 * n_var)


def destination(n_var, n_check, interleave):
    """element of the group's fixInput every stream position goes to"""
    K = n_var - n_check
    m, k = code_bit(np.arange(32 * n_var), n_var, interleave)
    return np.where(k < K, m * K + k, 32 * K + m * n_check + (k - K))


def demap(rx, n_groups, n_var, n_check, interleave, mod_type, scale):
    """int8 fixInput [n_groups * 32 * n_var] of received symbols rx"""
    q = quantise(stream_levels(rx, n_groups, n_var, mod_type), scale)
    out = np.empty_like(q)
    out[:, destination(n_var, n_check, 1 if mod_type == 1 else interleave)] = q
    return out.reshape(-1)


def pack(fix):
    """llr4: element e in byte e / 2, low nibble for even e"""
    u = np.asarray(fix, dtype=np.int8).view(np.uint8) & 15
    return (u[0::2] | (u[1::2] << 4)).astype(np.uint8)


# ---- (c) inputs ----------------------------------------------------------------------------------------------------
def rx_floats(n_var, mod_type):
    """floats of one group"""
    return 32 * n_var if mod_type == 1 else 2 * (32 * n_var // mod_type)


def noisy_symbols(rng, frames, mod_type, interleave, sigma):
    """frames [n_groups, 32, n_var] bits -> constellation points + N(0, (sigma / sqrt 2)^2) per axis, float32 in the rx format"""
    frames = np.asarray(frames)
    out = []
    for fr in frames:
        if mod_type == 1:
            pts = (2.0 * fr.reshape(-1) - 1.0)  # positive means bit 1
        else:
            idx_i, idx_q = symbol_indices(fr, mod_type, interleave)
            t = np.array(TABLES[mod_type])
            pts = np.stack([t[idx_i], t[idx_q]], axis=1).reshape(-1)
        out.append(pts + rng.standard_normal(pts.size) * (sigma / math.sqrt(2)))
    return np.concatenate(out).astype(np.float32)


def special_values(scale):
    """what must end at -7 through the integer indefinite: NaN, both infinities and |y| >= 2^31 of either sign"""
    return np.array([np.nan, np.inf, -np.inf, 3e9 / scale, -3e9 / scale], dtype=np.float32)


def planted_values(scale):
    """every quantiser threshold j / scale (j = -8 .. 8) with its float neighbours on both sides and their negatives, both zeros,
    the smallest denormal and special_values"""
    v = []
    for j in range(-8, 9):
        x = f32(j / scale)
        for y in (x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))):
            v += [y, -y]
    v += [f32(0.0), f32(-0.0), f32(1.4e-45), f32(-1.4e-45)]
    return np.concatenate([np.array(v, dtype=np.float32), special_values(scale)])


def special_positions(n_var, n_check, interleave, frames=(0, 1, 31)):
    """stream positions of a group where an addressing mistake would show: both ends of the group, both sides of the frame
    boundaries of `frames`, and both sides of their K boundary - by stream position and by code bit"""
    K = n_var - n_check
    pos = {0, 32 * n_var - 1}
    stride = n_var // interleave
    for m in frames:
        pos |= {m * n_var, (m + 1) * n_var - 1}
        if m > 0:
            pos.add(m * n_var - 1)
        if m < 31:
            pos.add((m + 1) * n_var)
        for k in (K - 1, K):
            pos.add(m * n_var + k)
            pos.add(m * n_var + (k % stride) * interleave + k // stride)  # the position that carries code bit k
    return sorted(pos)


def plant(rx, n_groups, n_var, n_check, interleave, mod_type, scale, window=8):
    """Overwrite rx in place: around the float of every special position a window of planted values (rotating through the
    list), the whole list once at the very start and once at the very end, special_values on the special positions' own floats."""
    vals = planted_values(scale)
    spec = special_values(scale)
    L, per = len(vals), rx_floats(n_var, mod_type)
    assert rx.size == n_groups * per and 2 * L <= rx.size
    j = 0
    for g in range(n_groups):
        for pos in special_positions(n_var, n_check, 1 if mod_type == 1 else interleave):
            base = pos if mod_type == 1 else 2 * (pos // mod_type)
            for f in range(max(0, base - window // 2), min(per, base + window // 2)):
                rx[g * per + f] = vals[j % L]
                j += 1
    rx[:L] = vals
    rx[rx.size - L:] = vals
    for g in range(n_groups):
        for i, pos in enumerate(special_positions(n_var, n_check, 1 if mod_type == 1 else interleave, frames=(0, 31))):
            base = pos if mod_type == 1 else 2 * (pos // mod_type)
            if L <= g * per + base < rx.size - L:
                rx[g * per + base] = spec[(i + g) % len(spec)]
    return rx
