"""Random codewords of the built-in 50G-PON code for every decode kernel: the batches, the table of kernel selections and the cached
CPU references of tests/test_codeword_cases_cpu.py and tests/test_gpu_codeword_cases.py (a plain helper, no fixtures).

The decoders are not sign-symmetric (sw_update of csrc/lnsfaid_swar.h clamps with sign-selected constants, the hard decision is
En > 0, zero messages take the sign of En), and on the all-zero codeword a converged frame sits at -31 everywhere: the positive limit,
the "new message not negative" half of every constant pair and decisions of 1 are reached by residual errors only, and a syndrome,
dirty check or flip stage that rotated or packed bits wrongly still finds the all-zero word clean.  Every batch here is built on
96 random messages (numpy's default_rng(1)) encoded with tests/gf2_encoder.py, three groups in the group layout:

    mixed      gf2_encoder.qpsk_llr at MIXED[method]: early-stopping groups, full-length groups and the flip stage side by side
    clean      the same at CLEAN[method]: every group stops early, not all in the same iteration
    staggered  lane l of every group at 3.0 + 0.1 l dB (STAGGERED_SEED): lanes that are clean after two iterations beside lanes
               that never converge - parking and resume at their widest under the per-codeword rule
    minus8     the mixed batch with every -7 replaced by -8
    hard1 / hard4 / hard7   +-magnitude on the codeword, every position flipped with probability 0.01 (default_rng(HARD_SEED)):
               the images LNSFAID_LINE_HARD feeds the decoder; every |LLR| equal makes every first / second minimum a tie
    erasures   noiseless +-7 with 10 % of the positions set to 0; lane ERASED_LANE of every group all 0, lane COMPLEMENT_LANE the
               bitwise complement of its codeword at +-7 (a confident non-codeword)

DecodeMethod 0 (CLDPC::Decode) has no syndrome stage and no early stop: every record is (MAX_ITER, 0), under the group rule and under
the per-codeword rule.  The conditions on iterations below are therefore asked of DecodeMethods 1 .. 5; of DecodeMethod 0 the mixed
batch has wrong and right frames and the clean batch only right ones (its clean batch sits higher for that).
"""
import concurrent.futures

import numpy as np

import early_stop_ref as esr
import gf2_encoder
import line_ref as lr
import oracle_abi as oa

NG = 3          # groups per batch: the least that gives early-stopping groups, full-length groups and a relaunch side by side
FRAMES = NG * 32
MAX_ITER = 10
METHODS = (0, 1, 2, 3, 4, 5)
EARLY_STOP_METHODS = (1, 2, 3, 4, 5)
BF_METHODS = (2, 3, 4, 5)       # DecodeMethods with a bit-flipping stage
SWAR_METHODS = (0, 1, 2, 5)     # what oracle/swar_emul.cpp's host-compiled layer step is compared on
WINDOW_METHODS = (1, 3, 4, 5)   # lnsfaid_cfg_default gives these an error-floor window (floor_iter_thresh >= 0)
MESSAGE_SEED = 1
HARD_SEED = 2
ERASURE_SEED = 3
STAGGERED_SEED = 0
ERASED_LANE, COMPLEMENT_LANE = 5, 9
BATCHES = ("mixed", "clean", "staggered", "minus8", "hard1", "hard4", "hard7", "erasures")
# hard1 is the one batch on which no decoder converges and En does not reach +-31: with every |LLR| equal to 1 the minima of a row
# are 0 or 1, and the messages such minima give are too weak to correct one flip in a hundred (no own iteration count below MAX_ITER
# in any DecodeMethod; En of DecodeMethods 1, 2, 5 was seen to stay within -7 .. 7).  It is kept for what it does reach: ties in
# every minimum search, zero messages on most edges, and decisions that follow the channel.  Normalised min-sum with factor 24 even
# turns a minimum of 1 into (1 * 24) >> 5 = 0: every message is 0 and En keeps the channel's value in every iteration (EN_STAYS).
EN_UNSATURATED = ("hard1",)
EN_STAYS = ((0, "hard1"),)

# DecodeMethod -> (Eb/N0 in dB, seed of gf2_encoder.qpsk_llr).  Found with the CPU port by a sweep over 3.45 .. 3.65 dB in steps of
# 0.05 with seeds 0 .. 2 (mixed) and over 4.0 .. 5.0 dB with seeds 0 and 1 (clean); the comment holds the group records (iterations,
# bf_iterations) and the wrong frames of 96 the sweep saw.  With floor_iter_thresh = -1 (DecodeMethods 1, 3, 4, 5) the sweep saw the
# same records and counts at these points.  tests/test_codeword_cases_cpu.py asserts the conditions of its docstring on every run.
MIXED = {
    0: (3.55, 0),  # [[10, 0], [10, 0], [10, 0]], 5 frames wrong
    1: (3.55, 0),  # [[9, 0], [10, 0], [10, 0]], 2 frames wrong
    2: (3.55, 1),  # [[9, 0], [10, 10], [10, 10]], 4 frames wrong (seed 0: [[10, 0], [10, 10], [10, 10]], no group below MAX_ITER)
    3: (3.55, 0),  # [[9, 0], [10, 0], [10, 50]], 1 frame wrong
    4: (3.55, 0),  # [[9, 0], [10, 0], [10, 50]], 2 frames wrong
    5: (3.55, 0),  # [[8, 0], [10, 0], [10, 10]], 2 frames wrong
}
CLEAN = {
    0: (4.2, 1),  # [[10, 0], [10, 0], [10, 0]], 0 frames wrong
    1: (4.2, 1),  # [[4, 0], [4, 0], [5, 0]]
    2: (4.2, 1),  # [[4, 0], [4, 0], [5, 0]]
    3: (4.2, 1),  # [[4, 0], [4, 0], [5, 0]]
    4: (4.2, 1),  # [[4, 0], [4, 0], [5, 0]]
    5: (4.2, 0),  # [[4, 0], [5, 0], [5, 0]] (seed 1: [[5, 0], [5, 0], [5, 0]])
}
# staggered, STAGGERED_SEED 0: every group runs MAX_ITER iterations and the whole flip stage; under the per-codeword rule the own
# iterations inside a group take the values 2, 3, 4, 5, 7, 8, 10 (group 0 of DecodeMethods 1 .. 4; six to eight values in every group
# of DecodeMethods 1 .. 5)


def cfg_of(abi, lib, method, window="preset"):
    """lnsfaid_cfg_default at MAX_ITER iterations (DecodeMethod 0 with the one factor 24: the four-rows kernel's NMS); window "off":
    floor_iter_thresh = -1, the configuration that takes DecodeMethods 1, 3, 4 and 5 to the window-free kernels"""
    cfg = abi.default_cfg(method, MAX_ITER, lib)
    if method == 0:
        cfg.factor_1 = cfg.factor_2 = 24
    if window == "off":
        cfg.floor_iter_thresh = -1
    else:
        assert window == "preset", window
    return cfg


def windows_of(method):
    """the window settings a DecodeMethod is tested at"""
    return ("preset", "off") if method in WINDOW_METHODS else ("preset",)


_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
        _cache[key] = v
    return _cache[key]


def encoder(code50):
    return _once("encoder", lambda: gf2_encoder.Encoder(code50))


def messages(code50):
    """[FRAMES, K] uint8 0 / 1"""
    return _once("messages", lambda: np.random.default_rng(MESSAGE_SEED).integers(0, 2, (FRAMES, code50.K), dtype=np.uint8))


def codewords(code50):
    """[FRAMES, N] int8 0 / 1: the sent frames, frame-major as the decoders return their decisions"""
    def make():
        cw = encoder(code50).encode(messages(code50))
        assert cw[:, :code50.K].any() and cw[:, code50.K:].any() and not esr.unsatisfied(code50, cw).any()
        return cw
    return _once("codewords", make)


def qpsk_rows(cw, eb_n0, seed, scale=13.0, rate=0.8444444):
    """gf2_encoder.qpsk_llr with an Eb/N0 per frame (eb_n0: [n]): [n, N] int8 frame-major, not yet in the group layout"""
    cw = np.asarray(cw, dtype=np.int8)
    sigma = (1.0 / np.sqrt(rate * 2 * 10.0 ** (0.1 * np.asarray(eb_n0, dtype=np.float64))) / np.sqrt(2.0)).astype(np.float32)
    x = np.random.default_rng(seed).standard_normal(cw.shape, dtype=np.float32) * sigma[:, None]
    x += np.where(cw > 0, np.float32(0.707107), np.float32(-0.707107))
    return np.clip(np.trunc(x * np.float32(scale)), -7, 7).astype(np.int8)


def _hard(cw, magnitude):
    flip = np.random.default_rng(HARD_SEED).random(cw.shape) < 0.01  # the same flips at every magnitude
    return np.where((cw > 0) ^ flip, magnitude, -magnitude).astype(np.int8)


def _erasures(cw):
    f = np.where(cw > 0, 7, -7).astype(np.int8)
    f[np.random.default_rng(ERASURE_SEED).random(cw.shape) < 0.10] = 0
    f[ERASED_LANE::32] = 0
    f[COMPLEMENT_LANE::32] = np.where(cw[COMPLEMENT_LANE::32] > 0, -7, 7)
    return f


def channel(code50, cw, method, name):
    """[FRAMES, N] int8 frame-major: codewords `cw` through the channel of batch `name` (mixed, clean and minus8 depend on the
    method; the noise does not depend on the codewords)"""
    if name in ("mixed", "clean"):
        eb_n0, seed = (MIXED if name == "mixed" else CLEAN)[method]
        return lr.frames_of(gf2_encoder.qpsk_llr(cw, eb_n0, seed), code50.N, code50.K)
    if name == "minus8":
        f = channel(code50, cw, method, "mixed")
        f[f == -7] = -8
        return f
    if name == "staggered":
        return qpsk_rows(cw, 3.0 + 0.1 * (np.arange(FRAMES) % 32), STAGGERED_SEED)
    if name == "erasures":
        return _erasures(cw)
    assert name in ("hard1", "hard4", "hard7"), name
    return _hard(cw, int(name[4]))


def frames(code50, method, name):
    """[FRAMES, N] int8 frame-major: what the channel delivered for batch `name`"""
    return _once(("frames", method if name in ("mixed", "clean", "minus8") else None, name),
                 lambda: channel(code50, codewords(code50), method, name))


def batch(code50, method, name):
    """int8 fixInput of NG groups in the group layout, read-only"""
    return _once(("batch", method, name), lambda: lr.group_layout(np.ascontiguousarray(frames(code50, method, name)), code50.K))


def sent_info(code50):
    """the inputBits of lnsfaid_count_errors: [32][K] int8 0 / 1 per group"""
    return _once("info", lambda: np.ascontiguousarray(messages(code50).astype(np.int8).reshape(-1)))


def reference(abi, lib, code50, method, name, window="preset", kind="avx2", groups=NG):
    """(decodedBits int8 [32 groups * N], records [groups, 2]) under the group rule on the first `groups` groups, computed once per
    process and shared read-only.  kind "avx2": the CPU port, "oracle": the scalar oracle"""
    def make():
        fix = batch(code50, method, name)[:groups * 32 * code50.N]
        return oa.decode_mt(code50, cfg_of(abi, lib, method, window), fix, groups, threads=groups, kind=kind)
    return _once(("ref", method, name, window, kind, groups), make)


def references(abi, lib, code50, todo):
    """reference() of many (method, name[, window[, kind[, groups]]]) side by side (the libraries release the interpreter)"""
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda t: reference(abi, lib, code50, *t), todo))


def codeword_reference_of(abi, lib, code50, method, key, fix, n_groups):
    """(decodedBits [32 n_groups, N], [32 n_groups, 2] iterations / bf_iterations) of every codeword of `fix` (group layout) under the
    per-codeword rule: tests/early_stop_ref.py's 32 copies of a codeword through the CPU port; cached under `key`"""
    def make():
        out, st = esr.per_codeword_oracle(code50, cfg_of(abi, lib, method), fix, n_groups, kind="avx2")
        return np.ascontiguousarray(out), st
    return _once(("cw", method, key), make)


def codeword_reference(abi, lib, code50, method, name):
    return codeword_reference_of(abi, lib, code50, method, name, batch(code50, method, name), NG)


# ---- the line and burst entries ----------------------------------------------------------------------------------------------------
# (batch, format, magnitude): LLR4 for every DecodeMethod, HARD - the signs of the hard batches at their magnitude - for HARD_METHODS
LINE_CASES = (("mixed", lr.LLR4, 0), ("minus8", lr.LLR4, 0), ("staggered", lr.LLR4, 0),
              ("hard1", lr.HARD, 1), ("hard4", lr.HARD, 4), ("hard7", lr.HARD, 7))
HARD_METHODS = (1, 2, 5)
LINE_COUNTS = (FRAMES, 33)  # every codeword, and 33 taken from the front: a last group of one codeword
PUNCTURED = 384             # puncture_tail of the built-in code
# S_c cycles through: nothing, 22.5 block columns, K - 32 (the largest the rule of include/lnsfaid.h allows)
BURST_SHORT = (0, 5760, 14560)


def line_methods(fmt):
    return METHODS if fmt == lr.LLR4 else HARD_METHODS


def line_case(abi, lib, code50, method, name, fmt, magnitude):
    """(line of FRAMES codewords, decodedBits [FRAMES, N], [FRAMES, 2] iterations / bf_iterations): the batch re-laid as a line and
    what the decoder is given for it (tests/line_ref.py's frames_of_line) through the per-codeword rule of the CPU port.  A line of
    the first n codewords is the front of this one, and a codeword's reference does not depend on its neighbours"""
    N, K, L = code50.N, code50.K, code50.N - PUNCTURED
    line = _once(("line", method, name), lambda: lr.line_of(frames(code50, method, name), L, fmt))
    image = lr.group_layout(lr.frames_of_line(line, FRAMES, N, L, fmt, magnitude), K)
    return (line,) + codeword_reference_of(abi, lib, code50, method, ("line", name), image, NG)


def burst_shortened(n=FRAMES):
    return np.array([BURST_SHORT[c % len(BURST_SHORT)] for c in range(n)], dtype=np.uint32)


def burst_case(abi, lib, code50, method, name, fmt, magnitude, where):
    """(frames [FRAMES, N] as received, decodedBits, records) of the burst form: the batch's messages with zeros in every codeword's
    known range, encoded, through the batch's channel; the reference is the per-codeword rule of the CPU port on the image
    tests/burst_ref.py's frames_of_burst gives for the burst line (known range -7, punctured tail 0)"""
    import burst_ref as br
    N, K, L = code50.N, code50.K, code50.N - PUNCTURED
    s = burst_shortened()

    def make():
        cw = encoder(code50).encode(br.zero_known(messages(code50), s, where))
        return channel(code50, cw, method, name)
    rx = _once(("burst", method, name, where), make)
    line = br.burst_line_of(rx, K, L, fmt, s, where)
    image = lr.group_layout(br.frames_of_burst(line, FRAMES, N, K, L, fmt, magnitude, s, where), K)
    return (rx,) + codeword_reference_of(abi, lib, code50, method, ("burst", name, where), image, NG)


def wrong_frames(code50, out):
    """mask [frames]: the decoded frame differs from the sent one"""
    out = np.asarray(out).reshape(-1, code50.N)
    return (out != codewords(code50)[:out.shape[0]]).any(axis=1)


def pack_frames(bits):
    """[n, N] 0 / 1 -> the packed decisions [n, N / 32] uint32, bit b of word w = position 32 w + b"""
    return np.packbits((np.asarray(bits) != 0).astype(np.uint8), axis=1, bitorder="little").view("<u4").astype(np.uint32)


# ---- the kernel selections of the int8 group rule ----------------------------------------------------------------------------------
# name -> the kernel file it stands for.  "on" is lnsfaid_select_zero_shift(LNSFAID_ZERO_SHIFT_ON): on the built-in code it asks for
# what the default picks, so its accessors must repeat the default's.
SELECTIONS = ("default", "edge_off", "windowed", "loop", "on", "rotating", "hbm", "rows2", "waves2")
KERNEL_OF = {"default": "4e, or 4s with a window, or 4 for DecodeMethod 0", "edge_off": "4w", "windowed": "4s", "loop": "4z",
             "on": "as default", "rotating": "4", "hbm": "4, messages through HBM", "rows2": "the two-rows kernel", "waves2": "5"}
# what include/lnsfaid.h refuses: DecodeMethod 0 has no rotation-free, layer-static, register or two-waves instance
REFUSED = {0: ("edge_off", "windowed", "loop", "on", "waves2", "registers")}
# ("registers" is lnsfaid_select_message_store(LNSFAID_MSG_REGISTERS), asserted refused beside "hbm"; no launch of its own elsewhere:
# registers are the default store of DecodeMethods 1 .. 5)


def selection_state(method, window, selection):
    """"run", "refused" (an lnsfaid_select_* call returns LNSFAID_E_INVAL) or "absent": every select call is accepted but the form
    does not apply to the configuration - the window-free kernels with a window that can open - which the accessors must say"""
    if selection in REFUSED.get(method, ()):
        return "refused"
    if selection == "edge_off" and window == "preset" and method in WINDOW_METHODS:
        return "absent"
    return "run"
