"""The error-floor window off its presets: batches, case table and cached references for tests/test_floor_window_cpu.py and
tests/test_gpu_floor_window.py (a plain helper, no fixtures).

The rule under test, per codeword and layered iteration (rem = iterations still to run after this one):
    window = rem <= floor_iter_thresh
    lme    = min(unsat, 255) < (uint8_t)floor_err_count      DecodeMethods 1, 3, 4 (selective offset inside the window)
    lme    = min(unsat, 127) < (int8_t)floor_err_count       DecodeMethod 5, DecodeMethod 2 with EF_ELIMINATION 1 / 2 (_ef tables, erasure)
The presets - (4, 100) for DecodeMethods 1, 3, 4, (6, 50) for 5, (6, 100) and (6, 20) for EF_ELIMINATION 1 and 2 - barely show on
the channel batches of the other tests; here every case is chosen so that a kernel which ignored lme, tested `<=` for `<`,
applied the wrong cast or opened the window one iteration off returns something else than the reference.

Batches, 4 groups (128 frames) each:
    channel     ReferenceChannel(code50, 1901, 13.0).groups(3.5, 4): most frames fail, every iteration runs
    near_clean  nearly clean frames with a few confident errors, default_rng(71)

Families (name: DecodeMethod, EF_ELIMINATION, top = the largest count the family's cast leaves unchanged):
    m1: 1, -, 255   m3: 3, -, 255   m4: 4, -, 255   m5: 5, preset, 127   m2ef1: 2, 1, 127   m2ef2: 2, 2, 127

Cases per family (all from lnsfaid_cfg_default, only the two integers and max_iteration changed) with the measured sensitivity:
frames of 128 whose decisions differ in the scalar oracle's results, "r" where a group record (iterations, bf_iterations)
differs too.  tests/test_floor_window_cpu.py asserts the conditions in the right-hand column on every run.

                                                            m1    m3    m4    m5  m2ef1 m2ef2   condition
count cast, channel, 6 iterations, threshold 6, against the same case with threshold -1 ("off"):
    count top                                               84    26    68    39    18    17    >= 8 or r
    count top + 1     (uint8_t)256 == 0, (int8_t)128 < 0     0     0     0     0     0     0    equal: nothing is below it
    count -1          255 as uint8_t, negative as int8_t    84    26    68     0     0     0    >= 8 or r; equal for the FAID family
    count WRAP        300 / 500 / 500 / 356 / 356 / 356      9    22    65    28    16    15    >= 8 or r; equals count WRAP - 256
                      (300 -> 44 shows in 0 / 4 / 7 / 1 / 1 frames of m3 / m4 / m5 / m2ef1 / m2ef2: swapped for 244 and 100)
    top against top + 1                                     84    26    68    39    18    17    >= 16
    -1 against top                                           0     0     0     -     -     -    equal (OMS family)
`<` boundary, channel, 6 iterations, threshold 6, count c against c + 1 (BOUNDARY, found by scanning c downwards from top):
    (251, 252) / (251, 252) / (251, 252) / (125, 126) / (126, 127) / (126, 127)
                                                             2     1     2     1     1     1    >= 1
window position, near_clean, 3 iterations, count top, threshold against the next one:
    -1 against 0                                            17    0r    0r   100    0r    0r    >= 1 or r
    0 against 1                                             48    2r   27r   114   19r    0r    >= 1 or r
    1 against 2                                             82   44r    75   120    80    8r    >= 1 or r
    2 against 3, 2 against 1 << 20                           0     0     0     0     0     0    equal: rem <= 2 covers all three
presets against "off", 6 iterations:
    channel                                                 31     0    19     9    16     0    >= 8 or r, but for m3 and m2ef2
    near_clean                                              5r    1r    3r    0r   15r    0r    >= 8 or r
    (m3 and m2ef2 at their presets on `channel` are measured at 0: INSENSITIVE_PRESETS; their top rows take that place)
"off", threshold -1, both batches at 6 iterations: the twin of the rows above, and the window-free kernel's cases.

Under the per-codeword rule (32 copies of a codeword through the AVX2 port) the neighbours the per-codeword entries are tested
on differ as follows; tests/test_gpu_floor_window.py asserts >= 1 frame or a record:
    top against top + 1                                    84r   26r   48r   15r    7r    7r
    boundary pair (the same counts)                          2    1r    1r    1r    1r    1r
    position thresholds 0 against 1                        48r    2r    8r   89r   11r    0r
"""
import collections
import concurrent.futures
import ctypes as C

import numpy as np

import early_stop_ref as esr
import oracle_abi as oa

NG = 4  # groups per batch: the smallest at which every sensitivity condition below held (do not enlarge)
FRAMES = NG * 32
HUGE = 1 << 20

# name -> (DecodeMethod, EF_ELIMINATION or None for the preset's, top = the largest count the family's cast leaves unchanged)
FAMILIES = collections.OrderedDict([
    ("m1", (1, None, 255)), ("m3", (3, None, 255)), ("m4", (4, None, 255)),
    ("m5", (5, None, 127)), ("m2ef1", (2, 1, 127)), ("m2ef2", (2, 2, 127)),
])
OMS = ("m1", "m3", "m4")

# (c, c + 1) on `channel`, 6 iterations, threshold 6: two counts next to each other whose reference results differ (CPU scan)
BOUNDARY = {"m1": (251, 252), "m3": (251, 252), "m4": (251, 252), "m5": (125, 126), "m2ef1": (126, 127), "m2ef2": (126, 127)}

# `<=` in place of `<` at count c is `<` at count c + 1 (min(unsat, top) <= c is min(unsat, top) < c + 1, and c + 1 <= top passes
# the cast unchanged): a kernel that tests `<=` returns the reference's result of c + 1 for c, which differs from that of c.

# a count above 256 that either cast wraps to a count inside the range: 300 (44) where 44 shows in 8 frames, else the smallest
# round one that does (DecodeMethod 3 needs a count near the top: 500 is 244)
WRAP = {"m1": 300, "m3": 500, "m4": 500, "m5": 356, "m2ef1": 356, "m2ef2": 356}

# counts the cast turns into "never": top + 1 is (uint8_t)256 == 0 or (int8_t)128 < 0, and -1 stays negative as int8_t (as uint8_t it
# is 255, the top).  These cases must EQUAL their window-off twin.
NEVER = {f: ((top + 1,) if f in OMS else (top + 1, -1)) for f, (_, _, top) in FAMILIES.items()}

# presets whose window does not show on `channel` at 6 iterations (0 frames, same records); the family's top row takes their place
INSENSITIVE_PRESETS = (("m3", "channel"), ("m2ef2", "channel"))

Case = collections.namedtuple("Case", "family kind batch max_iter thresh count")  # thresh / count None: the preset's


def case_id(c):
    t = "preset" if c.thresh is None else ("huge" if c.thresh == HUGE else str(c.thresh))
    n = "preset" if c.count is None else str(c.count)
    return "%s-%s-%s-it%d-t%s-c%s" % (c.family, c.kind, c.batch, c.max_iter, t, n)


def family_cases(family):
    top = FAMILIES[family][2]
    lo, hi = BOUNDARY[family]
    cases = [Case(family, "cast", "channel", 6, 6, n) for n in (top, top + 1, -1, WRAP[family])]
    cases += [Case(family, "boundary", "channel", 6, 6, n) for n in (lo, hi)]
    cases += [Case(family, "position", "near_clean", 3, t, top) for t in (-1, 0, 1, 2, 3, HUGE)]
    cases += [Case(family, "preset", b, 6, None, None) for b in ("channel", "near_clean")]
    cases += [Case(family, "off", b, 6, -1, None) for b in ("channel", "near_clean")]
    return cases


def find(family, kind, batch=None, thresh=None, count=None):
    got = [c for c in family_cases(family) if c.kind == kind and batch in (None, c.batch) and thresh in (None, c.thresh)
           and count in (None, c.count)]
    assert len(got) == 1, (family, kind, batch, thresh, count, got)
    return got[0]


def twin(c):
    """the same case with the window configured away"""
    return find(c.family, "off", batch=c.batch) if c.max_iter == 6 else find(c.family, "position", thresh=-1)


def cfg_of(abi, lib, c):
    method, ef, _ = FAMILIES[c.family]
    cfg = abi.default_cfg(method, c.max_iter, lib)
    if ef is not None:
        assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), ef) == 0
    if c.thresh is not None:
        cfg.floor_iter_thresh = c.thresh
    if c.count is not None:
        cfg.floor_err_count = c.count
    assert cfg.max_iteration == c.max_iter
    return cfg


_batches = {}


def batch(code50, name):
    """int8 fixInput of NG groups, read-only"""
    if name not in _batches:
        if name == "channel":
            fix = oa.ReferenceChannel(code50, 1901, 13.0).groups(3.5, NG)
        else:
            # nearly clean frames with a few confident errors (the recipe of test_ef_elimination_variants_of_decode_faid, restated)
            assert name == "near_clean"
            rng = np.random.default_rng(71)
            N, K = code50.N, code50.K
            llr = np.full((NG * 32, N), -3, dtype=np.int16) + rng.integers(-2, 3, size=(NG * 32, N))
            for l in range(NG * 32):
                nf = int(rng.integers(2, 24))
                llr[l, rng.integers(17 * 256, 67 * 256, size=nf)] = rng.integers(3, 8, size=nf)
            llr = np.clip(llr, -7, 7).astype(np.int8).reshape(NG, 32, N)
            fix = np.concatenate([np.concatenate([g[:, :K].reshape(-1), g[:, K:].reshape(-1)]) for g in llr])
        fix = np.ascontiguousarray(fix, dtype=np.int8)
        fix.flags.writeable = False
        _batches[name] = fix
    return _batches[name]


_refs = {}


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _compute(abi, lib, code50, key):
    c, kind, rule = key
    cfg = cfg_of(abi, lib, c)
    fix = batch(code50, c.batch)
    if rule == "group":
        return _frozen(*oa.decode_mt(code50, cfg, fix, NG, threads=NG, kind=kind))
    out, st = esr.per_codeword_oracle(code50, cfg, fix, NG, kind=kind)
    return _frozen(np.ascontiguousarray(out).reshape(-1), st)


def references(abi, lib, code50, cases, kind="oracle", rule="group"):
    """[(decodedBits int8 [FRAMES * N], records)] of `cases`, computed once per process and shared read-only.  rule "group":
    records are the [NG, 2] iterations / bf_iterations of the groups; rule "codeword": every codeword decoded under the
    per-codeword rule, records [FRAMES, 2].  Missing ones are computed side by side (the libraries release the interpreter)."""
    keys = [(c, kind, rule) for c in cases]
    todo = [k for k in dict.fromkeys(keys) if k not in _refs]
    if todo:
        batch(code50, "channel"), batch(code50, "near_clean")
        with concurrent.futures.ThreadPoolExecutor(4 if rule == "group" else 1) as ex:
            for k, r in zip(todo, ex.map(lambda k: _compute(abi, lib, code50, k), todo)):
                _refs[k] = r
    return [_refs[k] for k in keys]


def reference(abi, lib, code50, c, kind="oracle", rule="group"):
    return references(abi, lib, code50, [c], kind, rule)[0]


def differ(a, b):
    """(frames whose decisions differ, the records differ) between two references"""
    frames = int((a[0].reshape(FRAMES, -1) != b[0].reshape(FRAMES, -1)).any(axis=1).sum())
    return frames, not np.array_equal(a[1], b[1])
