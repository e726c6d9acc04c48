"""Quasi-cyclic codes of other geometries than the built-in 12 x 69 blocks: a deterministic generator, the table of named shapes with
the property each was chosen for, a QPSK/AWGN synthesiser that takes sigma per component, the (shape, DecodeMethod) batches and the
cached CPU references of tests/test_code_shapes_cpu.py and tests/test_gpu_code_shapes.py (a plain helper, no fixtures).

A shape is described explicitly: block rows, block columns, puncture_tail and, per layer, the list of (block column, shift).  The
descriptions come from `describe`: the information part is realised from a column-weight list and a row-degree list (columns by
descending weight, each into the layers with the most room left, ties and shifts from numpy's default_rng(seed)); the parity part is
lower block-bidiagonal (block row r holds parity block columns r - 1 and r), so it is always invertible.  Rows ascend in block
column, no block column occurs twice in a row, every information column has weight >= 2.

Limits the shapes are placed against (csrc/lnsfaid_device.h, lnsfaid_capi.hip): 32 block rows, 256 block columns, row degree 2 .. 24,
column weight <= 16 (15 for DecodeMethod 3), LDS image <= 0xffff bytes; registers and the cached syndrome walk up to 12 layers; the
bit-flipping stage's cached walk up to 64 block columns of weight W and 14 circulants of them per layer; the two-waves kernel from
448 words (56 block columns) on.
"""
import collections
import concurrent.futures
import ctypes as C

import numpy as np

import early_stop_ref as esr
import gf2_encoder
import oracle_abi as oa

Z = 256
NG = 3          # groups per batch
FRAMES = NG * 32
MAX_ITER = 10   # layered iterations of every configuration of this module
W = 3           # REGULAR_COL_WEIGHT of lnsfaid_cfg_default
METHODS = (0, 1, 2, 3, 4, 5)
BF_METHODS = (2, 3, 4, 5)  # DecodeMethods with a bit-flipping stage

Shape = collections.namedtuple("Shape", "name nbr nbc puncture_tail layers seed")

# name -> (block rows, block columns, puncture_tail, seed, [(column weight, information columns of it)], information edges per layer,
#          {layer: leading edges forced to shift 0})
_RECIPES = collections.OrderedDict([
    # 4 layers (< 12); degrees 23 / 23 / 14 / 7; layer 1 has four zero-shift edges and degree 23, one of the two degrees the
    # rotation-free step is compiled for (23 from one group of four on, 22 from five groups on) - which takes 21 information columns
    # in one layer, hence 4 x 26 blocks and not 4 x 20; 12 weight-3 columns, at most 12 of them in
    # a layer, so the bit-flipping stage's cached walk fits (the one shape of this table with real columns in that arm)
    ("few", (4, 26, 0, 4201, [(4, 2), (3, 12), (2, 8)], [22, 21, 12, 5], {1: 4})),
    # 13 layers: one more than the register instances and the cached syndrome walk take; 20 weight-3 columns, at most 8 per layer
    ("thirteen", (13, 40, 256, 1340, [(6, 4), (4, 3), (3, 20)], [8] * 5 + [7] * 8, {})),
    # 32 layers of degree 3 .. 5; column weights 15, 11, 6, 5, 4, 3, 2 (and the parity part's 2 and 1): all four weight classes
    ("most", (32, 48, 96, 3248, [(15, 1), (11, 2), (6, 3), (5, 1), (4, 2), (3, 6), (2, 1)], [3] * 24 + [2] * 8, {})),
    # N = 27648; layers 1 .. 10 of degree 24; 70 weight-3 columns (> 64).  More than 64 weight-3 columns in 12 layers put more than
    # 14 of their circulants into some layer (65 * 3 / 12 > 16), so bfw_fits is 0 here too: the four-rows kernels take the uncached
    # walk for either reason, and n_wcols alone decides in the two-waves kernel (it does not look at bfw_fits)
    ("wide", (12, 108, 512, 12108, [(3, 70), (2, 26)], [22] * 11 + [20], {})),
    # 40 weight-3 columns (<= 64), 15 of their circulants in every layer (> 14)
    ("crowded", (8, 60, 128, 860, [(3, 40), (2, 12)], [18] * 8, {})),
    # no column of weight 3
    ("noflip", (6, 24, 256, 624, [(4, 9), (2, 9)], [9] * 6, {})),
])
NAMES = tuple(_RECIPES)


def describe(name):
    """the explicit description of a named shape"""
    return realise(name, *_RECIPES[name])


def realise(name, nbr, nbc, tail, seed, weights, row_info, zero_lead=None):
    """a recipe (the format of _RECIPES) -> its explicit description"""
    zero_lead = zero_lead or {}
    kb = nbc - nbr
    colw = [w for w, n in weights for _ in range(n)]
    assert len(colw) == kb and sum(colw) == sum(row_info) and len(row_info) == nbr, name
    rng = np.random.default_rng(seed)
    room = np.array(row_info, dtype=np.int64)
    cols_of = [[] for _ in range(nbr)]
    # spread the weights over the block columns so that no weight sits in one run of neighbouring columns
    place = rng.permutation(kb)
    for w, cb in sorted(zip(colw, place.tolist()), key=lambda t: (-t[0], t[1])):
        order = np.lexsort((rng.random(nbr), -room))  # most room first, ties at random
        take = order[:w]
        assert (room[take] > 0).all(), (name, "the column weights and the layer degrees do not fit")
        room[take] -= 1
        for br in take.tolist():
            cols_of[br].append(cb)
    assert not room.any(), name
    layers = []
    for br in range(nbr):
        cols = sorted(cols_of[br]) + ([kb + br - 1] if br else []) + [kb + br]
        shifts = rng.integers(0, Z, len(cols)).tolist()
        for j in range(zero_lead.get(br, 0)):
            shifts[j] = 0
        layers.append(list(zip(cols, shifts)))
    return Shape(name, nbr, nbc, tail, layers, seed)


class CodeHolder:
    """a pyabi.Code with the buffers it points to kept alive: pos_vn, deg, deg_rows, code, N, M, K (as tests/test_gpu_more.py's
    _derived_code), and the description it was built from"""


def build(shape, abi=None):
    """Shape (or anything with nbr, nbc, puncture_tail, layers) -> CodeHolder.  Nothing is checked here: lnsfaid_create decides"""
    abi = abi or oa.pyabi
    i = np.arange(Z, dtype=np.int64)[:, None]
    rows, classes, counts = [], [], []
    for layer in shape.layers:
        cb = np.array([c for c, _ in layer], dtype=np.int64)[None, :]
        sh = np.array([s for _, s in layer], dtype=np.int64)[None, :]
        rows.append((cb * Z + (sh + i) % Z).reshape(-1))
        if classes and classes[-1] == len(layer):  # consecutive layers of one degree merge into one class
            counts[-1] += Z
        else:
            classes.append(len(layer))
            counts.append(Z)
    flat = np.concatenate(rows).astype(np.uint16) if rows else np.zeros(0, np.uint16)
    h = CodeHolder()
    h.shape = shape
    h.pos_vn = (C.c_uint16 * max(flat.size, 1)).from_buffer_copy(flat.tobytes() if flat.size else b"\0\0")
    h.deg = (C.c_int32 * len(classes))(*classes)
    h.deg_rows = (C.c_int32 * len(counts))(*counts)
    h.code = abi.Code()
    h.N, h.M = shape.nbc * Z, shape.nbr * Z
    h.K = h.N - h.M
    h.code.n_var, h.code.n_check, h.code.n_edges, h.code.z = h.N, h.M, int(flat.size), Z
    h.code.puncture_tail, h.code.nb_degres = shape.puncture_tail, len(classes)
    h.code.deg, h.code.deg_rows, h.code.pos_vn = h.deg, h.deg_rows, h.pos_vn
    return h


def column_weights(shape):
    w = np.zeros(shape.nbc, dtype=np.int64)
    for layer in shape.layers:
        for cb, _ in layer:
            w[cb] += 1
    return w


def weight_class(w):
    """the library's weight classes: 3 / 6 / 11 / every other weight"""
    return {3: 0, 6: 1, 11: 2}.get(int(w), 3)


def lds_bytes(N, M):
    """lf_lds_bytes of csrc/lnsfaid_device.h restated: En, the hard-decision plane, the syndrome words, 40 words of scratch"""
    hard = (N + 15) & ~15
    p = hard + (N // 32) * 4
    stat = (p + (M // 32 + 2) * 4 + 7) & ~7
    return stat + (32 + 8) * 4


def properties(shape, abi=None, lib=None):
    """what the table's property rows are stated in, from the description and the library's host-side queries (no GPU)"""
    abi = abi or oa.pyabi
    h = build(shape, abi)
    colw = column_weights(shape)
    kb = shape.nbc - shape.nbr
    zero_groups, _ = abi.code_zero_shift_order(h.code, lib)
    info = abi.code_bf_walk(h.code, W, lib)[3]
    w_per_layer = [sum(1 for cb, _ in layer if colw[cb] == W) for layer in shape.layers]
    return {
        "layers": shape.nbr, "N": h.N, "M": h.M, "K": h.K,
        "degrees": [len(layer) for layer in shape.layers],
        "column_weights": colw,
        "info_min_weight": int(colw[:kb].min()),
        "zero_groups": zero_groups,
        "bfw_fits": int(info[3]), "n_wcols": int(info[4]),
        "w_per_layer": w_per_layer,
        "classes": sorted({weight_class(w) for w in colw}),
        "lds_bytes": lds_bytes(h.N, h.M),
    }


def check_structure(shape):
    """the generator's own promises"""
    kb = shape.nbc - shape.nbr
    assert len(shape.layers) == shape.nbr
    for br, layer in enumerate(shape.layers):
        cols = [c for c, _ in layer]
        assert cols == sorted(set(cols)), (shape.name, br, "ascending, no block column twice")
        assert all(0 <= c < shape.nbc and 0 <= s < Z for c, s in layer)
        assert [c for c in cols if c >= kb] == ([kb + br - 1] if br else []) + [kb + br], (shape.name, br, "lower bidiagonal parity part")
    assert column_weights(shape)[:kb].min() >= 2, shape.name


def check_properties(name, p):
    """the property row of the table, one shape each: the contract the shapes are kept to"""
    d, colw = p["degrees"], p["column_weights"]
    n3 = int((colw == W).sum())
    assert p["n_wcols"] == n3 and p["info_min_weight"] >= 2 and 2 <= min(d) and max(d) <= 24 and colw.max() <= 16
    if name == "few":
        assert p["layers"] < 12 and min(d) < 8 and max(d) >= 16 and 0 < n3 <= 64 and p["bfw_fits"] == 1
        # a layer the rotation-free step has an instance for (lnsfaid_kernel4z.hip: degree 23 with 1, 2 or 4 groups, 22 with 5)
        assert any((deg == 23 and zg >= 1) or (deg == 22 and zg >= 5) for deg, zg in zip(d, p["zero_groups"]))
    elif name == "thirteen":
        assert p["layers"] == 13 and n3 <= 64 and max(p["w_per_layer"]) <= 14 and p["bfw_fits"] == 1
    elif name == "most":
        assert p["layers"] == 32 and colw.max() == 15 and p["classes"] == [0, 1, 2, 3] and max(d) <= 8
        assert {3, 6, 11} <= set(colw.tolist())
    elif name == "wide":
        assert p["N"] == 27648 and p["layers"] == 12 and max(d) == 24 and n3 > 64
    elif name == "crowded":
        assert p["layers"] <= 12 and n3 <= 64 and max(p["w_per_layer"]) >= 15 and p["bfw_fits"] == 0
    elif name == "noflip":
        assert p["layers"] <= 12 and n3 == 0 and p["bfw_fits"] == 1
    else:
        raise AssertionError(name)


_codes = {}


def code(name, abi=None):
    """the CodeHolder of a named shape, built once per process"""
    if name not in _codes:
        shape = describe(name)
        check_structure(shape)
        _codes[name] = build(shape, abi)
    return _codes[name]


_encoders = {}


def encoder(name):
    """gf2_encoder.Encoder of a named shape (dense Gauss-Jordan on its parity part), built once per process"""
    if name not in _encoders:
        _encoders[name] = gf2_encoder.Encoder(code(name))
    return _encoders[name]


def qpsk_awgn(codewords, sigma, seed, scale=13.0):
    """[n, N] 0 / 1 codewords (n a multiple of 32) through QPSK + AWGN + the 4-bit quantiser, sigma per component given directly
    (oa.synth_llr and gf2_encoder.qpsk_llr fix the 50G-PON rate and parity length): int8 fixInput in the group layout"""
    cw = np.asarray(codewords, dtype=np.int8)
    n, N = cw.shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, N), dtype=np.float32) * np.float32(sigma) + np.where(cw > 0, np.float32(0.707107), np.float32(-0.707107))
    return np.clip(np.trunc(x * np.float32(scale)), -7, 7).astype(np.int8)


def group_layout(frames, K):
    return gf2_encoder.to_group_layout(np.ascontiguousarray(frames), K)


def frames_of(flat, N, K):
    """the inverse of group_layout: [n, N] frame-major"""
    g = np.asarray(flat).reshape(-1, 32 * N)
    return np.ascontiguousarray(np.concatenate([g[:, :32 * K].reshape(-1, 32, K), g[:, 32 * K:].reshape(-1, 32, N - K)], axis=2).reshape(-1, N))


def zero_batch(name, sigma, seed, n_groups=NG):
    """the all-zero codeword form: int8 fixInput of n_groups groups"""
    h = code(name)
    return group_layout(qpsk_awgn(np.zeros((32 * n_groups, h.N), np.int8), sigma, seed), h.K)


def random_batch(name, sigma, seed, n_groups=NG):
    """the random-codeword form: (int8 fixInput, the sent codewords int8 0 / 1 [32 n_groups, N] frame-major, as the decoders return
    their decisions)"""
    h = code(name)
    msg = np.random.default_rng(seed + 1).integers(0, 2, (32 * n_groups, h.K), dtype=np.uint8)
    cw = encoder(name).encode(msg)
    return group_layout(qpsk_awgn(cw, sigma, seed), h.K), cw


# ---- batches -------------------------------------------------------------------------------------------------------------------
# (shape, DecodeMethod) -> ((sigma, seed) of the mixed batch, (sigma, seed) of the clean batch); NG groups each, MAX_ITER layered
# iterations, lnsfaid_cfg_default (DecodeMethod 0 with the one factor 24: the default pair 1 / 6 normalises every message to 0).
#   mixed  random codewords (random_batch): a group stops before MAX_ITER, a group runs every layered iteration, a record has
#          bf_iterations > 0 where the method has a bit-flipping stage, a decoded frame differs from what was sent
#   clean  the all-zero codeword (zero_batch): every group stops early, not all in the same iteration
#   DecodeMethod 0 has no early stop: mixed has wrong and right frames, clean only right ones
# Found with the CPU port by a sweep from high sigma down, seeds 0 .. 5 at each step; the comment holds the records (iterations,
# bf_iterations per group) and the wrong frames of 96 the sweep saw.  tests/test_code_shapes_cpu.py asserts the conditions.
BATCHES = {
    ("few", 0): ((0.35, 0), (0.28, 0)),  # [[10, 0], [10, 0], [10, 0]], 95 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("few", 1): ((0.31, 0), (0.30, 3)),  # [[10, 0], [9, 0], [7, 0]], 3 frames wrong | [[8, 0], [5, 0], [8, 0]], 0 wrong
    ("few", 2): ((0.31, 0), (0.29, 1)),  # [[10, 10], [10, 10], [6, 0]], 3 frames wrong | [[5, 0], [3, 0], [8, 0]], 0 wrong
    ("few", 3): ((0.31, 0), (0.30, 3)),  # [[10, 50], [9, 0], [7, 0]], 3 frames wrong | [[8, 0], [5, 0], [8, 0]], 0 wrong
    ("few", 4): ((0.31, 0), (0.30, 3)),  # [[10, 50], [9, 0], [7, 0]], 3 frames wrong | [[8, 0], [5, 0], [8, 0]], 0 wrong
    ("few", 5): ((0.31, 0), (0.31, 5)),  # [[10, 10], [10, 10], [7, 0]], 4 frames wrong | [[9, 0], [6, 0], [6, 0]], 0 wrong
    ("thirteen", 0): ((0.41, 0), (0.33, 2)),  # [[10, 0], [10, 0], [10, 0]], 79 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("thirteen", 1): ((0.34, 2), (0.33, 0)),  # [[6, 0], [10, 0], [10, 0]], 8 frames wrong | [[8, 0], [6, 0], [6, 0]], 0 wrong
    ("thirteen", 2): ((0.36, 2), (0.36, 5)),  # [[7, 0], [10, 10], [10, 10]], 4 frames wrong | [[8, 0], [6, 0], [9, 0]], 0 wrong
    ("thirteen", 3): ((0.34, 4), (0.33, 0)),  # [[6, 0], [10, 50], [10, 6]], 1 frames wrong | [[8, 0], [6, 0], [6, 0]], 0 wrong
    ("thirteen", 4): ((0.34, 2), (0.33, 0)),  # [[6, 0], [10, 50], [10, 50]], 8 frames wrong | [[8, 0], [6, 0], [6, 0]], 0 wrong
    ("thirteen", 5): ((0.36, 2), (0.36, 0)),  # [[7, 0], [10, 10], [10, 10]], 4 frames wrong | [[7, 0], [6, 0], [6, 0]], 0 wrong
    ("most", 0): ((0.42, 0), (0.38, 1)),  # [[10, 0], [10, 0], [10, 0]], 52 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("most", 1): ((0.36, 3), (0.34, 3)),  # [[6, 0], [10, 0], [10, 0]], 5 frames wrong | [[6, 0], [8, 0], [6, 0]], 0 wrong
    ("most", 2): ((0.37, 5), (0.39, 1)),  # [[10, 10], [8, 0], [10, 10]], 8 frames wrong | [[8, 0], [7, 0], [6, 0]], 0 wrong
    ("most", 3): ((0.36, 3), (0.34, 3)),  # [[6, 0], [10, 50], [10, 50]], 3 frames wrong | [[6, 0], [8, 0], [6, 0]], 0 wrong
    ("most", 4): ((0.36, 3), (0.34, 3)),  # [[6, 0], [10, 50], [10, 50]], 5 frames wrong | [[6, 0], [8, 0], [6, 0]], 0 wrong
    ("most", 5): ((0.37, 1), (0.38, 1)),  # [[10, 10], [10, 10], [7, 0]], 7 frames wrong | [[9, 0], [7, 0], [6, 0]], 0 wrong
    ("wide", 0): ((0.27, 1), (0.23, 0)),  # [[10, 0], [10, 0], [10, 0]], 94 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("wide", 1): ((0.25, 3), (0.25, 4)),  # [[10, 0], [10, 0], [8, 0]], 9 frames wrong | [[4, 0], [4, 0], [3, 0]], 1 wrong
    ("wide", 2): ((0.24, 1), (0.24, 0)),  # [[10, 10], [5, 0], [10, 10]], 2 frames wrong | [[4, 0], [5, 0], [3, 0]], 0 wrong
    ("wide", 3): ((0.25, 3), (0.25, 4)),  # [[10, 50], [10, 50], [8, 0]], 8 frames wrong | [[4, 0], [4, 0], [3, 0]], 1 wrong
    ("wide", 4): ((0.25, 3), (0.25, 4)),  # [[10, 50], [10, 50], [8, 0]], 9 frames wrong | [[4, 0], [4, 0], [3, 0]], 1 wrong
    ("wide", 5): ((0.25, 2), (0.25, 4)),  # [[10, 10], [9, 0], [10, 10]], 8 frames wrong | [[5, 0], [4, 0], [6, 0]], 1 wrong
    ("crowded", 0): ((0.33, 0), (0.25, 1)),  # [[10, 0], [10, 0], [10, 0]], 95 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("crowded", 1): ((0.29, 4), (0.28, 5)),  # [[10, 0], [4, 0], [10, 0]], 9 frames wrong | [[3, 0], [8, 0], [3, 0]], 1 wrong
    ("crowded", 2): ((0.29, 4), (0.28, 5)),  # [[10, 10], [5, 0], [10, 10]], 9 frames wrong | [[4, 0], [9, 0], [6, 0]], 1 wrong
    ("crowded", 3): ((0.29, 4), (0.28, 5)),  # [[10, 50], [4, 0], [10, 50]], 8 frames wrong | [[3, 0], [8, 0], [3, 0]], 1 wrong
    ("crowded", 4): ((0.29, 4), (0.28, 5)),  # [[10, 50], [4, 0], [10, 50]], 9 frames wrong | [[3, 0], [8, 0], [3, 0]], 1 wrong
    ("crowded", 5): ((0.29, 1), (0.28, 4)),  # [[10, 10], [8, 0], [10, 10]], 7 frames wrong | [[6, 0], [5, 0], [7, 0]], 2 wrong
    ("noflip", 0): ((0.36, 4), (0.27, 1)),  # [[10, 0], [10, 0], [10, 0]], 95 frames wrong | [[10, 0], [10, 0], [10, 0]], 0 wrong
    ("noflip", 1): ((0.29, 1), (0.29, 3)),  # [[10, 0], [10, 0], [8, 0]], 6 frames wrong | [[3, 0], [9, 0], [8, 0]], 1 wrong
    ("noflip", 2): ((0.29, 4), (0.28, 1)),  # [[6, 0], [5, 0], [10, 10]], 4 frames wrong | [[5, 0], [6, 0], [5, 0]], 0 wrong
    ("noflip", 3): ((0.29, 1), (0.29, 3)),  # [[10, 2], [10, 50], [8, 0]], 6 frames wrong | [[3, 0], [9, 0], [8, 0]], 1 wrong
    ("noflip", 4): ((0.29, 1), (0.29, 3)),  # [[10, 50], [10, 50], [8, 0]], 6 frames wrong | [[3, 0], [9, 0], [8, 0]], 1 wrong
    ("noflip", 5): ((0.30, 2), (0.29, 1)),  # [[10, 10], [10, 10], [8, 0]], 6 frames wrong | [[5, 0], [6, 0], [4, 0]], 0 wrong
}


def cfg_of(abi, lib, key):
    """the configurations of this module by name: "m0" .. "m5" lnsfaid_cfg_default ("m0" with Factor_1 = Factor_2 = 24, the four-rows
    kernel's NMS), "m0two" factors 24 / 28 (the two-rows kernel), "m0default" the default pair, "m2ef1" / "m2ef2" DecodeMethod 2 with
    EF_ELIMINATION 1 / 2, "m2classes" / "m5classes" a table set that differs between the four weight classes (the two-rows kernel)"""
    method = int(key[1])
    cfg = abi.default_cfg(method, MAX_ITER, lib)
    rest = key[2:]
    if key == "m0":
        cfg.factor_1 = cfg.factor_2 = 24
    elif key == "m0two":
        cfg.factor_1, cfg.factor_2 = 24, 28
    elif rest in ("ef1", "ef2"):
        assert lib.lnsfaid_cfg_ef_elimination(C.byref(cfg), int(rest[2])) == 0
    elif rest == "classes":
        for it in range(6):
            base = list(cfg.v2c_map[it][0])
            for a in range(8):
                cfg.v2c_map[it][1][a] = min(7, base[a] + (1 if a >= 2 else 0))
                cfg.v2c_map[it][2][a] = max(0, base[a] - (1 if a >= 3 else 0))
                cfg.v2c_map[it][3][a] = min(7, base[a] + (1 if a == 2 else 0))
    else:
        assert rest in ("", "default"), key
    return cfg


def method_of(key):
    return int(key[1])


_batches = {}


def batch(name, method, which):
    """(int8 fixInput of NG groups, the sent codewords [FRAMES, N]) of a (shape, DecodeMethod) batch, read-only; which: "mixed" or
    "clean" """
    k = (name, method, which)
    if k not in _batches:
        sigma, seed = BATCHES[(name, method)][0 if which == "mixed" else 1]
        if which == "mixed":
            fix, cw = random_batch(name, sigma, seed)
        else:
            fix, cw = zero_batch(name, sigma, seed), np.zeros((FRAMES, code(name).N), np.int8)
        fix.flags.writeable = False
        cw.flags.writeable = False
        _batches[k] = (fix, cw)
    return _batches[k]


_refs = {}


def reference(abi, lib, name, key, which, kind="avx2", groups=NG):
    """(decodedBits int8 [32 groups * N], records [groups, 2]) of configuration `key` on the first `groups` groups of the batch of
    (shape, DecodeMethod of key), computed once per process and shared read-only.  kind "avx2": the CPU port, "oracle": the scalar
    oracle"""
    k = (name, key, which, kind, groups)
    if k not in _refs:
        h = code(name)
        fix = batch(name, method_of(key), which)[0][:groups * 32 * h.N]
        out, st = oa.decode_mt(h, cfg_of(abi, lib, key), fix, groups, threads=groups, kind=kind)
        out.flags.writeable = False
        st.flags.writeable = False
        _refs[k] = (out, st)
    return _refs[k]


def references(abi, lib, todo):
    """reference() of many (name, key, which[, kind[, groups]]) side by side (the libraries release the interpreter)"""
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        return list(ex.map(lambda t: reference(abi, lib, *t), todo))


CODEWORDS = (0, 5, 31, 32, 40, 63, 64, 95)  # the subset the per-codeword rule is tested on: first and last of every group


def codeword_reference(abi, lib, name, key, which):
    """(decodedBits [8, N], [8, 2] iterations / bf_iterations) of CODEWORDS under the per-codeword rule: tests/early_stop_ref.py's
    32 copies of a codeword through the CPU port"""
    k = (name, key, which, "codeword")
    if k not in _refs:
        h = code(name)
        out, st = esr.per_codeword_oracle(h, cfg_of(abi, lib, key), batch(name, method_of(key), which)[0], NG, kind="avx2",
                                          cws=list(CODEWORDS))
        _refs[k] = (np.ascontiguousarray(out), st)
    return _refs[k]


def wrong_frames(h, out, cw):
    """mask [frames]: the decoded frame differs from the sent one"""
    return (np.asarray(out).reshape(-1, h.N) != cw).any(axis=1)


def check_batch_conditions(name, method, mixed, clean):
    """the conditions of the table's comment on the records and decisions the references gave; mixed / clean: (out, records)"""
    h = code(name)
    wrong = wrong_frames(h, mixed[0], batch(name, method, "mixed")[1])
    wrong_clean = wrong_frames(h, clean[0], batch(name, method, "clean")[1])
    it, bf = mixed[1][:, 0], mixed[1][:, 1]
    if method == 0:
        assert wrong.any() and not wrong.all(), (name, method, int(wrong.sum()))
        assert not wrong_clean.any(), (name, method, int(wrong_clean.sum()))
        return
    assert (it < MAX_ITER).any() and (it == MAX_ITER).any() and wrong.any(), (name, method, mixed[1].tolist(), int(wrong.sum()))
    if method in BF_METHODS:
        assert (bf > 0).any(), (name, method, mixed[1].tolist())
    ci = clean[1][:, 0]
    assert (ci < MAX_ITER).all() and len(set(ci.tolist())) > 1 and not clean[1][:, 1].any(), (name, method, clean[1].tolist())


def capture_case(abi, lib, name, n=33):
    """(frame indices, {format: line}, bits [n, N / 32], sent [n, N / 32]) for the line-format failure capture: n codewords of the
    DecodeMethod 2 mixed batch with the CPU port's decisions - up to 16 of the frames it left wrong or unsatisfied, filled up with the
    first other frames, in ascending order"""
    import line_ref as lr
    h = code(name)
    fix, cw = batch(name, 2, "mixed")
    out, _ = reference(abi, lib, name, "m2", "mixed")
    dec = out.reshape(FRAMES, h.N)
    bad = np.flatnonzero((dec != cw).any(axis=1) | (esr.unsatisfied(h, dec) > 0))
    assert bad.size > 0
    idx = np.sort(np.concatenate([bad[:16], np.setdiff1d(np.arange(FRAMES), bad[:16])[:n - min(16, bad.size)]]))
    assert idx.size == n
    pack = lambda x: np.packbits((x != 0).astype(np.uint8), axis=1, bitorder="little").view("<u4").astype(np.uint32)
    frames = frames_of(fix, h.N, h.K)[idx]
    L = h.N - h.code.puncture_tail
    lines = {fmt: lr.line_of(frames, L, fmt) for fmt in (lr.HARD, lr.LLR4)}
    return idx, lines, pack(dec[idx]), pack(cw[idx])


# ---- codes at and beyond the limits of lnsfaid_create -------------------------------------------------------------------------------
def _even(total, parts):
    """total edges over `parts` layers, as evenly as they go"""
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def _edit(shape, layers):
    return shape._replace(layers=layers)


def first_lds_overflow(nbr=20):
    """the first block-column count whose LDS image passes 16-bit addresses, for nbr layers"""
    nbc = nbr + 1
    while lds_bytes(nbc * Z, nbr * Z) <= 0xffff:
        nbc += 1
    return nbc


def limit_shape(name):
    """ACCEPTED / REFUSED by name"""
    if name in ("rows32", "rows33"):  # LF_MAX_BR
        nbr = int(name[4:])
        return realise(name, nbr, nbr + 8, 0, 33, [(8, 8)], _even(64, nbr))
    if name in ("degree24", "degree25"):  # LF_MAX_DEG: layer 1 takes 22 / 23 information columns next to its two parity columns
        d = int(name[6:]) - 2
        return realise(name, 2, 25, 0, 25, [(2, d - 3), (1, 26 - d)], [20, d])
    if name in ("degree2", "degree1"):  # layer 0 is its diagonal parity circulant and one information edge / nothing else
        s = realise(name, 3, 11, 0, 21, [(2, 8)], [1, 8, 7])
        return s if name == "degree2" else _edit(s, [s.layers[0][1:]] + s.layers[1:])
    if name in ("plain", "twice", "descending"):  # layer 1 names a block column twice / has two neighbours the wrong way round
        s = realise(name, 3, 11, 0, 22, [(2, 8)], [4, 6, 6])
        if name == "plain":
            return s
        row = list(s.layers[1])
        row[1:3] = [(row[0][0], row[1][1]), row[2]] if name == "twice" else [row[2], row[1]]
        return _edit(s, [s.layers[0], row, s.layers[2]])
    if name in ("weight16", "weight17"):  # LF_MAX_COLW: information column 0 in every layer
        nbr = int(name[6:])
        return realise(name, nbr, nbr + 8, 0, 16, [(nbr, 1), (4, 7)], _even(nbr + 28, nbr))
    if name in ("lds_last", "lds_over"):  # the widest code whose LDS image keeps 16-bit addresses, and one block column more
        nbr = 20
        nbc = first_lds_overflow(nbr) - (1 if name == "lds_last" else 0)
        return realise(name, nbr, nbc, 0, 65, [(2, nbc - nbr)], _even(2 * (nbc - nbr), nbr))
    raise KeyError(name)


# what lnsfaid_create must refuse with LNSFAID_E_CODE -> the nearest code it must accept
REFUSED = collections.OrderedDict([("rows33", "rows32"), ("degree25", "degree24"), ("degree1", "degree2"), ("twice", "plain"),
                                   ("descending", "plain"), ("weight17", "weight16"), ("lds_over", "lds_last")])


# ---- the line-format round trip ---------------------------------------------------------------------------------------------------
ROUND_TRIP_KEY = 0x5EED0F50C0DE2025
# mean flips per codeword of the binary symmetric channel.  `wide` (rate 8 / 9, column weights 2 and 3, 512 punctured parity bits) is
# left with unsatisfied checks by a single flip at some positions - codeword 3 of this stream at 1.0 and at 1.5, in the CPU port as
# on the device - so its channel is kept below that; tests/test_code_shapes_cpu.py decodes every case with the CPU port.
ROUND_TRIP_FLIPS = {"few": 3.0, "thirteen": 3.0, "most": 3.0, "wide": 0.6}


def round_trip_case(abi, lib, name, n=33):
    """(payload [n, K / 32], sent line, sent codewords [n, N / 32], threshold of the channel, received line, flips per codeword) from
    the host forms: lnsfaid_line_payload_random_host, lnsfaid_encode_line_host, lnsfaid_line_bsc_host with stream key + 1"""
    c = code(name).code
    payload = abi.line_payload_random_host(c, ROUND_TRIP_KEY, 0, n, lib)
    line, bits = abi.encode_line_host(c, payload, n, True, lib)
    thr = abi.line_bsc_threshold(ROUND_TRIP_FLIPS[name] / (c.n_var - c.puncture_tail), lib)
    rx, flips, _ = abi.line_bsc_host(c, line, n, ROUND_TRIP_KEY + 1, 0, thr, lib=lib)
    return payload, line, bits, thr, rx, flips
