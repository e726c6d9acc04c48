"""The syndrome walk of the bit-flipping stage split by what the stage can change, on the host: the tables the library
builds (lnsfaid_code_bf_walk, no GPU) are walked here as the kernels walk them - per (layer, 32-row word) the XOR over the slots of
alignbit(word at the high address, word at the low address, bit offset) on an image of the LDS that holds the hard-decision plane
and the zero word - and the parity plane of the full walk must equal the fixed share XOR the walk of the flipped columns."""
import numpy as np
import pytest

LAYERS, COLS, Z = 12, 69, 256


def _walk(tab, lds):
    """tab [layers][slots][8][2] -> parity words [layers][8] for every plane of lds [planes][words]"""
    lo, hi, sh = (tab[..., 0] & 0xffff) >> 2, (tab[..., 0] >> 16) >> 2, tab[..., 1].astype(np.uint64)
    assert not ((tab[..., 0] & 0x00030003).any() or (sh > 31).any())
    pair = lds[:, lo].astype(np.uint64) | (lds[:, hi].astype(np.uint64) << np.uint64(32))  # v_alignbit_b32(high, low, shift)
    return np.bitwise_xor.reduce(((pair >> sh) & np.uint64(0xffffffff)).astype(np.uint32), axis=2)


def _circulants(tab, info):
    """per layer the set of (block column, shift) of the table's real slots, from word 0's entry; every real slot checked to be one"""
    hard0, zero = info[0], info[1]
    out = []
    for br in range(tab.shape[0]):
        found = []
        for j in range(tab.shape[1]):
            x, y = int(tab[br, j, 0, 0]), int(tab[br, j, 0, 1])
            if x == (zero | (zero << 16)):
                assert y == 0 and (tab[br, j, :, 0] == x).all() and not tab[br, j, :, 1].any()
                continue
            w = ((x & 0xffff) - hard0) // 4
            found.append((w // 8, ((w % 8) * 32 + y) % Z))
        assert len(set(found)) == len(found)
        out.append(found)
    return out


def _base_matrix(code50):
    """per layer the (block column, shift) of its circulants, from the first row of the layer in the code's own table"""
    pos = np.ctypeslib.as_array(code50.pos_vn).astype(np.int64)
    rows, e = [], 0
    degs = np.repeat(np.ctypeslib.as_array(code50.deg), np.ctypeslib.as_array(code50.deg_rows))
    for br in range(LAYERS):
        d = int(degs[br * Z])
        rows.append([(int(v) // Z, int(v) % Z) for v in pos[e:e + d]])
        e += d * Z
    return rows


@pytest.fixture(scope="module")
def planes(code50):
    rng = np.random.default_rng(3101)
    nw = code50.N // 32
    p = rng.integers(0, 1 << 32, size=(201, nw), dtype=np.uint64).astype(np.uint32)
    p[200] = 0
    return p


def _lds(planes, info):
    hard0, zero = info[0], info[1]
    lds = np.full((planes.shape[0], zero // 4 + 1), 0xdeadbeef, np.uint32)  # anything but the plane and the zero word is poison
    lds[:, hard0 // 4:hard0 // 4 + planes.shape[1]] = planes
    lds[:, zero // 4] = 0
    return lds


@pytest.mark.parametrize("W,n_cols", [(3, 50), (6, 17)])
def test_split_walk(abi, lib, code50, planes, W, n_cols):
    full, flipped, fixed, info = abi.code_bf_walk(code50.code, W, lib)
    assert full.shape == (LAYERS, 24, 8, 2) and fixed.shape == full.shape and flipped.shape == (LAYERS, info[2], 8, 2)
    assert info[2] % 2 == 0 and info[4] == n_cols
    rows = _base_matrix(code50)
    weight = np.bincount([cb for r in rows for cb, _ in r], minlength=COLS)
    assert int((weight == W).sum()) == n_cols
    cf, cw, cx = _circulants(full, info), _circulants(flipped, info), _circulants(fixed, info)
    fits = all(sum(weight[cb] == W for cb, _ in r) <= info[2] for r in rows)
    assert info[3] == int(fits)
    assert fits and info[2] == 14  # 2 x 7 slots hold either split of the built-in code: the equality below is always checked
    for br in range(LAYERS):
        assert sorted(cf[br]) == sorted(rows[br])
        # every circulant of the base matrix in exactly one of the two tables, by its column's weight
        assert sorted(cx[br]) == sorted(x for x in rows[br] if weight[x[0]] != W)
        assert sorted(cw[br]) == sorted(x for x in rows[br] if weight[x[0]] == W)
        assert sorted(cw[br] + cx[br]) == sorted(rows[br])
        if W == 3:
            assert len(cw[br]) in (12, 13), (br, len(cw[br]))
    lds = _lds(planes, info)
    want = _walk(full, lds)
    got = _walk(fixed, lds) ^ _walk(flipped, lds)
    assert np.array_equal(want, got)
    # and the full walk is the syndrome: parity of rows 32 k .. 32 k + 31 of layer br on the first planes
    for p in (0, 200):
        bits = ((planes[p][:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
        for br in range(LAYERS):
            par = np.zeros(Z, np.uint32)
            for cb, sh in rows[br]:
                par ^= np.roll(bits[cb * Z:cb * Z + Z], -sh).astype(np.uint32)
            words = (par.reshape(8, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
            assert np.array_equal(words, want[p, br])


def test_total_split_of_the_built_in_code(abi, lib, code50):
    """150 of the 275 circulants lie in the 50 block columns of weight 3"""
    _, flipped, fixed, info = abi.code_bf_walk(code50.code, 3, lib)
    assert sum(len(x) for x in _circulants(flipped, info)) == 150
    assert sum(len(x) for x in _circulants(fixed, info)) == 125
