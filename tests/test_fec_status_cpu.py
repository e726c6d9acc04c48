"""lnsfaid_fec_status_host / lnsfaid_fec_status_packed_host (include/lnsfaid.h "FEC status") against the numpy
restatement of the definition (tests/fec_status_ref.py): exact integer equalities.  No GPU: the host forms are what
tests/test_gpu_fec_status.py holds the device forms against."""
import ctypes as C

import numpy as np
import pytest

import capture_ref as cr
import fec_status_ref as fr
import oracle_abi as oa

E_INVAL = -1


def _check(abi, lib, code, fix, dec, sent, n_groups, with_sent=True):
    """host form == definition: records codeword for codeword, out and vs_sent added to what they hold"""
    want_rec, want_out, want_vs = fr.status(code, fix, dec, sent, n_groups, with_sent)
    rec, out, vs = abi.fec_status_host(code, fix, dec, sent, n_groups, out=[3, 5, 7, 1 << 40], vs_sent=[1, 2, 3, 4] if with_sent else None,
                                       lib=lib)
    bad = np.nonzero(rec != want_rec)[0]
    assert bad.size == 0, (bad[:8], rec[bad[:8]], want_rec[bad[:8]])
    assert out == [a + b for a, b in zip([3, 5, 7, 1 << 40], want_out)], (out, want_out)
    assert vs == ([a + b for a, b in zip([1, 2, 3, 4], want_vs)] if with_sent else None), (vs, want_vs)
    return rec, want_out, want_vs


def test_golden_codeword(abi, lib, code50):
    """32 copies of the reference's known codeword with LLRs that agree with every bit: nothing unsatisfied, nothing corrected"""
    N, M = code50.N, code50.M
    cw = fr.golden_codeword(N)
    assert fr.unsatisfied(code50.code, cw[None, :])[0] == 0
    frames = np.tile(cw, (32, 1))
    fix = cr.layout_of(np.where(frames > 0, 5, -3).astype(np.int8), 1, N, M)
    dec = np.ascontiguousarray(frames.reshape(-1))
    rec, out, vs = _check(abi, lib, code50.code, fix, dec, cr.layout_of(frames, 1, N, M), 1)
    assert not rec["unsatisfied"].any() and not rec["corrected"].any()
    assert out == [32, 0, 0, 0] and vs == [32, 0, 0, 0]


def test_random_decisions(abi, lib, code50):
    """a dense syndrome: about half of the 3072 checks of every codeword, any wrong rotation shows"""
    fix, dec, sent = fr.random_batch(code50.code, 11, 2, dirty=1.0)
    rec, out, vs = _check(abi, lib, code50.code, fix, dec, sent, 2)
    assert (rec["unsatisfied"] > 1200).all() and (rec["unsatisfied"] < 1900).all()
    assert out == [64, 64, 0, 0] and vs == [64, 64, 0, 0]


@pytest.fixture(scope="module")
def pairs(code50):
    return fr.pair_batch(code50.code, 25, 25)


def test_planted_pairs(abi, lib, code50, pairs):
    """two flipped neighbours of one check: w(a) + w(b) - 2 * (checks they share), and they share the planted one"""
    code = code50.code
    fix, dec, sent = pairs
    rec, _, _ = _check(abi, lib, code, fix, dec, sent, 25)
    pos, row_of = fr.tables(code)
    weight = np.bincount(pos, minlength=code.n_var)
    checks_of = {}
    i = 0
    for r in fr.pair_rows(code):
        vn = pos[row_of == r]
        for a, b in zip(vn[:-1], vn[1:]):
            for v in (a, b):
                if v not in checks_of:
                    checks_of[v] = set(row_of[pos == v].tolist())
            shared = len(checks_of[a] & checks_of[b])
            assert shared >= 1 and rec["unsatisfied"][i] == weight[a] + weight[b] - 2 * shared, (r, a, b)
            i += 1
    assert i == 789


def test_corrected(abi, lib, code50):
    """LLRs over -8 .. 7 with zeros; differences at both sides of n_var - puncture_tail and of K, in frames 0 and 31 of a group (the
    two-segment layout); differences in the punctured tail alone count nothing"""
    N, M, K = code50.N, code50.M, code50.K
    L = N - code50.code.puncture_tail
    rng = np.random.default_rng(5)
    llr = rng.integers(-8, 8, (64, N), dtype=np.int8)
    assert (llr == 0).any() and (llr == -8).any()
    bits = (llr > 0).astype(np.int8)  # decisions = channel decisions: corrected 0 everywhere
    fix = cr.layout_of(llr, 2, N, M)
    rec, _, _ = _check(abi, lib, code50.code, fix, np.ascontiguousarray(bits.reshape(-1)), None, 2)
    assert not rec["corrected"].any()
    want = np.zeros(64, dtype=np.int64)
    for c, ks in {0: [L - 1], 1: [L], 31: [K - 1], 32: [K], 33: [K - 1, K, L - 1, L, N - 1], 63: [0, L - 1], 40: list(range(L, N)),
                  5: [0, 1, 15, 16, 31, 32, 255, 256]}.items():
        bits[c, ks] ^= 1
        want[c] = sum(1 for k in ks if k < L)
    rec, _, _ = _check(abi, lib, code50.code, fix, np.ascontiguousarray(bits.reshape(-1)), None, 2)
    assert rec["corrected"].tolist() == want.tolist()
    # fixInput == NULL: 0 for every codeword
    rec, out, _ = _check(abi, lib, code50.code, None, np.ascontiguousarray(bits.reshape(-1)), None, 2)
    assert not rec["corrected"].any() and out[2] == out[3] == 0


def test_vs_sent(abi, lib, code50, encoder):
    N, M, K = code50.N, code50.M, code50.K
    code = code50.code
    rng = np.random.default_rng(8)
    sent_frames = encoder.encode(rng.integers(0, 2, (64, K), dtype=np.uint8))
    assert not fr.unsatisfied(code, sent_frames).any()
    dec = sent_frames.copy()
    other = encoder.encode(rng.integers(0, 2, (1, K), dtype=np.uint8))[0]
    dec[3] = other                      # a valid but wrong codeword: undetected
    dec[31, [7, K - 1]] ^= 1            # wrong information bits, checks unsatisfied: detected
    dec[32, K + 5] ^= 1                 # one wrong parity bit only: a false alarm
    dec[63, N - 1] ^= 1
    sent = cr.layout_of(sent_frames, 2, N, M)
    flat = np.ascontiguousarray(dec.reshape(-1))
    rec, out, vs = _check(abi, lib, code, None, flat, sent, 2)
    assert vs == [64, 2, 1, 2] and out == [64, 3, 0, 0]
    assert rec["unsatisfied"][3] == 0 and rec["unsatisfied"][31] > 0 and rec["unsatisfied"][32] > 0
    info = np.ascontiguousarray(sent_frames[:, :K].reshape(-1))
    assert vs[1] == oa.Oracle(code50, abi.default_cfg(2, 10)).count_errors(flat, info, 2)[1]
    # sent == NULL with vs_sent: the all-zero codeword
    _, _, vs0 = _check(abi, lib, code, None, flat, None, 2)
    assert vs0[1] == oa.Oracle(code50, abi.default_cfg(2, 10)).count_errors(flat, None, 2)[1] == 64
    # a decision byte that is not 0 / 1 is a 1-bit for the syndrome and differs from a sent 1
    odd = flat.copy().reshape(64, N)
    k1 = int(np.nonzero(sent_frames[10, :K])[0][0])
    odd[10, k1] = 3
    rec, _, vs = _check(abi, lib, code, None, np.ascontiguousarray(odd.reshape(-1)), sent, 2)
    assert rec["unsatisfied"][10] == 0 and vs == [64, 3, 2, 2]


def test_golden_group_with_a_trapped_frame(abi, lib, code50):
    """the 3.55 dB golden group: its one error frame (frame 9, 156 wrong information bits) leaves 175 checks unsatisfied - a
    detected failure -, the other 31 frames are the codeword"""
    N, M = code50.N, code50.M
    z, fix, dec = fr.golden_group("m2_3p55dB_cw_g0", N)
    sent = cr.layout_of(np.tile(fr.golden_codeword(N), (32, 1)), 1, N, M)
    rec, out, vs = _check(abi, lib, code50.code, fix, dec, sent, 1)
    assert vs == [32, 1, 0, 0]
    assert rec["unsatisfied"].tolist() == [175 if m == 9 else 0 for m in range(32)]
    assert out[:2] == [32, 1] and out[2] == int((rec["corrected"][rec["unsatisfied"] == 0] > 0).sum())


@pytest.mark.parametrize("with_fix,with_sent", [(True, True), (False, True), (True, False)], ids=["all", "no_llr", "no_sent"])
def test_packed_equals_int8(abi, lib, code50, with_fix, with_sent):
    code = code50.code
    fix, dec, sent = fr.random_batch(code, 21, 2)
    dec01 = (dec != 0).astype(np.int8)  # the packed form carries bits: compare on decisions that are 0 / 1
    a = abi.fec_status_host(code, fix if with_fix else None, dec01, sent if with_sent else None, 2, vs_sent=True, lib=lib)
    b = abi.fec_status_packed_host(code, abi.pack_llr4(fix, lib) if with_fix else None, fr.pack_decisions(dec01), sent if with_sent else None,
                                   2, vs_sent=True, lib=lib)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    assert a[0]["unsatisfied"].any() and (a[0]["unsatisfied"] == 0).any() and 0 < a[2][1] < 64
    want = fr.status(code, fix if with_fix else None, dec01, sent if with_sent else None, 2, True)
    assert a[0].tobytes() == want[0].tobytes() and a[1:] == want[1:]
    if with_fix:
        assert (fix == -8).any() and a[0]["corrected"].any()


def _toy_code(abi):
    """3 x 6 circulants of size 5: 30 bits, 15 checks, layers of degree 3, 4, 3, a punctured tail of 3"""
    z, base = 5, [[(0, 1), (2, 0), (3, 4)], [(0, 0), (1, 2), (3, 3), (4, 1)], [(1, 4), (2, 2), (5, 0)]]
    pos = [cb * z + (sh + i) % z for row in base for i in range(z) for cb, sh in row]
    keep = ((C.c_uint16 * len(pos))(*pos), (C.c_int32 * 3)(3, 4, 3), (C.c_int32 * 3)(z, z, z))
    code = abi.Code(n_var=6 * z, n_check=3 * z, n_edges=len(pos), z=z, puncture_tail=3, nb_degres=3,
                    deg=C.cast(keep[1], C.POINTER(C.c_int32)), deg_rows=C.cast(keep[2], C.POINTER(C.c_int32)),
                    pos_vn=C.cast(keep[0], C.POINTER(C.c_uint16)))
    return code, keep


def test_toy_code(abi, lib):
    """the host form is driven by the tables, not shaped like the 50G-PON code"""
    code, keep = _toy_code(abi)
    N, M = code.n_var, code.n_check
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (64, N), dtype=np.int8)
    bits[:8] = 0
    bits[1, 4] = 1
    llr = rng.integers(-8, 8, (64, N), dtype=np.int8)
    sent = rng.integers(0, 2, (64, N), dtype=np.int8)
    sent[:8] = 0
    rec, out, vs = _check(abi, lib, code, cr.layout_of(llr, 2, N, M), np.ascontiguousarray(bits.reshape(-1)), cr.layout_of(sent, 2, N, M), 2)
    assert rec["unsatisfied"][0] == 0 and rec["unsatisfied"][1] == 2 and len(set(rec["unsatisfied"].tolist())) > 3
    assert vs[0] == 64 and vs[1] == 57
    # n_var % 32 != 0: no packed form
    assert lib.lnsfaid_fec_status_packed_host(C.byref(code), None, bits.ctypes.data, None, 1, None, None, None) == E_INVAL


def test_rules(abi, lib, code50):
    code = code50.code
    N = code50.N
    fix, dec, sent = fr.random_batch(code, 4, 1)
    bits = fr.pack_decisions(dec)
    rec = np.full(32, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    out, vs = (C.c_uint64 * 4)(1, 2, 3, 4), (C.c_uint64 * 4)(5, 6, 7, 8)
    host, packed = lib.lnsfaid_fec_status_host, lib.lnsfaid_fec_status_packed_host
    assert host(None, fix.ctypes.data, dec.ctypes.data, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == E_INVAL
    assert packed(None, None, bits.ctypes.data, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == E_INVAL
    assert host(C.byref(code), fix.ctypes.data, None, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == E_INVAL
    assert packed(C.byref(code), None, None, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == E_INVAL
    for field, value in (("n_check", 0), ("n_check", N), ("puncture_tail", N + 1), ("n_edges", 70399), ("n_var", N - 1)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert host(C.byref(broken), fix.ctypes.data, dec.ctypes.data, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == E_INVAL, field
    # a refused call touches nothing
    assert (rec == 0x5A5A5A5A5A5A5A5A).all() and list(out) == [1, 2, 3, 4] and list(vs) == [5, 6, 7, 8]
    # n_groups 0: a no-op, every buffer may be NULL
    assert host(C.byref(code), None, None, None, 0, None, None, None) == 0
    assert packed(C.byref(code), None, None, None, 0, rec.ctypes.data, out, vs) == 0
    assert (rec == 0x5A5A5A5A5A5A5A5A).all() and list(out) == [1, 2, 3, 4] and list(vs) == [5, 6, 7, 8]
    # every output is optional; out and vs_sent are added to: call twice
    assert host(C.byref(code), fix.ctypes.data, dec.ctypes.data, sent.ctypes.data, 1, None, None, None) == 0
    want = fr.status(code, fix, dec, sent, 1, True)
    for n in (1, 2):
        assert host(C.byref(code), fix.ctypes.data, dec.ctypes.data, sent.ctypes.data, 1, rec.ctypes.data, out, vs) == 0
        assert list(out) == [a + n * b for a, b in zip([1, 2, 3, 4], want[1])]
        assert list(vs) == [a + n * b for a, b in zip([5, 6, 7, 8], want[2])]
    assert rec.view(fr.RECORD).tobytes() == want[0].tobytes()


def test_pyabi_wrapper(abi, lib, code50):
    assert abi.fec_record_dtype() == fr.RECORD
    fix, dec, sent = fr.random_batch(code50.code, 4, 1)
    rec, out, vs = abi.fec_status_host(code50.code, fix, dec, sent, 1, lib=lib)
    assert rec.dtype == fr.RECORD and rec.size == 32 and out[0] == 32 and vs is None
    rec, out, vs = abi.fec_status_host(code50.code, None, dec, None, 1, records=False, out=None, vs_sent=True, lib=lib)
    assert rec is None and out is None and vs[0] == 32
