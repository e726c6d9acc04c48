"""lnsfaid_capture_errors_host (include/lnsfaid.h "error-frame capture") against the numpy restatement of the
definition (tests/capture_ref.py), byte for byte.  No GPU: the host function is what tests/test_gpu_capture.py holds the device
path against."""
import ctypes as C

import numpy as np
import pytest

import capture_ref as cr

E_INVAL = -1
N_GROUPS = 3


@pytest.fixture(scope="module")
def batches(code50):
    return {name: cr.batch(code50.N, code50.M, N_GROUPS, 100 + i, *spec) for i, (name, spec) in enumerate(sorted(cr.CASES.items()))}


def _host(lib, code50, fix, dec, sent, n_groups=N_GROUPS):
    ptr = [a.ctypes.data if a is not None else None for a in (fix, dec, sent)]
    return lambda skip, cap, r, p, f, s, o: lib.lnsfaid_capture_errors_host(code50.N, code50.M, ptr[0], ptr[1], ptr[2], n_groups, skip, cap,
                                                                            r, p, f, s, o)


@pytest.mark.parametrize("case", sorted(cr.CASES))
def test_host_equals_definition(lib, code50, batches, case):
    fix, dec, sent = batches[case]
    N, M = code50.N, code50.M
    fn = _host(lib, code50, fix, dec, sent)
    found, rec, pay = cr.check_against_ref(fn, N, M, fix, dec, sent, N_GROUPS, 0, 96)
    errs, par_only, k_edge = cr.CASES[case]
    assert rec["codeword"].tolist() == sorted(errs + k_edge) and found == len(errs) + len(k_edge)
    assert (rec["info_errors"] > 0).all() and (rec["reserved"] == 0).all()
    for cw in k_edge:
        r = rec[rec["codeword"] == cw][0]
        assert r["info_errors"] == 1 and r["parity_errors"] == 1
    # capacity 0 (counts only, NULL buffers allowed), 1 and more than found; every skip of the issue
    cr.check_against_ref(fn, N, M, fix, dec, sent, N_GROUPS, 0, 0)
    for cap in (1, found + 3):
        for skip in sorted({0, max(found - 1, 0), found, found + 5}):
            cr.check_against_ref(fn, N, M, fix, dec, sent, N_GROUPS, skip, cap, slots=cap)
    # paging with capacity 2 concatenates to the one-shot result
    recs, pays, skip = [], [], 0
    while True:
        f2, r2, p2 = cr.check_against_ref(fn, N, M, fix, dec, sent, N_GROUPS, skip, 2)
        assert f2 == found
        recs.append(r2)
        pays.append(p2)
        skip += r2.size
        if r2.size == 0 or skip >= found:
            break
    assert np.concatenate(recs).tobytes() == rec.tobytes() and np.concatenate(pays).tobytes() == pay.tobytes()


def test_parity_errors_alone_change_nothing(lib, code50, batches):
    """the same batch without its parity-only frames: same records but for parity_errors of no frame, same counters"""
    N, M = code50.N, code50.M
    fix, dec, sent = batches["parity_only"]
    _, dec_without, _ = cr.batch(N, M, N_GROUPS, 100 + sorted(cr.CASES).index("parity_only"), cr.CASES["parity_only"][0])
    a = cr.capture(N, M, fix, dec, sent, N_GROUPS, 0, 96)
    b = cr.capture(N, M, fix, dec_without, sent, N_GROUPS, 0, 96)
    assert a[0] == b[0] == 2 and a[1].tobytes() == b[1].tobytes() and a[3] == b[3]
    got = cr.check_against_ref(_host(lib, code50, fix, dec, sent), N, M, fix, dec, sent, N_GROUPS, 0, 96)
    assert got[1]["codeword"].tolist() == [7, 40]


@pytest.mark.parametrize("no_fix,no_sent", [(True, False), (False, True), (True, True)], ids=["no_fix", "no_sent", "neither"])
def test_null_inputs(lib, code50, batches, no_fix, no_sent):
    """sent = NULL is the all-zero codeword: every frame with a 1 among its information decisions is an error frame; fixInput = NULL
    zeroes the LLR section"""
    N, M = code50.N, code50.M
    fix, dec, sent = batches["group_edges"]
    if no_sent:  # decisions against zero: keep the error frames rare enough to be a pattern - the planted flips themselves
        dec = (dec.reshape(-1, N) ^ cr.frames_of(sent, N_GROUPS, N, M)).reshape(-1)
    fix, sent = (None if no_fix else fix), (None if no_sent else sent)
    found, rec, pay = cr.check_against_ref(_host(lib, code50, fix, dec, sent), N, M, fix, dec, sent, N_GROUPS, 0, 96)
    assert rec["codeword"].tolist() == [0, 31, 32, 63, 95]
    if no_fix:
        assert not pay[:, 0].any()
    if no_sent:
        assert not pay[:, 2].any()


def test_counters_are_those_of_count_errors(lib, code50, batches):
    """TestFrame, ErrorFrame, ErrorBits, LT3ErrBitFrame by lnsfaid_count_errors' definition (CLDPC.cpp:4842-4876: the first K
    decisions of a frame against its information bits), added to what out holds; out = NULL is allowed"""
    N, M, K = code50.N, code50.M, code50.K
    fix, dec, sent = batches["adjacent_pairs"]
    info = cr.frames_of(sent, N_GROUPS, N, M)[:, :K]
    wrong = (dec.reshape(-1, N)[:, :K] != info).sum(axis=1)
    want = [96, int((wrong > 0).sum()), int(wrong.sum()), int(((wrong > 0) & (wrong < 3)).sum())]
    assert want[3] > 0 and want[3] < want[1]
    fn = _host(lib, code50, fix, dec, sent)
    rc, found, stored, _, _, cnt, intact = cr.guarded_call(lambda r, p, f, s, o: fn(0, 96, r, p, f, s, o), N, 96, out=[0, 0, 0, 0])
    assert rc == 0 and cnt == want and found == want[1] and intact
    rc, found, stored, _, _, cnt, intact = cr.guarded_call(lambda r, p, f, s, o: fn(0, 96, r, p, f, s, o), N, 96, out=[1, 2, 3, 1 << 50])
    assert rc == 0 and cnt == [1 + want[0], 2 + want[1], 3 + want[2], (1 << 50) + want[3]]
    rc, found, stored, _, _, cnt, intact = cr.guarded_call(lambda r, p, f, s, o: fn(0, 96, r, p, f, s, None), N, 96)
    assert rc == 0 and found == want[1] and stored == want[1] and intact


def test_pyabi_wrapper(abi, lib, code50, batches):
    N, M = code50.N, code50.M
    fix, dec, sent = batches["group_edges"]
    want = cr.capture(N, M, fix, dec, sent, N_GROUPS, 1, 3)
    found, rec, pay, cnt = abi.capture_errors_host(N, M, fix, dec, sent, N_GROUPS, skip=1, capacity=3, counters=True, lib=lib)
    assert found == 5 and rec.dtype == cr.RECORD and rec.tobytes() == want[1].tobytes() and pay.shape == (3, 3, N)
    assert pay.tobytes() == want[2].tobytes() and cnt == want[3]
    assert len(abi.capture_errors_host(N, M, None, dec, None, N_GROUPS, lib=lib)) == 3


def test_rules(lib, code50, batches):
    N, M = code50.N, code50.M
    fix, dec, sent = batches["group_edges"]
    fn = lib.lnsfaid_capture_errors_host
    rec = np.full(96, 0x5A5A5A5A, dtype=np.uint32).view(cr.RECORD)
    pay = np.full(96 * 3 * N, 0x5A, dtype=np.int8)
    found, stored = C.c_uint64(77), C.c_uint64(88)
    out = (C.c_uint64 * 4)(1, 2, 3, 4)
    f, s = C.byref(found), C.byref(stored)
    args = (fix.ctypes.data, dec.ctypes.data, sent.ctypes.data)
    assert fn(N, M, args[0], None, args[2], N_GROUPS, 0, 96, rec.ctypes.data, pay.ctypes.data, f, s, out) == E_INVAL  # decodedBits
    assert fn(N, M, *args, N_GROUPS, 0, 96, rec.ctypes.data, pay.ctypes.data, None, s, out) == E_INVAL  # found
    assert fn(N, M, *args, N_GROUPS, 0, 96, rec.ctypes.data, pay.ctypes.data, f, None, out) == E_INVAL  # stored
    assert fn(N, M, *args, N_GROUPS, 0, 1, None, pay.ctypes.data, f, s, out) == E_INVAL  # records with capacity > 0
    assert fn(N, M, *args, N_GROUPS, 0, 1, rec.ctypes.data, None, f, s, out) == E_INVAL  # payload with capacity > 0
    for n_var, n_check in ((N, 0), (N, N), (0, 0), (M, N)):
        assert fn(n_var, n_check, *args, N_GROUPS, 0, 96, rec.ctypes.data, pay.ctypes.data, f, s, out) == E_INVAL
    # a refused call touches nothing
    assert (found.value, stored.value, list(out)) == (77, 88, [1, 2, 3, 4])
    assert (rec.view(np.uint32) == 0x5A5A5A5A).all() and (pay == 0x5A).all()
    # capacity 0 counts only: NULL records and payload are fine
    info = [1 + cw % 5 for cw in (0, 31, 32, 63, 95)]
    assert fn(N, M, *args, N_GROUPS, 0, 0, None, None, f, s, out) == 0
    assert (found.value, stored.value, list(out)) == (5, 0, [97, 7, 3 + sum(info), 4 + sum(1 for n in info if n < 3)])
    # n_groups 0: a no-op that sets found = stored = 0, whatever else is NULL
    found.value, stored.value = 77, 88
    assert fn(N, M, None, None, None, 0, 0, 96, None, None, f, s, out) == 0 and (found.value, stored.value) == (0, 0)
    assert fn(N, M, None, None, None, 0, 0, 96, None, None, None, None, None) == 0
    assert list(out)[0] == 97
