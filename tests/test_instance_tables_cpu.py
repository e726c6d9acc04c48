"""The instance table of the four-rows decoders (LF4_INSTANCE_TABLE, lnsfaid_frame4.h): every family of kernels hands out the same
set of instances for (method, ef, rm).  No GPU: the functions only return addresses."""
import ctypes as C
import itertools

import pytest

METHODS, EFS, RMS = range(-1, 7), range(3), range(2)


@pytest.fixture(scope="module")
def families(lib):
    dll = C.CDLL(lib._name)

    def table(name, *tail):
        fn = getattr(dll, name)
        fn.restype = C.c_void_p
        fn.argtypes = [C.c_int] * (3 + len(tail))
        return {(m, ef, rm): fn(m, ef, rm, *tail) for m, ef, rm in itertools.product(METHODS, EFS, RMS)}

    return {
        "lf_decode4_func": table("lf_decode4_func"),
        "lf_decode4cw_func": table("lf_decode4cw_func"),
        "lf_decode4l_func": table("lf_decode4l_func"),
        "lf_decode4b_func": table("lf_decode4b_func"),
        "lf_decode4p_func group rule": table("lf_decode4p_func", 0),
        "lf_decode4p_func per codeword": table("lf_decode4p_func", 1),
    }


def test_an_instance_exactly_for_the_decode_methods(families):
    for name, t in families.items():
        for (m, ef, rm), p in t.items():
            assert (p is not None) == (0 <= m <= 5), (name, m, ef, rm)


def test_method_0_has_the_streaming_instance_only(families):
    for name, t in families.items():
        assert len({t[(0, ef, rm)] for ef in EFS for rm in RMS}) == 1, name


def test_the_erasing_instance_is_one_of_its_own(families):
    for name, t in families.items():
        assert t[(2, 2, 0)] == t[(2, 2, 1)], name
        assert t[(2, 2, 0)] not in (t[(2, 0, 0)], t[(2, 0, 1)]), name


def test_the_message_store_selects_an_instance(families):
    for name, t in families.items():
        for m in range(1, 6):
            assert t[(m, 0, 0)] != t[(m, 0, 1)], (name, m)


def test_no_instance_serves_two_families(families):
    sets = {name: {p for p in t.values() if p is not None} for name, t in families.items()}
    for a, b in itertools.combinations(sets, 2):
        assert not (sets[a] & sets[b]), (a, b)
