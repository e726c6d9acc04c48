"""Burst-format line calls without a GPU (include/lnsfaid.h "burst-format line calls"): the three host forms against
the numpy restatement of the formats (tests/burst_ref.py) and against tests/gf2_encoder.py, shortened = NULL against the line
helpers, the error rules, the ABI surface, the stand-alone sanitizer program, and the build-time properties of the two new kernel
files (lnsfaid_kernel4b.hip, lnsfaid_encoder_burst.hip) taken from a cross-compile for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import burst_ref as br
import line_ref as lr
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL = -1
HARD, LLR4, TAIL, HEAD = br.HARD, br.LLR4, br.TAIL, br.HEAD
NEW_SYMBOLS = {"lnsfaid_decode_burst": 11, "lnsfaid_decode_burst_device": 11, "lnsfaid_encode_burst": 7, "lnsfaid_encode_burst_device": 7,
               "lnsfaid_encode_burst_host": 9, "lnsfaid_burst_to_llr4": 8, "lnsfaid_burst_words": 5}
BATCHES = [("cycle", 33), ("burst", 33), ("cycle", 1), ("cycle", 65)]
BATCH_IDS = ["cycle33", "burst33", "one", "cycle65"]


def _dims(code50):
    N, M, K = code50.N, code50.M, code50.K
    return N, M, K, N - code50.code.puncture_tail


@pytest.fixture(scope="module")
def circ50(abi, lib, code50):
    return abi.code_parity_inverse(code50.code, lib)


def test_shortening_set(code50):
    N, M, K, L = _dims(code50)
    assert br.SHORT == (0, 32, 224, 256, 288, 5760, 8288, 14560) and br.SHORT[-1] == K - 32
    assert all(s % 32 == 0 for s in br.SHORT) and any((s // 32) % 2 for s in br.SHORT)
    s = br.burst_shaped_batch(33)
    assert sorted(np.nonzero(s)[0].tolist()) == [7, 8, 32]


@pytest.mark.parametrize("name,n", BATCHES, ids=BATCH_IDS)
def test_burst_words(abi, lib, code50, name, n):
    N, M, K, L = _dims(code50)
    s = br.batch(name, n)
    assert abi.burst_words(code50.code, s, n, lib) == br.burst_words(n, K, L, s)
    assert abi.burst_words(code50.code, None, n, lib) == (n * L, n * K)
    assert abi.burst_words(code50.code, None, 0, lib) == (0, 0)


@pytest.mark.parametrize("where", [TAIL, HEAD], ids=["tail", "head"])
@pytest.mark.parametrize("fmt,magnitude", [(HARD, 1), (HARD, 7), (LLR4, 0)], ids=["hard1", "hard7", "llr4"])
@pytest.mark.parametrize("name,n", BATCHES, ids=BATCH_IDS)
def test_burst_to_llr4(abi, lib, code50, name, n, fmt, magnitude, where):
    """random levels over all of -8 .. 7: the helper against the numpy restatement, byte for byte"""
    N, M, K, L = _dims(code50)
    s = br.batch(name, n)
    rng = np.random.default_rng(7 + n)
    frames = rng.integers(-8, 8, (n, N), dtype=np.int8)
    line = br.burst_line_of(frames, K, L, fmt, s, where)
    line_bits, _ = br.burst_words(n, K, L, s)
    assert line.size == (line_bits // 32 if fmt == HARD else line_bits // 2)
    got = abi.burst_to_llr4(code50.code, line, fmt, magnitude, s, where, n, lib)
    want = br.llr4_of_burst(line, n, N, K, L, fmt, magnitude, s, where)
    assert got.tobytes() == want.tobytes()
    # the known range is -7, the punctured tail 0, in the frame-major view of what came out
    f = lr.frames_of(lr.unpack_nibbles(got), N, K)[:n]
    for c, S in enumerate(s):
        k0, k1 = br.known_range(K, S, where)
        assert (f[c, k0:k1] == -7).all() and (f[c, L:] == 0).all()
    assert (lr.frames_of(lr.unpack_nibbles(got), N, K)[n:] == 0).all()


@pytest.mark.parametrize("fmt,magnitude", [(HARD, 4), (LLR4, 0)], ids=["hard4", "llr4"])
def test_null_shortened_is_line_to_llr4(abi, lib, code50, fmt, magnitude):
    N, M, K, L = _dims(code50)
    n = 33
    frames = np.random.default_rng(3).integers(-8, 8, (n, N), dtype=np.int8)
    line = lr.line_of(frames, L, fmt)
    want = abi.line_to_llr4(code50.code, line, fmt, magnitude, n, lib)
    for where in (TAIL, HEAD):
        assert abi.burst_to_llr4(code50.code, line, fmt, magnitude, None, where, n, lib).tobytes() == want.tobytes()
        assert abi.burst_to_llr4(code50.code, line, fmt, magnitude, np.zeros(n, np.uint32), where, n, lib).tobytes() == want.tobytes()


@pytest.mark.parametrize("where", [TAIL, HEAD], ids=["tail", "head"])
@pytest.mark.parametrize("name,n", BATCHES, ids=BATCH_IDS)
def test_encode_burst_host(abi, lib, code50, encoder, circ50, name, n, where):
    N, M, K, L = _dims(code50)
    s = br.batch(name, n)
    msg = br.zero_known(np.random.default_rng(11 + n).integers(0, 2, (n, K), dtype=np.uint8), s, where)
    payload = br.burst_payload_of(msg, s, where)
    assert np.array_equal(br.expand_payload(payload, n, K, s, where), msg)
    cw = encoder.encode(msg)  # gf2_encoder on the expanded message
    line, bits = abi.encode_burst_host(code50.code, payload, s, where, n, True, lib, circ50)
    assert bits.tobytes() == lr.payload_of(cw).tobytes()
    assert line.tobytes() == br.burst_line_of_codewords(cw, K, L, s, where).tobytes()
    for c, S in enumerate(s):  # bits: zeros in the known range
        k0, k1 = br.known_range(K, S, where)
        assert not bits[c, k0 // 32:k1 // 32].any()
    line_only, none = abi.encode_burst_host(code50.code, payload, s, where, n, False, lib, circ50)
    assert none is None and line_only.tobytes() == line.tobytes()


def test_null_shortened_is_encode_line_host(abi, lib, code50, circ50):
    N, M, K, L = _dims(code50)
    n = 33
    payload = np.random.default_rng(5).integers(0, 2 ** 32, n * K // 32, dtype=np.uint64).astype(np.uint32)
    want_line, want_bits = abi.encode_line_host(code50.code, payload, n, True, lib, circ50)
    for where in (TAIL, HEAD):
        for s in (None, np.zeros(n, np.uint32)):
            line, bits = abi.encode_burst_host(code50.code, payload, s, where, n, True, lib, circ50)
            assert line.tobytes() == want_line.tobytes() and bits.tobytes() == want_bits.tobytes()


def test_error_rules(abi, lib, code50, circ50):
    """every refusal leaves the patterned outputs untouched"""
    N, M, K, L = _dims(code50)
    code = code50.code
    n = 3
    good = np.array([0, 32, 256], np.uint32)
    line = np.full(n * L // 32, 0x5A5A5A5A, np.uint32)
    payload = np.full(n * K // 32, 0x5A5A5A5A, np.uint32)
    bits = np.full(n * N // 32, 0x5A5A5A5A, np.uint32)
    llr4 = np.full(32 * N // 2, 0x5A, np.uint8)
    totals = np.full(2, 0x5A5A5A5A5A5A5A5A, np.uint64)
    pc, pl, pp, pb, p4 = circ50.ctypes.data, line.ctypes.data, payload.ctypes.data, bits.ctypes.data, llr4.ctypes.data
    pt0, pt1 = totals.ctypes.data, totals.ctypes.data + 8
    to_llr4, enc, words = lib.lnsfaid_burst_to_llr4, lib.lnsfaid_encode_burst_host, lib.lnsfaid_burst_words

    def untouched():
        assert (line == 0x5A5A5A5A).all() and (payload == 0x5A5A5A5A).all() and (bits == 0x5A5A5A5A).all()
        assert (llr4 == 0x5A).all() and (totals == 0x5A5A5A5A5A5A5A5A).all()

    # S not a multiple of 32, S = K, S > K
    for bad in (31, 33, 16, K, K + 32, 2 ** 32 - 32):
        s = good.copy()
        s[1] = bad
        ps = s.ctypes.data
        assert words(C.byref(code), ps, n, pt0, pt1) == E_INVAL, bad
        for where in (TAIL, HEAD):
            assert to_llr4(C.byref(code), pl, HARD, 4, ps, where, n, p4) == E_INVAL, bad
            assert to_llr4(C.byref(code), pl, LLR4, 0, ps, where, n, p4) == E_INVAL, bad
            assert enc(C.byref(code), pc, circ50.size, pp, ps, where, n, pl, pb) == E_INVAL, bad
    ps = good.ctypes.data
    for where in (2, -1, 99):  # a bad `where`
        assert to_llr4(C.byref(code), pl, HARD, 4, ps, where, n, p4) == E_INVAL
        assert enc(C.byref(code), pc, circ50.size, pp, ps, where, n, pl, pb) == E_INVAL
    # NULL buffers, a NULL code, the rules of the line helpers
    assert to_llr4(C.byref(code), None, HARD, 4, ps, TAIL, n, p4) == E_INVAL
    assert to_llr4(C.byref(code), pl, HARD, 4, ps, TAIL, n, None) == E_INVAL
    assert to_llr4(None, pl, HARD, 4, ps, TAIL, n, p4) == E_INVAL
    assert to_llr4(C.byref(code), pl, 2, 4, ps, TAIL, n, p4) == E_INVAL
    assert to_llr4(C.byref(code), pl, HARD, 0, ps, TAIL, n, p4) == E_INVAL
    assert to_llr4(C.byref(code), pl, HARD, 8, ps, TAIL, n, p4) == E_INVAL
    assert enc(C.byref(code), pc, circ50.size, None, ps, TAIL, n, pl, pb) == E_INVAL
    assert enc(C.byref(code), pc, circ50.size, pp, ps, TAIL, n, None, pb) == E_INVAL
    assert enc(None, pc, circ50.size, pp, ps, TAIL, n, pl, pb) == E_INVAL
    assert enc(C.byref(code), None, circ50.size, pp, ps, TAIL, n, pl, pb) == E_INVAL
    assert enc(C.byref(code), pc, circ50.size - 1, pp, ps, TAIL, n, pl, pb) == E_INVAL
    assert words(None, ps, n, pt0, pt1) == E_INVAL
    broken = type(code)()
    C.memmove(C.byref(broken), C.byref(code), C.sizeof(code))
    broken.puncture_tail -= 8  # L no multiple of 32
    assert words(C.byref(broken), ps, n, pt0, pt1) == E_INVAL
    assert to_llr4(C.byref(broken), pl, HARD, 4, ps, TAIL, n, p4) == E_INVAL
    assert enc(C.byref(broken), pc, circ50.size, pp, ps, TAIL, n, pl, pb) == E_INVAL
    # n_codewords 0 is a no-op
    assert to_llr4(C.byref(code), None, HARD, 4, None, TAIL, 0, None) == 0
    assert enc(C.byref(code), pc, circ50.size, None, None, HEAD, 0, None, None) == 0
    untouched()
    assert words(C.byref(code), ps, n, pt0, None) == 0 and totals[0] == n * L - 288 and totals[1] == 0x5A5A5A5A5A5A5A5A


def test_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(4096, np.uint32)
    p = buf.ctypes.data
    for name in ("lnsfaid_decode_burst", "lnsfaid_decode_burst_device"):
        assert getattr(lib, name)(None, p, HARD, 4, None, TAIL, 1, p, None, None, None) == E_INVAL, name
        assert getattr(lib, name)(None, None, HARD, 4, None, TAIL, 0, None, None, None, None) == E_INVAL, name
    for name in ("lnsfaid_encode_burst", "lnsfaid_encode_burst_device"):
        assert getattr(lib, name)(None, p, None, TAIL, 1, p, None) == E_INVAL, name
        assert getattr(lib, name)(None, None, None, TAIL, 0, None, None) == E_INVAL, name


# ---- the ABI surface ----
_CTYPES = {"int32_t": C.c_int32, "size_t": C.c_size_t}  # every pointer but the code struct's is a void pointer in pyabi


def _header_prototype(name):
    header = open(os.path.join(ROOT, "include", "lnsfaid.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    types = []
    for arg in m.group(1).split(","):
        t = re.sub(r"\s*\b\w+\s*$", "", " ".join(arg.split()))  # drop the parameter's name
        types.append(t.replace(" *", "*"))
    return types


@pytest.mark.parametrize("name", sorted(NEW_SYMBOLS))
def test_abi_surface(abi, lib, name):
    assert getattr(lib, name) is not None
    res, args = abi.SYMBOLS[name]
    assert res is C.c_int
    want = []
    for t in _header_prototype(name):
        if t == "const lnsfaid_code*":
            want.append(C.POINTER(abi.Code))
        elif t.endswith("*"):
            want.append(C.c_void_p)
        else:
            want.append(_CTYPES[t])
    assert args == want, (name, args, want)
    assert len(args) == NEW_SYMBOLS[name]


def test_constants_and_methods(abi):
    assert (abi.SHORTEN_TAIL, abi.SHORTEN_HEAD) == (TAIL, HEAD) == (0, 1)
    header = open(os.path.join(ROOT, "include", "lnsfaid.h")).read()
    assert re.search(r"#define LNSFAID_SHORTEN_TAIL 0\b", header) and re.search(r"#define LNSFAID_SHORTEN_HEAD 1\b", header)
    for m in ("decode_burst", "decode_burst_device", "encode_burst", "encode_burst_device"):
        assert callable(getattr(abi.Decoder, m))
    for f in ("burst_words", "burst_to_llr4", "encode_burst_host"):
        assert callable(getattr(abi, f))


def test_stand_alone_program_under_the_sanitizers(tmp_path, circ50):
    """host/burst_selftest.cpp: the three host forms on heap buffers of exactly the documented sizes at odd addresses, built with the
    Makefile's $(SANITIZE) flags (address and undefined behaviour) and run as a process of its own"""
    path = tmp_path / "circ.bin"
    circ50.tofile(str(path))
    subprocess.check_call(["make", "-C", HOST, "burst_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "burst_selftest"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "burst_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- build-time properties of the two new kernel files ----
def _compile(tmp, name):
    out = tmp / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, name + ".hip")], check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("isa_burst")
    return {name: _compile(tmp, name) for name in ("lnsfaid_kernel4b", "lnsfaid_kernel4l", "lnsfaid_encoder_burst")}


def _instances(asm, kernel):
    """template arguments (the mangled <METHOD, RM, EF2>) -> (vgpr_count, vgpr_spill_count, private_segment_fixed_size)"""
    out = {}
    for name, m in kernel_meta(asm).items():
        if kernel in name:
            out[re.search(r"kernelI(\w+?)EEv", name).group(1)] = m
    return out


def test_decode_instances_against_the_line_kernel(isa):
    """all twelve instances, each without scratch and without spills, and with no more vector registers than the line kernel's
    instance of the same template arguments compiled here - which is what keeps two waves per SIMD (at most 256)"""
    burst = _instances(isa["lnsfaid_kernel4b"], "lnsfaid_decode4b_kernel")
    line = _instances(isa["lnsfaid_kernel4l"], "lnsfaid_decode4l_kernel")
    assert len(burst) == 12 and sorted(burst) == sorted(line), (sorted(burst), sorted(line))
    for inst, (vgpr, spill, scratch) in burst.items():
        print(inst, "burst", (vgpr, spill, scratch), "line", line[inst])
        assert spill == 0 and scratch == 0, (inst, spill, scratch)
        assert vgpr <= 256 and vgpr <= line[inst][0], (inst, vgpr, line[inst][0])


def test_decode_kernel_has_no_calls_and_scalar_descriptor(isa):
    asm = isa["lnsfaid_kernel4b"]
    parts = re.split(r"^(_Z\w+):", asm, flags=re.M)
    bodies = {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if "lnsfaid_decode4b_kernel" in parts[i]}
    assert len(bodies) == 12
    for name, body in bodies.items():
        calls = len(re.findall(r"s_swappc_b64", body))
        assert calls <= (2 if "ILi2ELb0ELb1E" in name else 0), (name, calls)  # <2, RM = false, EF2 = true>: the erasure plane
        # the descriptor is one 16-byte scalar load, in staging and again in the epilogue
        assert len(re.findall(r"s_load_dwordx4", body)) >= 2, name


def test_encode_kernel_resources(isa):
    meta = {n: m for n, m in kernel_meta(isa["lnsfaid_encoder_burst"]).items() if "lnsfaid_encode_burst_kernel" in n}
    assert len(meta) == 1
    (vgpr, spill, scratch), = meta.values()
    assert spill == 0 and scratch == 0 and vgpr <= 128, (vgpr, spill, scratch)
