"""Line-format encode without a GPU (include/lnsfaid.h "line-format encode"): lnsfaid_encode_line_host - the
definition of what the device calls return - against the independent numpy encoder (tests/gf2_encoder.py) in the formats of
tests/line_ref.py, its error rules, the stand-alone sanitizer program, the ABI surface and the build-time properties of the kernel
(lnsfaid_encoder_line.hip)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import encode_line_ref as el
import line_ref as lr
from test_fec_status_cpu import _toy_code
from test_line_cpu import _CTYPES, _header_prototype
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL, E_CODE = -1, -2
NEW_SYMBOLS = ["lnsfaid_encode_line", "lnsfaid_encode_line_device", "lnsfaid_encode_line_host"]
KERNEL = "lnsfaid_encode_line_kernel"


@pytest.fixture(scope="module")
def circ50(abi, lib, code50):
    return abi.code_parity_inverse(code50.code, lib)


def _dims(code):
    return code.n_var, code.n_var - code.n_check, code.n_var - code.puncture_tail


@pytest.mark.parametrize("with_bits", [False, True], ids=["line", "line+bits"])
@pytest.mark.parametrize("n", [1, 31, 33])
def test_host_form_equals_the_numpy_encoder(abi, lib, code50, encoder, circ50, n, with_bits):
    payload, want_line, want_bits = el.batch(encoder, "random", n, 1000 * n)
    assert payload.any(axis=1).all() and want_line[:, payload.shape[1]:].any(axis=1).all()  # never the all-zero word
    line, bits = abi.encode_line_host(code50.code, payload, n, with_bits, lib, circ50)
    assert line.shape == want_line.shape and np.array_equal(line, want_line)
    assert np.array_equal(line[:, :payload.shape[1]], payload)
    if with_bits:
        assert np.array_equal(bits, want_bits) and np.array_equal(bits[:, :line.shape[1]], line)
    else:
        assert bits is None


def test_unit_vectors(abi, lib, code50, encoder, circ50):
    """one information bit per codeword, in a different block column and at a different rotation each: a wrong shift, block column or
    rotation direction shows here"""
    payload, want_line, want_bits = el.batch(encoder, "unit")
    assert payload.shape[0] == 57 and (np.unpackbits(payload.view(np.uint8), axis=1).sum(axis=1) == 1).all()
    line, bits = abi.encode_line_host(code50.code, payload, 57, True, lib, circ50)
    bad = np.nonzero((bits != want_bits).any(axis=1))[0]
    assert bad.size == 0, bad.tolist()
    assert np.array_equal(line, want_line)
    # codewords of different block columns differ in their parity bits
    assert len({row.tobytes() for row in line[:, payload.shape[1]:]}) == 57


def test_known_answer(abi, lib, code50, circ50):
    """the reference's own codeword: its first K bits encode to its first L bits, and with bits to all N"""
    N, K, L = _dims(code50.code)
    cw = el.golden_codeword(N)
    payload = lr.payload_of(cw[None, :K])
    line, bits = abi.encode_line_host(code50.code, payload, 1, True, lib, circ50)
    assert np.array_equal(line, lr.line_of(cw[None, :].astype(np.int8), L, lr.HARD).reshape(1, -1))
    assert np.array_equal(np.unpackbits(bits.view(np.uint8), bitorder="little"), cw)
    line_only, none = abi.encode_line_host(code50.code, payload, 1, False, lib, circ50)
    assert none is None and np.array_equal(line_only, line)


def test_bits_are_codewords_for_fec_status(abi, lib, code50, encoder, circ50):
    n = 33
    N, K, L = _dims(code50.code)
    payload, _, _ = el.batch(encoder, "random", n, 1000 * n)
    line, bits = abi.encode_line_host(code50.code, payload, n, True, lib, circ50)
    padded = np.zeros((64, N // 32), np.uint32)
    padded[:n] = bits
    llr4 = abi.line_to_llr4(code50.code, line.reshape(-1), lr.HARD, 4, n, lib)
    rec, out, _ = abi.fec_status_packed_host(code50.code, llr4, padded.reshape(-1), None, 2, lib=lib)
    assert not rec["unsatisfied"].any(), rec["unsatisfied"].tolist()
    assert not rec["corrected"][:n].any()  # the line is the first L bits of every codeword
    assert out[1] == 0


def test_derived_code(abi, lib):
    """any quasi-cyclic code: block columns 67 and 68 dropped from block rows 2 and up, against that code's own numpy encoder"""
    dc, enc = el.derived(abi, lib)
    N, K, L = _dims(dc.code)
    n = 3
    payload, want_line, want_bits = el.expected(enc, el.messages(n, K, 77), L)
    line, bits = abi.encode_line_host(dc.code, payload, n, True, lib)
    assert np.array_equal(line, want_line) and np.array_equal(bits, want_bits)


def test_error_rules(abi, lib, code50, circ50):
    code = code50.code
    N, K, L = _dims(code)
    n = 2
    payload = np.random.default_rng(5).integers(0, 1 << 32, n * K // 32, dtype=np.uint64).astype(np.uint32)
    line, bits = np.full(n * L // 32, 0x5A5A5A5A, np.uint32), np.full(n * N // 32, 0x5A5A5A5A, np.uint32)
    fn = lib.lnsfaid_encode_line_host
    pc, pp, pl, pb = circ50.ctypes.data, payload.ctypes.data, line.ctypes.data, bits.ctypes.data
    assert fn(None, pc, circ50.size, pp, n, pl, pb) == E_INVAL
    assert fn(C.byref(code), None, circ50.size, pp, n, pl, pb) == E_INVAL
    assert fn(C.byref(code), pc, circ50.size - 1, pp, n, pl, pb) == E_INVAL
    assert fn(C.byref(code), pc, 0, pp, n, pl, pb) == E_INVAL
    assert fn(C.byref(code), pc, circ50.size, None, n, pl, pb) == E_INVAL
    assert fn(C.byref(code), pc, circ50.size, pp, n, None, pb) == E_INVAL
    # a code with L, K or N not a multiple of 32, or with information bits in the punctured tail
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16), ("puncture_tail", code.n_check + 32)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert fn(C.byref(broken), pc, circ50.size, pp, n, pl, pb) == E_INVAL, (field, value)
    toy, keep = _toy_code(abi)  # 30 bits, 15 checks, a tail of 3
    assert fn(C.byref(toy), pc, circ50.size, pp, 1, pl, pb) == E_INVAL
    # every refused call left the outputs alone
    assert (line == 0x5A5A5A5A).all() and (bits == 0x5A5A5A5A).all()
    # n_codewords 0: a no-op, NULL buffers allowed (circ is not one of them)
    assert fn(C.byref(code), pc, circ50.size, None, 0, None, None) == 0
    assert fn(C.byref(code), pc, circ50.size, pp, 0, pl, pb) == 0
    assert fn(C.byref(code), None, circ50.size, None, 0, None, None) == E_INVAL
    assert (line == 0x5A5A5A5A).all() and (bits == 0x5A5A5A5A).all()
    # and with the arguments right it writes exactly n codewords of each output
    wide_l, wide_b = np.full((n + 1) * L // 32, 0x5A5A5A5A, np.uint32), np.full((n + 1) * N // 32, 0x5A5A5A5A, np.uint32)
    assert fn(C.byref(code), pc, circ50.size, pp, n, wide_l.ctypes.data, wide_b.ctypes.data) == 0
    assert (wide_l[n * L // 32:] == 0x5A5A5A5A).all() and (wide_b[n * N // 32:] == 0x5A5A5A5A).all()
    assert not (wide_l[:n * L // 32] == 0x5A5A5A5A).any() and not (wide_b[:n * N // 32] == 0x5A5A5A5A).any()
    # the singular derived code has no inverse to pass
    with pytest.raises(ValueError, match="-2"):
        import encoder_ref as er
        abi.code_parity_inverse(er.derived_code(abi, lib, [68], 11).code, lib)


def test_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(1 << 12, np.uint32)
    p = buf.ctypes.data
    for name in ("lnsfaid_encode_line", "lnsfaid_encode_line_device"):
        assert getattr(lib, name)(None, p, 1, p, None) == E_INVAL, name
        assert getattr(lib, name)(None, None, 0, None, None) == E_INVAL, name
    assert not buf.any()


def test_stand_alone_program_under_the_sanitizers(tmp_path, circ50):
    """host/encode_line_selftest.cpp: lnsfaid_encode_line_host on heap buffers of exactly the documented sizes, every row of H checked
    against `bits` by the program itself, built with the Makefile's $(SANITIZE) flags and run as a process of its own.  B^-1 comes
    from this (unsanitised) process through a file."""
    path = tmp_path / "circ.bin"
    circ50.tofile(str(path))
    subprocess.check_call(["make", "-C", HOST, "encode_line_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "encode_line_selftest"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "encode_line_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the ABI surface ----
@pytest.mark.parametrize("name", NEW_SYMBOLS)
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
    assert len(args) == {"lnsfaid_encode_line": 5, "lnsfaid_encode_line_device": 5, "lnsfaid_encode_line_host": 7}[name]


# ---- build-time properties of the kernel ----
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa_enl") / "encoder_line.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_encoder_line.hip")], check=True, capture_output=True)
    return out.read_text()


def test_kernel_resources(asm):
    """no scratch, no spills, no function calls, 256 threads, eight waves per SIMD"""
    meta = {n: m for n, m in kernel_meta(asm).items() if KERNEL in n}
    assert len(meta) == 1, sorted(meta)
    (name, (vgpr, spill, scratch)), = meta.items()
    assert vgpr <= 64 and spill == 0 and scratch == 0, (vgpr, spill, scratch)
    funcs = re.findall(r"^(_Z\w+):", asm, flags=re.M)
    assert funcs == [name], funcs
    assert "s_swappc_b64" not in asm and "s_setpc_b64" not in asm
    block = [b for b in re.split(r"^\s+- \.agpr_count:", asm, flags=re.M)[1:] if name in b][0]
    assert int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", block).group(1)) == 256
    assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1)) == 0  # all LDS is dynamic


def test_kernel_moves_sixteen_bytes_per_lane(asm):
    """the payload comes in and the information words leave as 16-byte accesses; the parity words leave as whole words"""
    body = asm  # the file holds this one kernel (test_kernel_resources)
    assert len(re.findall(r"^\s+global_load_dwordx4 ", body, flags=re.M)) == 2  # the first round, and a round ahead in the loop
    assert len(re.findall(r"^\s+global_store_dwordx4 ", body, flags=re.M)) == 2  # line, bits
    assert len(re.findall(r"^\s+global_store_dword ", body, flags=re.M)) == 2
    assert not re.findall(r"^\s+global_store_(byte|short)", body, flags=re.M)


def test_lds_size_fits_without_a_launch_attribute(lib, code50):
    lib.lf_encode_line_lds_bytes.restype, lib.lf_encode_line_lds_bytes.argtypes = C.c_size_t, [C.c_int]
    assert 4 * code50.M < lib.lf_encode_line_lds_bytes(code50.M) <= 65536
    assert lib.lf_encode_line_lds_bytes(32 * 256) <= 65536  # the largest code lnsfaid_create accepts (32 block rows)
