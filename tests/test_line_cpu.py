"""Line-format decode without a GPU (include/lnsfaid.h "line-format decode"): the host helpers against the numpy
restatement of the formats (tests/line_ref.py), their error rules, the stand-alone sanitizer program, the build-time properties of
the line kernels (lnsfaid_kernel4l.hip) that tests/test_packed_io_isa.py holds for the packed twins, and the ABI surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import line_ref as lr
from test_fec_status_cpu import _toy_code
from test_kernel_isa import layer_loop_blocks
from test_packed_io_isa import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
E_INVAL = -1
NEW_SYMBOLS = ["lnsfaid_decode_line", "lnsfaid_decode_line_device", "lnsfaid_line_from_fixinput", "lnsfaid_line_to_llr4"]


def _dims(code50):
    N, M, K = code50.N, code50.M, code50.K
    return N, M, K, N - code50.code.puncture_tail


def _probed_frames(code50, n, seed):
    """LLRs over -8 .. 7 for the whole groups that hold n codewords, with probe values on both sides of K and of L in codewords 0 and
    31 of the first group (the two-segment layout) and in codeword 32"""
    N, M, K, L = _dims(code50)
    rng = np.random.default_rng(seed)
    frames = rng.integers(-8, 8, ((n + 31) // 32 * 32, N), dtype=np.int8)
    assert (frames == 0).any() and (frames == -8).any() and (frames == 7).any()
    probes = {0: 7, K - 1: -8, K: 1, L - 1: -1, L: 5}
    for c in (0, 31, 32):
        if c < frames.shape[0]:
            for k, v in probes.items():
                frames[c, k] = v
    return frames, probes


@pytest.mark.parametrize("n", [1, 31, 32, 33])
@pytest.mark.parametrize("fmt", [lr.HARD, lr.LLR4], ids=["hard", "llr4"])
def test_line_from_fixinput(abi, lib, code50, n, fmt):
    N, M, K, L = _dims(code50)
    frames, probes = _probed_frames(code50, n, 100 + n)
    fix = lr.group_layout(frames, K)
    line = abi.line_from_fixinput(code50.code, fix, n, fmt, lib)
    assert line.size == n * (L // 32 if fmt == lr.HARD else L // 2)
    assert np.array_equal(line, lr.line_of(frames[:n], L, fmt))
    for c in (0, 31, 32):
        if c >= n:
            continue
        for k, v in probes.items():
            if k >= L:
                continue
            if fmt == lr.HARD:
                assert (int(line[c * (L // 32) + k // 32]) >> (k % 32)) & 1 == int(v > 0), (c, k)
            else:
                nib = (int(line[c * (L // 2) + k // 2]) >> (4 * (k % 2))) & 15
                assert nib == v & 15, (c, k)
    # a difference in the punctured tail alone changes nothing, not even a value no nibble can hold
    other = frames.copy()
    other[:, L:] = 100
    assert np.array_equal(abi.line_from_fixinput(code50.code, lr.group_layout(other, K), n, fmt, lib), line)


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_line_to_llr4_hard_round_trip(abi, lib, code50, n):
    N, M, K, L = _dims(code50)
    frames, _ = _probed_frames(code50, n, 200 + n)
    line = abi.line_from_fixinput(code50.code, lr.group_layout(frames, K), n, lr.HARD, lib)
    for magnitude in (1, 4, 7):
        llr4 = abi.line_to_llr4(code50.code, line, lr.HARD, magnitude, n, lib)
        assert np.array_equal(llr4, lr.llr4_of_line(line, n, N, K, L, lr.HARD, magnitude))
        back = lr.frames_of(lr.unpack_nibbles(llr4), N, K)
        assert back.shape[0] == (n + 31) // 32 * 32
        # +-magnitude, 0 -> -magnitude; nibble 0 in the punctured tail and in the padding codewords
        assert np.array_equal(back[:n, :L], np.where(frames[:n, :L] > 0, magnitude, -magnitude))
        assert (frames[:n, :L] == 0).any()
        assert not back[:n, L:].any() and not back[n:].any()


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_line_to_llr4_soft_round_trip(abi, lib, code50, n):
    N, M, K, L = _dims(code50)
    frames, _ = _probed_frames(code50, n, 300 + n)
    line = abi.line_from_fixinput(code50.code, lr.group_layout(frames, K), n, lr.LLR4, lib)
    llr4 = abi.line_to_llr4(code50.code, line, lr.LLR4, 0, n, lib)  # magnitude is ignored
    assert np.array_equal(llr4, lr.llr4_of_line(line, n, N, K, L, lr.LLR4, 0))
    back = lr.frames_of(lr.unpack_nibbles(llr4), N, K)
    assert np.array_equal(back[:n, :L], frames[:n, :L])  # the identity below L, -8 included
    assert not back[:n, L:].any() and not back[n:].any()
    # for whole groups: the llr4 of the packed decode I/O with the tail set to 0
    if n % 32 == 0:
        erased = frames.copy()
        erased[:, L:] = 0
        assert np.array_equal(llr4, abi.pack_llr4(lr.group_layout(erased, K), lib))


def test_error_rules(abi, lib, code50):
    N, M, K, L = _dims(code50)
    code = code50.code
    n = 2
    frames, _ = _probed_frames(code50, n, 7)
    fix = lr.group_layout(frames, K)
    line = np.full(n * L // 2, 0x5A, np.uint8)
    llr4 = np.full(32 * N // 2, 0x5A, np.uint8)
    from_fix, to_llr4 = lib.lnsfaid_line_from_fixinput, lib.lnsfaid_line_to_llr4
    for fmt in (-1, 2):
        assert from_fix(C.byref(code), fix.ctypes.data, n, fmt, line.ctypes.data) == E_INVAL
        assert to_llr4(C.byref(code), line.ctypes.data, fmt, 4, n, llr4.ctypes.data) == E_INVAL
    for magnitude in (0, 8, -4):
        assert to_llr4(C.byref(code), line.ctypes.data, lr.HARD, magnitude, n, llr4.ctypes.data) == E_INVAL
    assert from_fix(None, fix.ctypes.data, n, lr.HARD, line.ctypes.data) == E_INVAL
    assert from_fix(C.byref(code), None, n, lr.HARD, line.ctypes.data) == E_INVAL
    assert from_fix(C.byref(code), fix.ctypes.data, n, lr.HARD, None) == E_INVAL
    assert to_llr4(C.byref(code), None, lr.HARD, 4, n, llr4.ctypes.data) == E_INVAL
    assert to_llr4(C.byref(code), line.ctypes.data, lr.HARD, 4, n, None) == E_INVAL
    # a code with L or K not a multiple of 32
    for field, value in (("puncture_tail", code.puncture_tail - 16), ("n_check", code.n_check + 16)):
        broken = abi.Code.from_buffer_copy(code)
        setattr(broken, field, value)
        assert from_fix(C.byref(broken), fix.ctypes.data, n, lr.HARD, line.ctypes.data) == E_INVAL, field
        assert to_llr4(C.byref(broken), line.ctypes.data, lr.LLR4, 0, n, llr4.ctypes.data) == E_INVAL, field
    toy, keep = _toy_code(abi)  # 30 bits, 15 checks, a tail of 3: L = 27, K = 15
    assert from_fix(C.byref(toy), fix.ctypes.data, 1, lr.HARD, line.ctypes.data) == E_INVAL
    assert to_llr4(C.byref(toy), line.ctypes.data, lr.HARD, 4, 1, llr4.ctypes.data) == E_INVAL
    # every refused call left the outputs alone
    assert (line == 0x5A).all() and (llr4 == 0x5A).all()
    # n_codewords 0: a no-op, NULL buffers allowed
    assert from_fix(C.byref(code), None, 0, lr.LLR4, None) == 0 and to_llr4(C.byref(code), None, lr.HARD, 4, 0, None) == 0
    # a transmitted value outside -8 .. 7 (LLR4 only: HARD takes the sign of any int8)
    for bad in (8, -9, 127, -128):
        f = frames.copy()
        f[1, L - 1] = bad
        assert from_fix(C.byref(code), lr.group_layout(f, K).ctypes.data, n, lr.LLR4, line.ctypes.data) == E_INVAL, bad
        assert from_fix(C.byref(code), lr.group_layout(f, K).ctypes.data, n, lr.HARD, line.ctypes.data) == 0


def test_entry_points_refuse_a_null_context(lib):
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    for name in ("lnsfaid_decode_line", "lnsfaid_decode_line_device"):
        assert getattr(lib, name)(None, p, lr.HARD, 4, 1, p, None, None) == E_INVAL, name
        assert getattr(lib, name)(None, None, lr.HARD, 4, 0, None, None, None) == E_INVAL, name


def test_stand_alone_program_under_the_sanitizers():
    """host/line_selftest.cpp: the helpers on heap buffers of exactly the documented sizes, built with the Makefile's $(SANITIZE)
    flags (address and undefined behaviour) and run as a process of its own"""
    subprocess.check_call(["make", "-C", HOST, "line_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "line_selftest")], capture_output=True, text=True)
    assert r.returncode == 0 and "line_selftest: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


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
    assert len(args) == {"lnsfaid_decode_line": 8, "lnsfaid_decode_line_device": 8, "lnsfaid_line_from_fixinput": 5,
                         "lnsfaid_line_to_llr4": 6}[name]


def test_line_stats_record(abi):
    assert abi.line_stats_dtype().itemsize == C.sizeof(abi.LineStats) == 16
    assert abi.line_stats_dtype().names == ("iterations", "bf_iterations", "unsatisfied", "corrected")
    assert (abi.LINE_HARD, abi.LINE_LLR4) == (lr.HARD, lr.LLR4) == (0, 1)


# ---- build-time properties of the line kernels ----
DECODER = "lnsfaid_decode4l_kernel"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa4l") / "kernel4l.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4l.hip")], check=True, capture_output=True)
    return out.read_text()


def _bodies(asm):
    parts = re.split(r"^(_Z\w+):", asm, flags=re.M)
    return {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if DECODER in parts[i]}


def test_every_instance_is_built(asm):
    # DecodeMethod 0 (HBM), 1..5 x {registers, HBM}, the erasing EF_ELIMINATION 2 instance: one set for both formats
    assert len(_bodies(asm)) == 12, sorted(_bodies(asm))


def test_no_scratch_no_spills_two_waves_per_simd(asm):
    meta = {n: m for n, m in kernel_meta(asm).items() if DECODER in n}
    assert len(meta) == 12, sorted(meta)
    for name, (vgpr, spill, scratch) in meta.items():
        assert vgpr <= 256 and spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


def test_no_function_calls_on_the_hot_path(asm):
    funcs = [m for m in re.findall(r"^(_Z\w+):", asm, flags=re.M) if DECODER not in m]
    assert all("build_erasure_plane4" in f for f in funcs), funcs
    for name, body in _bodies(asm).items():
        calls = len(re.findall(r"s_swappc_b64", body))
        assert calls <= (2 if "ILi2ELb0ELb1E" in name else 0), (name, calls)  # <2, RM = false, EF2 = true>: the erasure plane


def test_registers_instances_have_no_memory_traffic_in_the_layer_loop(asm):
    bodies = {n: b for n, b in _bodies(asm).items() if "Lb1ELb0E" in n}
    assert len(bodies) == 5, sorted(bodies)
    for name, body in bodies.items():
        loop = layer_loop_blocks(body)
        ops = [i for b in loop for i in b[2]]
        assert sum(len(b[2]) for b in loop) > 1500, name
        stores = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_store", i)]
        loads = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_load", i)]
        assert not stores, (name, stores)
        assert len(loads) <= 1 and all(i.startswith("global_load_dword ") for i in loads), (name, loads)


def test_staging_keeps_a_round_of_column_loads_in_flight(asm):
    # both formats: 23 loads per round before the first wait - words of bits (HARD), half-words of nibbles (LLR4)
    for name, body in _bodies(asm).items():
        lines = [l.strip() for l in body.split("\n") if re.match(r"^\s+[a-z]", l)]
        for op in ("global_load_dword ", "global_load_ushort "):
            run, best = 0, 0
            for l in lines:
                if l.startswith(op):
                    run += 1
                    best = max(best, run)
                elif l.startswith("s_waitcnt") and "vmcnt" in l:
                    run = 0
            assert best >= 23, (name, op, best)
