"""Build-time properties of the packed decoders (lnsfaid_kernel4p.hip) that the int8 four-rows kernels also hold
(tests/test_kernel_isa.py): no scratch, at most 256 VGPRs (two waves per SIMD), no spills, no calls on the hot
path, and for the messages-in-registers instances no vector memory in the layer loop but the edge-table prefetch.
Cross-compiles to gfx950 assembly; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_isa import layer_loop_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DECODERS = ("lnsfaid_decode4p_kernel", "lnsfaid_decode4pcw_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa4p") / "kernel4p.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4p.hip")], check=True, capture_output=True)
    return out.read_text()


def kernel_meta(asm):
    """kernel symbol -> (vgpr_count, vgpr_spill_count, private_segment_fixed_size) from the code-object metadata"""
    meta = {}
    for block in re.split(r"^\s+- \.agpr_count:", asm, flags=re.M)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = (int(re.search(r"\.vgpr_count:\s*(\d+)", block).group(1)),
                      int(re.search(r"\.vgpr_spill_count:\s*(\d+)", block).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)))
    return meta


def decoder_bodies(asm):
    parts = re.split(r"^(_Z\w+):", asm, flags=re.M)
    return {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2)
            if any(d in parts[i] for d in DECODERS)}


def test_every_instance_is_built(asm):
    bodies = decoder_bodies(asm)
    for d in DECODERS:
        # DecodeMethod 0 (HBM), 1..5 x {registers, HBM}, the erasing EF_ELIMINATION 2 instance
        assert sum(1 for n in bodies if d in n) == 12, sorted(n for n in bodies if d in n)


def test_no_scratch_no_spills_two_waves_per_simd(asm):
    meta = {n: m for n, m in kernel_meta(asm).items() if any(d in n for d in DECODERS)}
    assert len(meta) == 24, sorted(meta)
    for name, (vgpr, spill, scratch) in meta.items():
        assert vgpr <= 256 and spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


def test_no_function_calls_on_the_hot_path(asm):
    funcs = [m for m in re.findall(r"^(_Z\w+):", asm, flags=re.M) if not any(d in m for d in DECODERS) and "Kernel" not in m]
    funcs = [f for f in funcs if "kernel" not in f]
    assert all("build_erasure_plane4" in f for f in funcs), funcs
    for name, body in decoder_bodies(asm).items():
        calls = len(re.findall(r"s_swappc_b64", body))
        assert calls <= (2 if "ILi2ELb0ELb1E" in name else 0), (name, calls)  # <2, RM = false, EF2 = true>: the erasure plane


def test_registers_instances_have_no_memory_traffic_in_the_layer_loop(asm):
    bodies = {n: b for n, b in decoder_bodies(asm).items() if "Lb1ELb0E" in n}
    assert len(bodies) == 10, sorted(bodies)
    for name, body in bodies.items():
        loop = layer_loop_blocks(body)
        ops = [i for b in loop for i in b[2]]
        assert sum(len(b[2]) for b in loop) > 1500, name
        stores = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_store", i)]
        loads = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_load", i)]
        assert not stores, (name, stores)
        assert len(loads) <= 1 and all(i.startswith("global_load_dword ") for i in loads), (name, loads)


def test_staging_keeps_a_round_of_column_loads_in_flight(asm):
    # 23 half-word loads per round before the first wait, as the int8 staging issues 23 dword loads
    for name, body in decoder_bodies(asm).items():
        lines = [l.strip() for l in body.split("\n") if re.match(r"^\s+[a-z]", l)]
        run, best = 0, 0
        for l in lines:
            if l.startswith("global_load_ushort"):
                run += 1
                best = max(best, run)
            elif l.startswith("s_waitcnt") and "vmcnt" in l:
                run = 0
        assert best >= 23, (name, best)
