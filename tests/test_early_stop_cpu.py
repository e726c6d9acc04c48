"""The per-codeword early stop without a GPU: the properties of its kernel instances (lnsfaid_kernel4cw.hip, cross-compiled to
gfx950 assembly) and the host H x reference the GPU tests compare lnsfaid_codeword_stats.unsatisfied with."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_abi as oa
from early_stop_ref import unsatisfied
from test_kernel_isa import CSRC, HIPCC, ROOT, layer_loop_blocks


@pytest.fixture(scope="module")
def kernel4cw_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "kernel4cw.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "lnsfaid_kernel4cw.hip")], check=True, capture_output=True)
    return out.read_text()


def cw_bodies(asm):
    parts = re.split(r"^(_Z\w+):", asm, flags=re.M)
    return {parts[i]: parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if "lnsfaid_decode4cw_kernel" in parts[i]}


def test_every_instance_of_the_group_rule_kernel_has_a_per_codeword_one(kernel4cw_asm):
    names = sorted(cw_bodies(kernel4cw_asm))
    # methods 0..5 streamed through HBM, 1..5 with the messages in registers, the erasing instance of EF_ELIMINATION 2
    want = ["ILi0ELb0ELb0E"] + ["ILi%dELb%dELb0E" % (m, rm) for m in range(1, 6) for rm in (0, 1)] + ["ILi2ELb0ELb1E"]
    assert len(names) == len(want) and all(any(w in n for n in names) for w in want), names


def test_no_scratch_no_spills_and_two_waves_per_simd(kernel4cw_asm):
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", kernel4cw_asm)]
    assert sizes and all(s == 0 for s in sizes), sizes
    vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s*(\d+)", kernel4cw_asm)]
    assert vgprs and max(vgprs) <= 256, vgprs
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", kernel4cw_asm))
    funcs = [m for m in re.findall(r"^(_Z\w+):", kernel4cw_asm, flags=re.M) if "lnsfaid_decode4cw_kernel" not in m]
    assert all("build_erasure_plane4" in f for f in funcs), funcs


def test_messages_in_registers_means_no_memory_traffic_in_the_layer_loop(kernel4cw_asm):
    bodies = {n: b for n, b in cw_bodies(kernel4cw_asm).items() if "Lb1ELb0E" in n}
    assert len(bodies) == 5, sorted(bodies)
    for name, body in bodies.items():
        loop = layer_loop_blocks(body)
        ops = [i for b in loop for i in b[2]]
        assert len(ops) > 1500, name
        stores = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_store", i)]
        loads = [i for i in ops if re.match(r"(global|flat|buffer|scratch)_load", i)]
        assert not stores, (name, stores)
        assert len(loads) <= 1 and all(i.startswith("global_load_dword ") for i in loads), (name, loads)
        assert any("s_set_gpr_idx_on" in i for i in ops), name


def _golden_codeword(code50):
    packed = np.fromfile(os.path.join(ROOT, "tests", "golden", "codeword_50gpon.bin"), dtype=np.uint8)
    return np.unpackbits(packed)[:code50.N].astype(np.int8)


def test_host_syndrome_count(abi, lib, code50):
    """H x of the golden codeword is 0; a flipped bit breaks exactly the checks it is in; several flips the odd-covered ones
    (compared with a per-row count written out plainly)"""
    from early_stop_ref import check_rows
    cw = _golden_codeword(code50)
    pos, starts = check_rows(code50)
    rows = np.split(pos, starts[1:])
    assert len(rows) == code50.M
    rng = np.random.default_rng(5)
    frames = [cw.copy()]
    for nflip in (1, 2, 3, 40, 500):
        f = cw.copy()
        f[rng.choice(code50.N, nflip, replace=False)] ^= 1
        frames.append(f)
    frames.append(np.zeros(code50.N, np.int8))
    frames.append(np.ones(code50.N, np.int8))
    got = unsatisfied(code50, np.stack(frames))
    plain = [sum(int(f[r].sum() & 1) for r in rows) for f in frames]
    assert got.tolist() == plain
    assert got[0] == 0 and got[-2] == 0
    col_weight = np.bincount(pos, minlength=code50.N)
    flipped = np.nonzero(frames[1] != cw)[0][0]
    assert got[1] == col_weight[flipped]


def test_host_syndrome_agrees_with_the_oracle_stop(abi, lib, code50):
    """the oracle stops a group at decision point 1 (I = 0) exactly when the channel's hard decisions of all its lanes are a
    codeword: the host count of those decisions is 0 for such groups and not for the others"""
    cfg = abi.default_cfg(2, 10)
    fix = oa.ReferenceChannel(code50, 101, 13.0).groups(6.0, 2)  # strong channel: some frames arrive clean
    from early_stop_ref import replicate
    rep = replicate(code50, fix, 2, cws=list(range(8)))
    _, st = oa.decode_mt(code50, cfg, rep, 8)
    N, K, M = code50.N, code50.K, code50.M
    f = fix.reshape(2, 32 * N)[0]
    hard = np.concatenate([f[:32 * K].reshape(32, K), f[32 * K:].reshape(32, M)], axis=1)[:8]
    hard = (hard < 0).astype(np.int8)  # LLR sign; the punctured tail is erased, its decisions are 0
    hard[:, N - code50.code.puncture_tail:] = 0
    u = unsatisfied(code50, hard)
    assert ((u == 0) == (st[:, 0] == 0)).all(), (u.tolist(), st.tolist())
