"""The paired mask expanders of csrc/lnsfaid_swar.h (sw_mask7x2, sw_zero_mask2: one 64-bit shift serves two words)
against two calls of sw_mask7 / sw_zero_mask: every byte value in every byte position of either word, all 256 values of the first
word's top byte - the one foreign byte in what the second word's expander reads - against the sign patterns of the bytes next to it,
both argument orders.  tests/mask_pairs_exhaustive.cpp is the host program; it is built once plainly and once with the address and
undefined-behaviour sanitizers.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
CHECKS = ("mask7 definition", "mask7x2 every byte", "mask7x2 foreign byte", "zero_mask2", "shl8x2 halves")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_paired_expanders_equal_two_single_ones(tmp_path, flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "mask_pairs_exhaustive"
    subprocess.run([gxx, *flags, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "mask_pairs_exhaustive.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "total mismatches: 0", lines[-1]
    for name in CHECKS:
        assert any(l.startswith(name + ":") and l.endswith(" 0 mismatches") for l in lines), (name, lines)
