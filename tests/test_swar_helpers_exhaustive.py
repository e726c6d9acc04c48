"""The helpers of csrc/lnsfaid_swar.h that were rewritten to issue fewer instructions, each against the formulation it replaced
(kept in the header as the definition) over its WHOLE input domain - not over samples: thermometer code -> number for all 8^4
dwords; the merged clamp / update of one edge for every V2C t in [-38, 38], every magnitude c in 0..7, both signs of the old
message, both values of the row mask, the FAID and the min-sum family, in every byte position (also against the decoder's own
statement sat31(sat31(t) + L)); the minimum search over a group of four edges against the edge-by-edge chain for every running
pair and every four codes; the sign words of pass 2.  tests/swar_helpers_exhaustive.cpp is the host program; no GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")


def test_rewritten_helpers_equal_the_ones_they_replace(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "swar_helpers_exhaustive"
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "swar_helpers_exhaustive.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "total mismatches: 0", lines[-1]
    for name in ("therm2num", "update<FAID>", "update<min-sum>", "min_quad", "sign_quad<23>", "sign_quad<22>", "sign_quad<24>"):
        assert any(l.startswith(name + ":") and l.endswith(" 0 mismatches") for l in lines), (name, lines)
