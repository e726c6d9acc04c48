"""Times of the pre-FEC error counters (README "Pre-FEC error counters").

    python tools/gpu_prefec_time.py [--groups 2048]

The parent process starts every GPU step as a child under its own `timeout` and stops at the first step that fails
(tools/gpu_demap_time.py):
  prefec    lnsfaid_prefec_errors_device (whole codewords, sent bits on the device) for --groups groups resident in HBM, every
            mod_type with InterleaveModType 1 and QPSK with InterleaveModType 2, next to lnsfaid_demap_device (int8) on the same
            symbols in the same process: host clock around the synchronising call, median of 20 calls after 3 warm-up calls.
  frontend  lnsfaid_frontend_device, QPSK at Eb/N0 3.6 dB, --groups streams, with the fused counting off and on (the call
            copies seeds and draw counters and synchronises: the figures include that).  On a tree without the counters only the
            "off" figure is printed, so the same step times the parent commit.
Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
CASES = [(1, 1), (2, 1), (4, 1), (6, 1), (8, 1), (2, 2)]  # (mod_type, InterleaveModType)
SCALE = {1: 13.0, 2: 13.0, 4: 12.5, 6: 12.5, 8: 40.0}
RATE = 0.8444444


def _median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def _setup(groups):
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    pyabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pyabi)
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, groups, lib)
    return torch, pyabi, lib, code, dec


def step_prefec(groups):
    torch, pyabi, lib, code, dec = _setup(groups)
    n = groups * 32 * code.N
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sent = torch.randint(0, 2, (n,), dtype=torch.int8, device="cuda")
    for mod, il in CASES:
        floats = n if mod == 1 else 2 * (n // mod)
        d_rx = torch.randn(floats, dtype=torch.float32, device="cuda") * 0.6
        assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
        torch.cuda.synchronize()
        last = {}

        def count():
            last["c"] = dec.prefec_errors_device(d_rx.data_ptr(), groups, mod, d_sent.data_ptr(), pyabi.PREFEC_CODEWORD)
        ms, lo, hi = _median_ms(count)
        demap_ms, _, _ = _median_ms(lambda: dec.demap_device(d_rx.data_ptr(), groups, mod, SCALE[mod], d_out.data_ptr()))
        total = 4 * floats + n
        print(json.dumps({"step": "prefec", "groups": groups, "mod_type": mod, "interleave": il, "bytes_read": total,
                          "ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "GB_per_s": round(total / ms / 1e6, 1),
                          "demap_int8_ms": round(demap_ms, 3), "ratio_to_demap": round(ms / demap_ms, 3), "counters": last["c"]}), flush=True)
        del d_rx
    dec.close()


def step_frontend(groups):
    torch, pyabi, lib, code, dec = _setup(groups)
    sigma = 1.0 / math.sqrt(RATE * 2 * 10.0 ** 0.36)  # CSimulate::Configure at Eb/N0 3.6 dB, QPSK
    d_fix = torch.empty(groups * 32 * code.N, dtype=torch.int8, device="cuda")
    seeds = (C.c_uint32 * groups)(*[101 + 2 * i for i in range(groups)])
    draws = (C.c_uint64 * groups)(*([0] * groups))
    torch.cuda.synchronize()

    def call():
        assert lib.lnsfaid_frontend_device(dec.ctx, seeds, draws, groups, 2, sigma, 13.0, None, d_fix.data_ptr()) == 0
    row = {"step": "frontend", "streams": groups, "mod_type": 2, "eb_n0_db": 3.6}
    ms, lo, hi = _median_ms(call)
    row.update({"count_off_ms": round(ms, 3), "count_off_min_ms": round(lo, 3), "count_off_max_ms": round(hi, 3)})
    if hasattr(dec, "frontend_set_prefec"):
        dec.frontend_set_prefec(pyabi.PREFEC_INFO)
        ms, lo, hi = _median_ms(call)
        counters = dec.frontend_prefec_counters()
        dec.frontend_set_prefec(0)
        again, _, _ = _median_ms(call)
        row.update({"count_on_ms": round(ms, 3), "count_on_min_ms": round(lo, 3), "count_on_max_ms": round(hi, 3),
                    "count_off_again_ms": round(again, 3), "calls_counted": 23, "counters": counters})
    print(json.dumps(row), flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--step", choices=["prefec", "frontend"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return {"prefec": step_prefec, "frontend": step_frontend}[a.step](a.groups)
    for step in ("prefec", "frontend"):
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--groups", str(a.groups)]).returncode
        if rc != 0:
            print("step %s failed with exit status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
