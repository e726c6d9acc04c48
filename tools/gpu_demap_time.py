"""Times of the demapper for received symbols (README "Received symbols in, bits out").

    python tools/gpu_demap_time.py [--groups 2048]

The parent process starts every GPU step as a child under its own `timeout` and stops at the first step that fails
(tools/gpu_encode_time.py):
  demap   lnsfaid_demap_device and lnsfaid_demap_packed_device for --groups groups resident in HBM, every mod_type with
          InterleaveModType 1 and QPSK with InterleaveModType 2: host clock around the synchronising call, median of 20 calls
          after 3 warm-up calls.  Beside each figure the time of a device-to-device copy that moves the same total byte count
          (it copies (bytes read + bytes written) / 2, so that it reads and writes as much as the call together), same process.
  chain   symbols in HBM -> lnsfaid_demap_packed_device + lnsfaid_decode_packed_device + lnsfaid_count_errors_packed_device
          (QPSK, all-zero codeword at Eb/N0 3.0 dB, DecodeMethod 2, 10 iterations) next to decode + counters alone on the LLRs
          the first call left.
Prints one JSON line per measurement."""
import argparse
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
    return t[len(t) // 2]


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


def step_demap(groups):
    torch, pyabi, lib, code, dec = _setup(groups)
    n = groups * 32 * code.N
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    for mod, il in CASES:
        floats = n if mod == 1 else 2 * (n // mod)
        d_rx = torch.randn(floats, dtype=torch.float32, device="cuda") * 0.6
        assert lib.lnsfaid_frontend_set_interleave(dec.ctx, il) == 0
        for packed in (False, True):
            out_bytes = n // 2 if packed else n
            call = dec.demap_packed_device if packed else dec.demap_device
            torch.cuda.synchronize()
            ms = _median_ms(lambda: call(d_rx.data_ptr(), groups, mod, SCALE[mod], d_out.data_ptr()))
            total = 4 * floats + out_bytes
            src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty(total // 2, dtype=torch.uint8, device="cuda")

            def copy():
                dst.copy_(src)
                torch.cuda.synchronize()
            copy_ms = _median_ms(copy)
            print(json.dumps({"step": "demap", "groups": groups, "mod_type": mod, "interleave": il, "output": "llr4" if packed else "int8",
                              "bytes_read": 4 * floats, "bytes_written": out_bytes, "ms": round(ms, 3),
                              "GB_per_s": round(total / ms / 1e6, 1), "copy_same_bytes_ms": round(copy_ms, 3),
                              "copy_GB_per_s": round(total / copy_ms / 1e6, 1), "share_of_copy_rate": round(copy_ms / ms, 3)}), flush=True)
            del src, dst
        del d_rx
    dec.close()


def step_chain(groups):
    torch, pyabi, lib, code, dec = _setup(groups)
    n = groups * 32 * code.N
    sigma = 1.0 / math.sqrt(RATE * 2 * 10.0 ** 0.3)  # CSimulate::Configure at Eb/N0 3.0 dB, QPSK
    gen = torch.Generator(device="cuda").manual_seed(7)
    d_rx = torch.randn(n, dtype=torch.float32, device="cuda", generator=gen) * (sigma / math.sqrt(2.0)) - 0.707107
    d_llr4 = torch.empty(n // 2, dtype=torch.uint8, device="cuda")
    d_bits = torch.empty(n // 32, dtype=torch.int32, device="cuda")
    d_st = torch.zeros((groups, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    last = {}

    def decode():
        dec.decode_packed_device(d_llr4.data_ptr(), groups, d_bits.data_ptr(), d_st.data_ptr())
        last["counters"] = dec.count_errors_packed_device(d_bits.data_ptr(), None, groups)

    def chain():
        dec.demap_packed_device(d_rx.data_ptr(), groups, 2, SCALE[2], d_llr4.data_ptr())
        decode()
    chain_ms = _median_ms(chain, reps=10, warm=2)
    chain_counters = last["counters"]
    decode_ms = _median_ms(decode, reps=10, warm=2)
    assert last["counters"] == chain_counters
    dec.close()
    print(json.dumps({"step": "chain", "groups": groups, "codewords": groups * 32, "eb_n0_db": 3.0, "decode_method": 2,
                      "demap_decode_count_ms": round(chain_ms, 3), "decode_count_ms": round(decode_ms, 3),
                      "counters": chain_counters}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--step", choices=["demap", "chain"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return {"demap": step_demap, "chain": step_chain}[a.step](a.groups)
    for step in ("demap", "chain"):
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--groups", str(a.groups)]).returncode
        if rc != 0:
            print("step %s failed with exit status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
