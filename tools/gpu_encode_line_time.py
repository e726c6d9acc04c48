"""Times of the line-format encode (README "Line-format encode").

    python tools/gpu_encode_line_time.py [--codewords 65536] [--out profiles/r15_encode_line/encode_line_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_capture_time.py):
  encode   --codewords codewords (whole groups) of random payload resident in HBM, and the same messages as int8 groups.  Four
           calls alternate in one process, 20 times each after 3 warm-up calls, host clock around the synchronising call:
             groups_int8  lnsfaid_encode_device on the int8 groups (the call the parent commit has: unchanged in this tree)
             line         lnsfaid_encode_line_device without bits
             line_bits    lnsfaid_encode_line_device with bits
             copy         a device-to-device copy of n * L / 8 bytes: the bytes the line call writes, read and written once each (the
                          call itself reads the smaller n * K / 8)
           Then a fixed sample of 256 codewords, spread over the batch and over the places in a workgroup, is compared with
           lnsfaid_encode_line_host, line and bits.
Prints one JSON line (median, minimum and maximum in ms, bytes moved) and appends it to --out.  Exit status 1 when the sample differs
or when the line call without bits is slower than lnsfaid_encode_device, median against median: it does the same GF(2) work on seven
eighths of the parity rows and moves a sixth of the bytes, so a slower call has a broken way in or way out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
SAMPLE = 256


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step_encode(n, out_path, reps=20, warm=3):
    import numpy as np
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    pyabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pyabi)
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    N, K, L = code.N, code.K, code.N - code.code.puncture_tail
    assert n % 32 == 0, "--codewords: whole groups, so that lnsfaid_encode_device encodes the same batch"
    ng = n // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, ng, lib)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(15)
    d_pay = torch.randint(-2 ** 31, 2 ** 31, (n, K // 32), dtype=torch.int32, device="cuda", generator=gen)
    # the same messages one int8 per bit: [32][K] per group is codeword after codeword
    d_msg = torch.empty((n, K), dtype=torch.int8, device="cuda")
    shifts = torch.arange(32, dtype=torch.int32, device="cuda")
    for c0 in range(0, n, 4096):
        d_msg[c0:c0 + 4096] = ((d_pay[c0:c0 + 4096].unsqueeze(-1) >> shifts) & 1).reshape(-1, K).to(torch.int8)
    d_groups = torch.empty(n * N, dtype=torch.int8, device="cuda")
    d_line = torch.empty((n, L // 32), dtype=torch.int32, device="cuda")
    d_bits = torch.empty((n, N // 32), dtype=torch.int32, device="cuda")
    d_copy = torch.empty((n, L // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def copy():
        d_copy.copy_(d_line)
        torch.cuda.synchronize()
    calls = {
        "groups_int8": lambda: dec.encode_device(d_msg.data_ptr(), ng, d_groups.data_ptr()),
        "line": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), None),
        "line_bits": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), d_bits.data_ptr()),
        "copy": copy,
    }
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all four see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    # the sample: codeword i * n / 256 + i % 32, so every place of a workgroup occurs
    idx = np.array([min(i * (n // SAMPLE) + i % 32, n - 1) for i in range(SAMPLE)])
    d_idx = torch.from_numpy(idx).cuda()
    pay = d_pay[d_idx].cpu().numpy().view(np.uint32)
    want_line, want_bits = pyabi.encode_line_host(code.code, pay, SAMPLE, True, lib)
    got_line = d_line[d_idx].cpu().numpy().view(np.uint32)
    got_bits = d_bits[d_idx].cpu().numpy().view(np.uint32)
    # and against the int8 groups of the parent's call: [32][K] then [32][M] per group
    cw, g, m = torch.from_numpy(idx), torch.from_numpy(idx // 32), torch.from_numpy(idx % 32)
    grp = d_groups.reshape(ng, 32 * N)
    par = torch.stack([grp[int(gg), 32 * K + int(mm) * (N - K):32 * K + (int(mm) + 1) * (N - K)] for gg, mm in zip(g, m)]).cpu().numpy()
    par_bits = np.packbits(par.astype(np.uint8), axis=1, bitorder="little").view("<u4")
    row = {"step": "encode", "codewords": n, "reps": reps}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"groups_int8": n * (K + N), "line": n * (K + L) // 8, "line_bits": n * (K + L + N) // 8, "copy": 2 * n * L // 8}
    row["sample_equals_host_form"] = bool(np.array_equal(got_line, want_line) and np.array_equal(got_bits, want_bits))
    row["sample_parity_equals_groups_int8"] = bool(np.array_equal(got_bits[:, K // 32:], par_bits))
    row["line_over_copy"] = round(row["line_ms"]["median"] / row["copy_ms"]["median"], 2)
    row["line_over_groups_int8"] = round(row["line_ms"]["median"] / row["groups_int8_ms"]["median"], 3)
    row["pass"] = row["line_ms"]["median"] <= row["groups_int8_ms"]["median"]
    dec.close()
    text = json.dumps(row)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    return 0 if row["pass"] and row["sample_equals_host_form"] and row["sample_parity_equals_groups_int8"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_encode_line", "encode_line_time.jsonl"))
    ap.add_argument("--step", choices=["encode"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_encode(a.codewords, a.out)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "encode",
                         "--codewords", str(a.codewords), "--out", a.out]).returncode
    if rc != 0:
        print("step encode failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
