"""Times of the error-frame capture (README "Error-frame capture").

    python tools/gpu_capture_time.py [--groups 2048]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_prefec_time.py):
  capture   --groups groups (65 536 codewords) of decisions, sent frames and LLRs resident in HBM, a planted share of error frames
            (one wrong information bit each, spread evenly over the batch) of 0, 1e-3, 1e-2 and 1.  Two calls alternate in one
            process: lnsfaid_count_errors_device alone, and lnsfaid_capture_errors_device with capacity 256 and the counters on
            (which replaces it).  Host clock around the synchronising call, median of 20 calls each after 3 warm-up calls.
Prints one JSON line per share."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
SHARES = [0.0, 1e-3, 1e-2, 1.0]
CAPACITY = 256


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


def _median(t):
    t = sorted(t)
    return round(t[len(t) // 2], 3), round(t[0], 3), round(t[-1], 3)


def step_capture(groups, reps=20, warm=3):
    torch, pyabi, lib, code, dec = _setup(groups)
    N, K = code.N, code.K
    n_cw = groups * 32
    d_sent = torch.randint(0, 2, (groups, 32 * N), dtype=torch.int8, device="cuda")
    d_fix = torch.randint(-7, 8, (groups, 32 * N), dtype=torch.int8, device="cuda")
    d_info = d_sent[:, :32 * K].contiguous()  # [32][K] per group: the inputBits of lnsfaid_count_errors_device
    # the sent frames in decodedBits order: frame m of a group = its information part, then its parity part
    d_clean = torch.cat([d_sent[:, :32 * K].reshape(groups, 32, K), d_sent[:, 32 * K:].reshape(groups, 32, N - K)], dim=2).reshape(n_cw, N).contiguous()
    for share in SHARES:
        n_err = int(round(share * n_cw))
        d_dec = d_clean.clone()
        cw = torch.div(torch.arange(n_err, device="cuda") * n_cw, max(n_err, 1), rounding_mode="floor")
        if n_err:
            d_dec[cw, (cw * 977) % K] ^= 1
        first = cw[:CAPACITY].cpu().numpy()  # what the call has to store: the first planted frames, in order
        torch.cuda.synchronize()
        last = {}

        def count():
            last["count"] = dec.count_errors_device(d_dec.data_ptr(), d_info.data_ptr(), groups)

        def capture():
            last["capture"] = dec.capture_errors_device(d_fix.data_ptr(), d_dec.data_ptr(), d_sent.data_ptr(), groups, 0, CAPACITY, True)
        for _ in range(warm):
            count()
            capture()
        t_count, t_capture = [], []
        for _ in range(reps):  # alternated: both see the same state of the machine
            t0 = time.perf_counter()
            count()
            t1 = time.perf_counter()
            capture()
            t2 = time.perf_counter()
            t_count.append((t1 - t0) * 1e3)
            t_capture.append((t2 - t1) * 1e3)
        found, records, payload, counters = last["capture"]
        assert counters == last["count"] and found == n_err == counters[1] and len(records) == min(n_err, CAPACITY), (found, n_err, counters)
        assert records["codeword"].tolist() == first.tolist() and (records["info_errors"] == 1).all() and not records["parity_errors"].any()
        assert (payload[:, 1] != payload[:, 2]).sum() == len(records)  # decisions against sent bits: the one planted flip per frame
        c_ms, c_lo, c_hi = _median(t_count)
        x_ms, x_lo, x_hi = _median(t_capture)
        print(json.dumps({"step": "capture", "groups": groups, "codewords": n_cw, "error_frame_share": share, "found": found,
                          "stored": len(records), "capacity": CAPACITY, "bytes_copied_back": int(records.nbytes + payload.nbytes),
                          "count_errors_ms": c_ms, "count_errors_min_ms": c_lo, "count_errors_max_ms": c_hi,
                          "capture_ms": x_ms, "capture_min_ms": x_lo, "capture_max_ms": x_hi,
                          "capture_minus_count_ms": round(x_ms - c_ms, 3), "counters": counters}), flush=True)
        del d_dec
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--step", choices=["capture"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_capture(a.groups)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "capture",
                         "--groups", str(a.groups)]).returncode
    if rc != 0:
        print("step capture failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
