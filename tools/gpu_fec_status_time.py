"""Times of the FEC status calls (README "FEC status without the sent bits").

    python tools/gpu_fec_status_time.py [--groups 2048]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_prefec_time.py):
  status   --groups groups (65 536 codewords) of decisions, LLRs and sent frames resident in HBM; one frame in a hundred carries a wrong
           information bit, the others are their sent frame (the all-zero codeword), so the syndrome pass sees real work and the
           counters are known.  Alternated in one process: lnsfaid_fec_status_device and lnsfaid_fec_status_packed_device, each
           without and with the sent frames, lnsfaid_count_errors_device, and for every status call a device-to-device copy of
           the bytes that call reads (the yardstick: a kernel of this shape should run at about the copy's rate).  Host clock
           around the synchronising call, median of 20 calls each after 3 warm-up calls, with minimum and maximum.
Prints one JSON line per call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")


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


def step_status(groups, reps=20, warm=3):
    torch, pyabi, lib, code, dec = _setup(groups)
    N, K = code.N, code.K
    n_cw = groups * 32
    d_sent = torch.zeros(groups * 32 * N, dtype=torch.int8, device="cuda")
    d_dec = torch.zeros((n_cw, N), dtype=torch.int8, device="cuda")
    wrong = torch.arange(0, n_cw, 100, device="cuda")
    d_dec[wrong, (wrong * 977) % K] = 1
    d_fix = torch.randint(-7, 8, (groups * 32 * N,), dtype=torch.int8, device="cuda")
    # the packed forms of the same data: two nibbles per byte, 32 decisions per word
    nib = (d_fix.view(torch.uint8) & 15).reshape(-1, 2)
    d_llr4 = (nib[:, 0] | (nib[:, 1] << 4)).contiguous()
    del nib
    d_bits = torch.zeros((n_cw, N // 8), dtype=torch.uint8, device="cuda")
    d_bits[wrong, ((wrong * 977) % K) // 8] = (2 ** (((wrong * 977) % K) % 8)).to(torch.uint8)
    d_src = torch.empty(groups * 32 * (2 * N + K), dtype=torch.uint8, device="cuda").random_(0, 256)
    d_dst = torch.empty_like(d_src)
    torch.cuda.synchronize()
    reads = {"int8": 2 * N, "int8_sent": 2 * N + K, "packed": N // 2 + N // 8, "packed_sent": N // 2 + N // 8 + K}  # bytes per codeword
    last = {}

    def status(name):
        fn = dec.fec_status_packed_device if name.startswith("packed") else dec.fec_status_device
        a = (d_llr4.data_ptr(), d_bits.data_ptr()) if name.startswith("packed") else (d_fix.data_ptr(), d_dec.data_ptr())
        sent = name.endswith("_sent")
        last[name] = fn(a[0], a[1], d_sent.data_ptr() if sent else None, groups, records=False, vs_sent=True if sent else None)

    def copy(name):
        n = reads[name] * n_cw
        d_dst[:n].copy_(d_src[:n])
        torch.cuda.synchronize()

    def count(_):
        last["count"] = dec.count_errors_device(d_dec.data_ptr(), None, groups)
    calls = [(("status", k), status, k) for k in reads] + [(("copy", k), copy, k) for k in reads] + [(("count_errors", ""), count, "")]
    times = {c[0]: [] for c in calls}
    for rep in range(warm + reps):
        for key, fn, arg in calls:  # alternated: all see the same state of the machine
            t0 = time.perf_counter()
            fn(arg)
            t1 = time.perf_counter()
            if rep >= warm:
                times[key].append((t1 - t0) * 1e3)
    n_wrong = int(wrong.numel())
    for k in reads:
        _, out, vs = last[k]
        assert out[:2] == [n_cw, n_wrong] and out[2] == n_cw - n_wrong, (k, out)
        assert vs is None or vs == [n_cw, n_wrong, 0, 0], (k, vs)
    assert last["count"][:2] == [n_cw, n_wrong]
    for k in reads:
        s_ms, s_lo, s_hi = _median(times[("status", k)])
        c_ms, c_lo, c_hi = _median(times[("copy", k)])
        gb = reads[k] * n_cw / 1e9
        print(json.dumps({"step": "fec_status", "call": k, "groups": groups, "codewords": n_cw, "bytes_read_GB": round(gb, 3),
                          "status_ms": s_ms, "status_min_ms": s_lo, "status_max_ms": s_hi, "status_GBps": round(gb / s_ms * 1e3, 1),
                          "copy_ms": c_ms, "copy_min_ms": c_lo, "copy_max_ms": c_hi, "copy_read_GBps": round(gb / c_ms * 1e3, 1),
                          "status_over_copy": round(s_ms / c_ms, 3), "out": last[k][1], "vs_sent": last[k][2]}), flush=True)
    x_ms, x_lo, x_hi = _median(times[("count_errors", "")])
    print(json.dumps({"step": "fec_status", "call": "count_errors_device", "groups": groups, "codewords": n_cw,
                      "bytes_read_GB": round(K * n_cw / 1e9, 3), "ms": x_ms, "min_ms": x_lo, "max_ms": x_hi, "counters": last["count"]}), flush=True)
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--step", choices=["status"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_status(a.groups)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "status",
                         "--groups", str(a.groups)]).returncode
    if rc != 0:
        print("step status failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
