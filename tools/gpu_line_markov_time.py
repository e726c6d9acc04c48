"""Times of the line-format error-propagation channel (README "Line-format error-propagation channel").

    python tools/gpu_line_markov_time.py [--codewords 65536] [--out profiles/r22_line_markov/line_markov_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_line_link_time.py) and stops at the first
failure:
  markov   --codewords codewords resident in HBM, DecodeMethod 2, 10 iterations, magnitude 4.  The calls of one pass of a hard sweep
           with memory, and what they are compared with, alternate in one process, 20 times each after 3 warm-up passes, host clock
           around the synchronising call:
             payload        lnsfaid_line_payload_random_device
             encode         lnsfaid_encode_line_device on that payload (without bits)
             bsc_010        lnsfaid_line_bsc_device, p = 0.010, out of place, with d_flips and total_flips: the yardstick
             markov_010_05  lnsfaid_line_markov_device with the thresholds of (0.010, 0.5), out of place, with d_flips, d_runs and both
                            totals
             markov_010_09  the same at (0.010, 0.9)
             markov_005_05  the same at (0.005, 0.5): the gate's point
             copy_line      a device-to-device copy of the line
             decode_*       lnsfaid_decode_line_device, LNSFAID_LINE_HARD, with stats, on the output of each of the four
             counters       lnsfaid_line_count_errors_device on the payload decode_markov_005_05 returned, the sent payload and its stats
           Then the counters of the pass are compared with lnsfaid_line_count_errors_host on what the device returned, and a sample
           of 64 codewords of each channel output, its flips and its runs with the host form.
Prints one JSON line (median, minimum and maximum in ms, mean I / J of the decodes, flips, runs, the counters) and appends it to --out.
Exit status 1 when a comparison fails or when payload + encode + markov_005_05 + counters together take longer than
decode_markov_005_05, median against median: a sweep must stay bound by the decoder, not by what feeds it.  markov / bsc and
markov / copy are reported, not gated."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
SAMPLE = 64
KEY = 0x5EED0F50C0DE2025
POINTS = {"010_05": (0.010, 0.5), "010_09": (0.010, 0.9), "005_05": (0.005, 0.5)}


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step_markov(n, out_path, reps=20, warm=3):
    import numpy as np
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    pyabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pyabi)
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    K, L = code.K, code.N - code.code.puncture_tail
    kw, lw = K // 32, L // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, (n + 31) // 32, lib)

    def buf(*shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda")
    t = {p: pyabi.line_markov_thresholds(ber, a, lib) for p, (ber, a) in POINTS.items()}
    outs = ["bsc_010"] + ["markov_" + p for p in POINTS]
    d_pay, d_line, d_copy = buf(n, kw), buf(n, lw), buf(n, lw)
    d_rx = {o: buf(n, lw) for o in outs}
    d_back = {o: buf(n, kw) for o in outs}
    d_st = {o: buf(n, 4) for o in outs}
    d_flips = {o: buf(n) for o in outs}
    d_runs = {o: buf(n) for o in outs}
    threshold = pyabi.line_bsc_threshold(0.010, lib)
    torch.cuda.synchronize()
    last = {}

    def markov(p):
        o = "markov_" + p

        def f():
            last[o] = dec.line_markov_device(d_line.data_ptr(), n, KEY, 0, t[p], d_rx[o].data_ptr(), d_flips[o].data_ptr(), d_runs[o].data_ptr())
        return f

    def bsc():
        last["bsc_010"] = (dec.line_bsc_device(d_line.data_ptr(), n, KEY, 0, threshold, d_rx["bsc_010"].data_ptr(), d_flips["bsc_010"].data_ptr()), 0)

    def decode(o):
        return lambda: dec.decode_line_device(d_rx[o].data_ptr(), pyabi.LINE_HARD, n, d_back[o].data_ptr(), None, d_st[o].data_ptr(), 4)

    gate = "markov_005_05"

    def counters():
        last["counters"] = dec.line_count_errors_device(d_back[gate].data_ptr(), d_pay.data_ptr(), d_st[gate].data_ptr(), n, True, True, True)

    def copy_line():
        d_copy.copy_(d_line)
        torch.cuda.synchronize()
    calls = {
        "payload": lambda: dec.line_payload_random_device(KEY, 0, n, d_pay.data_ptr()),
        "encode": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), None),
        "bsc_010": bsc,
    }
    for p in POINTS:
        calls["markov_" + p] = markov(p)
    calls["copy_line"] = copy_line
    for o in outs:
        calls["decode_" + o] = decode(o)
    calls["counters"] = counters
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(ms)
    row = {"step": "markov", "codewords": n, "reps": reps}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"channel": 2 * n * L // 8 + 8 * n, "bsc": 2 * n * L // 8 + 4 * n, "copy_line": 2 * n * L // 8}
    for o in outs:
        st = d_st[o].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
        row["mean_I_J_" + o] = [round(float(st["iterations"].mean()), 3), round(float(st["bf_iterations"].mean()), 3)]
        row["uncorrectable_" + o] = int((st["unsatisfied"] > 0).sum())
        flips, runs = last[o]
        row["flips_" + o] = flips
        row["ber_in_" + o] = flips / (n * L)
        if runs:
            row["runs_" + o] = runs
            row["mean_run_" + o] = round(flips / runs, 4)
    for p in POINTS:
        row["t_" + p] = [int(x) for x in t[p]]
    row["counters_005_05"] = {"errors": last["counters"][0], "fec": last["counters"][1], "vs_sent": last["counters"][2]}
    st = d_st[gate].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
    back, pay = d_back[gate].cpu().numpy().view(np.uint32), d_pay.cpu().numpy().view(np.uint32)
    row["counters_equal_host_form"] = pyabi.line_count_errors_host(code.code, back, pay, st, n, True, True, True, lib) == last["counters"]
    ok = True
    for i in range(SAMPLE):
        c = min(i * (n // SAMPLE) + i % 32, n - 1)
        line = d_line[c].cpu().numpy().view(np.uint32).reshape(1, lw)
        for p in POINTS:
            o = "markov_" + p
            want, want_flips, want_runs, _, _ = pyabi.line_markov_host(code.code, line, 1, KEY, c, t[p], lib=lib)
            ok &= d_rx[o][c].cpu().numpy().tobytes() == want.tobytes()
            ok &= int(d_flips[o][c].cpu()) == int(want_flips[0]) and int(d_runs[o][c].cpu()) == int(want_runs[0])
    row["sample_equals_host_form"] = bool(ok)
    feed = sum(row[k + "_ms"]["median"] for k in ("payload", "encode", gate, "counters"))
    row["feed_ms"] = round(feed, 3)
    row["feed_over_decode_005_05"] = round(feed / row["decode_" + gate + "_ms"]["median"], 3)
    for p in POINTS:
        row["markov_%s_over_bsc" % p] = round(row["markov_" + p + "_ms"]["median"] / row["bsc_010_ms"]["median"], 3)
    row["bsc_max_over_min"] = round(row["bsc_010_ms"]["max"] / row["bsc_010_ms"]["min"], 3)
    row["markov_over_copy"] = round(row["markov_010_05_ms"]["median"] / row["copy_line_ms"]["median"], 2)
    row["pass"] = feed <= row["decode_" + gate + "_ms"]["median"]
    dec.close()
    text = json.dumps(row)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    return 0 if row["pass"] and row["sample_equals_host_form"] and row["counters_equal_host_form"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_line_markov", "line_markov_time.jsonl"))
    ap.add_argument("--step", choices=["markov"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_markov(a.codewords, a.out)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "markov",
                         "--codewords", str(a.codewords), "--out", a.out]).returncode
    if rc != 0:
        print("step markov failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
