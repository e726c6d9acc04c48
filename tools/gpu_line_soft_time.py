"""Times of the line-format soft channel (README "Line-format soft channel").

    python tools/gpu_line_soft_time.py [--codewords 65536] [--out profiles/r17_line_soft/line_soft_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_line_link_time.py) and stops at the first
failure:
  soft     --codewords codewords resident in HBM, DecodeMethod 2, 10 iterations.  The calls of one pass of a soft sweep, and what
           they are compared with, alternate in one process, 20 times each after 3 warm-up passes, host clock around the
           synchronising call:
             payload      lnsfaid_line_payload_random_device
             encode       lnsfaid_encode_line_device on that payload (without bits)
             soft_36      lnsfaid_line_soft_device with the table of Eb/N0 3.6 dB (default scale), with d_flips and total_flips
             soft_42      the same at 4.2 dB
             bsc_010      lnsfaid_line_bsc_device, p = 0.010, out of place, with d_flips and total_flips
             decode_36    lnsfaid_decode_line_device, LNSFAID_LINE_LLR4, with stats, on the output of soft_36
             decode_42    the same on the output of soft_42
             counters     lnsfaid_line_count_errors_device on the payload decode_42 returned, the sent payload and its stats
             copy_soft    two device-to-device copies, one of the bytes the soft call reads and one of the bytes it writes
           Then the counters of the pass are compared with lnsfaid_line_count_errors_host on what the device returned, and a sample
           of 64 codewords of the channel's output and flips with the host form.
Prints one JSON line (median, minimum and maximum in ms, mean I / J of the decodes, the counters) and appends it to --out.  Exit
status 1 when a comparison fails or when payload + encode + soft_42 + counters together take longer than decode_42, median against
median: a sweep must stay bound by the decoder, not by what feeds it.  soft / bsc and soft / copy are reported, not gated."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
SAMPLE = 64
KEY = 0x5EED0F50C0DE2025
SCALE = 13.0 / math.sqrt(2.0)


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step_soft(n, out_path, reps=20, warm=3):
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
    points = {"36": 3.6, "42": 4.2}
    table = {p: pyabi.line_awgn_table(1.0 / math.sqrt(2.0 * (K / L) * 10.0 ** (db / 10.0)), SCALE, lib) for p, db in points.items()}
    d_pay, d_line, d_hard = buf(n, kw), buf(n, lw), buf(n, lw)
    d_rx = {p: buf(n, 4 * lw) for p in points}
    d_back = {p: buf(n, kw) for p in points}
    d_st = {p: buf(n, 4) for p in points}
    d_flips = {p: buf(n) for p in points}
    d_bsc_flips = buf(n)
    d_copy_in, d_copy_out, d_copy_src = buf(n, lw), buf(n, 4 * lw), buf(n, 4 * lw)
    threshold = pyabi.line_bsc_threshold(0.010, lib)
    torch.cuda.synchronize()
    last = {}

    def soft(p):
        def f():
            last["flips_" + p] = dec.line_soft_device(d_line.data_ptr(), n, KEY, 0, table[p], d_rx[p].data_ptr(), d_flips[p].data_ptr())
        return f

    def bsc():
        last["flips_bsc"] = dec.line_bsc_device(d_line.data_ptr(), n, KEY, 0, threshold, d_hard.data_ptr(), d_bsc_flips.data_ptr())

    def decode(p):
        return lambda: dec.decode_line_device(d_rx[p].data_ptr(), pyabi.LINE_LLR4, n, d_back[p].data_ptr(), None, d_st[p].data_ptr())

    def counters():
        last["counters"] = dec.line_count_errors_device(d_back["42"].data_ptr(), d_pay.data_ptr(), d_st["42"].data_ptr(), n, True, True, True)

    def copy_soft():
        d_copy_in.copy_(d_line)
        d_copy_out.copy_(d_copy_src)
        torch.cuda.synchronize()
    calls = {
        "payload": lambda: dec.line_payload_random_device(KEY, 0, n, d_pay.data_ptr()),
        "encode": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), None),
        "soft_36": soft("36"),
        "soft_42": soft("42"),
        "bsc_010": bsc,
        "decode_36": decode("36"),
        "decode_42": decode("42"),
        "counters": counters,
        "copy_soft": copy_soft,
    }
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    row = {"step": "soft", "codewords": n, "reps": reps, "scale": round(SCALE, 8)}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"soft_read": n * L // 8, "soft_written": n * L // 2 + 4 * n, "copy_soft": 2 * (n * L // 8 + n * L // 2),
                    "bsc": 2 * n * L // 8 + 4 * n}
    for p in points:
        st = d_st[p].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
        row["mean_I_J_" + p] = [round(float(st["iterations"].mean()), 3), round(float(st["bf_iterations"].mean()), 3)]
        row["flips_" + p] = last["flips_" + p]
        row["ber_in_" + p] = last["flips_" + p] / (n * L)
        row["table_" + p] = [int(t) for t in table[p]]
    row["counters_42"] = {"errors": last["counters"][0], "fec": last["counters"][1], "vs_sent": last["counters"][2]}
    st = d_st["42"].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
    back, pay = d_back["42"].cpu().numpy().view(np.uint32), d_pay.cpu().numpy().view(np.uint32)
    row["counters_equal_host_form"] = pyabi.line_count_errors_host(code.code, back, pay, st, n, True, True, True, lib) == last["counters"]
    ok = True
    for i in range(SAMPLE):
        c = min(i * (n // SAMPLE) + i % 32, n - 1)
        line = d_line[c].cpu().numpy().view(np.uint32).reshape(1, lw)
        want, want_flips, _ = pyabi.line_soft_host(code.code, line, 1, KEY, c, table["42"], lib=lib)
        ok &= d_rx["42"][c].cpu().numpy().tobytes() == want.tobytes()
        ok &= int(d_flips["42"][c].cpu()) == int(want_flips[0])
    row["sample_equals_host_form"] = bool(ok)
    feed = sum(row[k + "_ms"]["median"] for k in ("payload", "encode", "soft_42", "counters"))
    row["feed_ms"] = round(feed, 3)
    row["feed_over_decode_42"] = round(feed / row["decode_42_ms"]["median"], 3)
    row["soft_over_bsc"] = round(row["soft_42_ms"]["median"] / row["bsc_010_ms"]["median"], 2)
    row["soft_over_copy"] = round(row["soft_42_ms"]["median"] / row["copy_soft_ms"]["median"], 2)
    row["pass"] = feed <= row["decode_42_ms"]["median"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_line_soft", "line_soft_time.jsonl"))
    ap.add_argument("--step", choices=["soft"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_soft(a.codewords, a.out)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "soft",
                         "--codewords", str(a.codewords), "--out", a.out]).returncode
    if rc != 0:
        print("step soft failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
