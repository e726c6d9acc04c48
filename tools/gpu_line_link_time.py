"""Times of the line-format link (README "Line-format link").

    python tools/gpu_line_link_time.py [--codewords 65536] [--out profiles/r16_line_link/line_link_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` (tools/gpu_encode_line_time.py) and stops at the first
failure:
  link     --codewords codewords resident in HBM, DecodeMethod 2, 10 iterations.  The calls of one pass of a sweep, and what they are
           compared with, alternate in one process, 20 times each after 3 warm-up passes, host clock around the synchronising call:
             payload      lnsfaid_line_payload_random_device
             encode       lnsfaid_encode_line_device on that payload (without bits)
             bsc_005      lnsfaid_line_bsc_device, p = 0.005, out of place, with d_flips and total_flips
             bsc_010      the same at p = 0.010
             decode_005   lnsfaid_decode_line_device, LNSFAID_LINE_HARD, magnitude 4, with stats, on the output of bsc_005
             decode_010   the same on the output of bsc_010
             counters     lnsfaid_line_count_errors_device on the payload decode_005 returned, the sent payload and its stats
             copy_payload / copy_line / copy_counters   device-to-device copies of the bytes the payload call writes, the channel
                          reads (and writes as many), and the counter call reads
           Then the counters of the pass are compared with lnsfaid_line_count_errors_host on what the device returned, and a sample
           of 64 codewords of payload and channel output with the host forms.
Prints one JSON line (median, minimum and maximum in ms, mean I / J of the decodes, the counters) and appends it to --out.  Exit
status 1 when a comparison fails or when payload + encode + bsc_005 + counters together take longer than decode_005, the cheapest
decode of a sweep, median against median: the point of the link is that a sweep is bound by the decoder, not by what feeds it."""
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


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step_link(n, out_path, reps=20, warm=3):
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
    kw, lw = K // 32, L // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, (n + 31) // 32, lib)

    def buf(*shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda")
    d_pay, d_line = buf(n, kw), buf(n, lw)
    d_rx = {"005": buf(n, lw), "010": buf(n, lw)}
    d_back = {"005": buf(n, kw), "010": buf(n, kw)}
    d_st = {"005": buf(n, 4), "010": buf(n, 4)}
    d_flips = buf(n)
    d_copy_pay, d_copy_line, d_copy_cnt = buf(n, kw), buf(n, lw), buf(n, 2 * kw + 4)
    d_cnt_src = buf(n, 2 * kw + 4)
    thr = {"005": pyabi.line_bsc_threshold(0.005, lib), "010": pyabi.line_bsc_threshold(0.010, lib)}
    torch.cuda.synchronize()
    last = {}

    def bsc(p):
        def f():
            last["flips_" + p] = dec.line_bsc_device(d_line.data_ptr(), n, KEY, 0, thr[p], d_rx[p].data_ptr(), d_flips.data_ptr())
        return f

    def decode(p):
        return lambda: dec.decode_line_device(d_rx[p].data_ptr(), pyabi.LINE_HARD, n, d_back[p].data_ptr(), None, d_st[p].data_ptr(), 4)

    def counters():
        last["counters"] = dec.line_count_errors_device(d_back["005"].data_ptr(), d_pay.data_ptr(), d_st["005"].data_ptr(), n, True, True, True)

    def copy(dst, src):
        def f():
            dst.copy_(src)
            torch.cuda.synchronize()
        return f
    calls = {
        "payload": lambda: dec.line_payload_random_device(KEY, 0, n, d_pay.data_ptr()),
        "encode": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), None),
        "bsc_005": bsc("005"),
        "bsc_010": bsc("010"),
        "decode_005": decode("005"),
        "decode_010": decode("010"),
        "counters": counters,
        "copy_payload": copy(d_copy_pay, d_pay),
        "copy_line": copy(d_copy_line, d_line),
        "copy_counters": copy(d_copy_cnt, d_cnt_src),
    }
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    row = {"step": "link", "codewords": n, "reps": reps}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"payload": n * K // 8, "bsc": 2 * n * L // 8 + 4 * n, "counters": n * (2 * K // 8 + 16),
                    "copy_payload": 2 * n * K // 8, "copy_line": 2 * n * L // 8, "copy_counters": 2 * n * (2 * K // 8 + 16)}
    for p in ("005", "010"):
        st = d_st[p].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
        row["mean_I_J_" + p] = [round(float(st["iterations"].mean()), 3), round(float(st["bf_iterations"].mean()), 3)]
        row["flips_" + p] = last["flips_" + p]
    row["counters_005"] = {"errors": last["counters"][0], "fec": last["counters"][1], "vs_sent": last["counters"][2]}
    # the counters against the host form on what the device returned; a sample of the generator's output against the host forms
    st = d_st["005"].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
    back, pay = d_back["005"].cpu().numpy().view(np.uint32), d_pay.cpu().numpy().view(np.uint32)
    row["counters_equal_host_form"] = pyabi.line_count_errors_host(code.code, back, pay, st, n, True, True, True, lib) == last["counters"]
    ok = True
    for i in range(SAMPLE):
        c = min(i * (n // SAMPLE) + i % 32, n - 1)
        ok &= np.array_equal(pay[c], pyabi.line_payload_random_host(code.code, KEY, c, 1, lib)[0])
        line = d_line[c].cpu().numpy().view(np.uint32).reshape(1, lw)
        want, _, _ = pyabi.line_bsc_host(code.code, line, 1, KEY, c, thr["005"], lib=lib)
        ok &= np.array_equal(d_rx["005"][c].cpu().numpy().view(np.uint32), want[0])
    row["sample_equals_host_form"] = bool(ok)
    feed = sum(row[k + "_ms"]["median"] for k in ("payload", "encode", "bsc_005", "counters"))
    row["feed_ms"] = round(feed, 3)
    row["feed_over_decode_005"] = round(feed / row["decode_005_ms"]["median"], 3)
    row["bsc_over_copy"] = round(row["bsc_005_ms"]["median"] / row["copy_line_ms"]["median"], 2)
    row["pass"] = feed <= row["decode_005_ms"]["median"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_line_link", "line_link_time.jsonl"))
    ap.add_argument("--step", choices=["link"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_link(a.codewords, a.out)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "link",
                         "--codewords", str(a.codewords), "--out", a.out]).returncode
    if rc != 0:
        print("step link failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
