"""Times of the line-format failure capture (README "Line-format failure capture").

    python tools/gpu_line_capture_time.py [--codewords 65536] [--out profiles/r21_line_capture/line_capture_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` and stops at the first failure:
  capture  --codewords codewords resident in HBM, DecodeMethod 2, 10 iterations.  One pass of a soft sweep at Eb/N0 4.2 dB is run
           once to fill the buffers: payload, encode (with bits: the sent words), soft channel, decode (with bits), counters.  Then
           decisions with planted failures are made from the sent words: codeword i differs from its sent word in payload bit 0
           when i is a multiple of 1 / share, for a share of 0 (nothing planted), 0.001, 0.01 and 1.  The calls below alternate in one
           process, 20 times each after 3 warm-up passes, host clock around the synchronising call:
             payload, encode_bits, soft_42, decode_42_bits, counters    the calls of the pass, encode and decode with their bits
             capture_real_llr4    lnsfaid_line_capture_device, select 3, capacity 256, on what the decode returned
             capture_<fmt>_<share>  the same on the planted decisions, LNSFAID_LINE_LLR4 with the soft channel's output as the line and
                                  LNSFAID_LINE_HARD with the encoder's line
             copy_flag            one device-to-device copy of exactly the bytes the flag pass reads: the decisions and the sent words
           A copy writes what it reads, so 0.5 of the copy's time is the time of reading these bytes at the copy's rate.
           Then the records of every planted call are compared with the plan - the first 256 planted indices in ascending order - and
           with lnsfaid_line_capture_host on a prefix of the batch that holds at least four planted failures.
Prints one JSON line (median, minimum and maximum in ms, found and stored per call) and appends it to --out.  Exit status 1 when a
comparison fails or when payload + encode_bits + soft_42 + counters + capture_real_llr4 together take longer than decode_42_bits,
median against median: a sweep that captures must stay bound by the decoder.  capture / copy is reported, not gated."""
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
KEY = 0x5EED0F50C0DE2025
SCALE = 13.0 / math.sqrt(2.0)
CAPACITY = 256
SHARES = {"0": 0, "0001": 1000, "001": 100, "1": 1}  # name -> period of the planted failures (0: none)


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step_capture(n, out_path, reps=20, warm=3):
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
    nw, kw, lw = N // 32, K // 32, L // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, (n + 31) // 32, lib)

    def buf(*shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda")
    table = pyabi.line_awgn_table(1.0 / math.sqrt(2.0 * (K / L) * 10.0 ** (4.2 / 10.0)), SCALE, lib)
    d_pay, d_line, d_sent, d_rx = buf(n, kw), buf(n, lw), buf(n, nw), buf(n, 4 * lw)
    d_back, d_bits, d_st, d_flips = buf(n, kw), buf(n, nw), buf(n, 4), buf(n)
    d_copy_src, d_copy_dst = buf(2, n, nw), buf(2, n, nw)
    last = {}

    def counters():
        last["counters"] = dec.line_count_errors_device(d_back.data_ptr(), d_pay.data_ptr(), d_st.data_ptr(), n, True, True, True)

    def capture(name, line, fmt, bits):
        def f():
            last[name] = dec.line_capture_device(line.data_ptr(), fmt, bits.data_ptr(), d_sent.data_ptr(), n, 0, 3, 0, CAPACITY)
        return f

    def copy_flag():
        d_copy_dst.copy_(d_copy_src)
        torch.cuda.synchronize()
    calls = {
        "payload": lambda: dec.line_payload_random_device(KEY, 0, n, d_pay.data_ptr()),
        "encode_bits": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line.data_ptr(), d_sent.data_ptr()),
        "soft_42": lambda: dec.line_soft_device(d_line.data_ptr(), n, KEY, 0, table, d_rx.data_ptr(), d_flips.data_ptr()),
        "decode_42_bits": lambda: dec.decode_line_device(d_rx.data_ptr(), pyabi.LINE_LLR4, n, d_back.data_ptr(), d_bits.data_ptr(), d_st.data_ptr()),
        "counters": counters,
        "capture_real_llr4": capture("capture_real_llr4", d_rx, pyabi.LINE_LLR4, d_bits),
    }
    for fn in calls.values():  # fill the buffers once: the planted decisions are made from the sent words
        fn()
    planted = {}
    for name, period in SHARES.items():
        b = d_sent.clone()
        if period:
            b[::period, 0] ^= 1
        planted[name] = b
        for fmt_name, fmt, line in (("llr4", pyabi.LINE_LLR4, d_rx), ("hard", pyabi.LINE_HARD, d_line)):
            calls["capture_%s_%s" % (fmt_name, name)] = capture("capture_%s_%s" % (fmt_name, name), line, fmt, b)
    calls["copy_flag"] = copy_flag
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    row = {"step": "capture", "codewords": n, "reps": reps, "capacity": CAPACITY}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"flag_read": 2 * n * N // 8, "copy_flag": 2 * 2 * n * N // 8, "record_hard": 32 + 4 * pyabi.line_capture_words(code.code, 0, lib),
                    "record_llr4": 32 + 4 * pyabi.line_capture_words(code.code, 1, lib)}
    row["counters_42"] = {"errors": last["counters"][0], "fec": last["counters"][1], "vs_sent": last["counters"][2]}
    row["found_stored"] = {k: [v[0], len(v[1])] for k, v in last.items() if k.startswith("capture")}
    vs = last["counters"][2]
    ok = last["capture_real_llr4"][0] == vs[1] + vs[3]  # ErrorFrame + FalseAlarmFrame of the same pass
    sent, rx, line = d_sent.cpu().numpy().view(np.uint32), d_rx.cpu().numpy().view(np.uint8).reshape(n, L // 2), d_line.cpu().numpy().view(np.uint32)
    for name, period in SHARES.items():
        plan = list(range(0, n, period)) if period else []
        bits = planted[name].cpu().numpy().view(np.uint32)
        m = min(n, 4 * period + 1) if period else 64
        for fmt_name, fmt, img in (("llr4", pyabi.LINE_LLR4, rx), ("hard", pyabi.LINE_HARD, line)):
            found, rec, sec = last["capture_%s_%s" % (fmt_name, name)]
            ok &= found == len(plan) and rec["index"].tolist() == plan[:CAPACITY]
            h_found, h_rec, h_sec = pyabi.line_capture_host(code.code, img[:m], fmt, bits[:m], sent[:m], m, 0, 3, 0, CAPACITY, lib)
            k = min(len(h_rec), len(rec))
            ok &= h_found == len([i for i in plan if i < m]) and k == min(h_found, CAPACITY)
            ok &= h_rec[:k].tobytes() == rec[:k].tobytes() and all(np.array_equal(h_sec[s][:k], sec[s][:k]) for s in h_sec)
    row["records_equal_plan_and_host_form"] = bool(ok)
    feed = sum(row[k + "_ms"]["median"] for k in ("payload", "encode_bits", "soft_42", "counters", "capture_real_llr4"))
    row["feed_ms"] = round(feed, 3)
    row["feed_over_decode_42"] = round(feed / row["decode_42_bits_ms"]["median"], 3)
    half_copy = 0.5 * row["copy_flag_ms"]["median"]
    row["capture_over_half_copy"] = {k[:-3]: round(row[k]["median"] / half_copy, 2) for k in row if k.startswith("capture_") and k.endswith("_ms")}
    row["capture_over_counters"] = round(row["capture_llr4_0_ms"]["median"] / row["counters_ms"]["median"], 2)
    row["pass"] = feed <= row["decode_42_bits_ms"]["median"]
    dec.close()
    text = json.dumps(row)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    return 0 if row["pass"] and row["records_equal_plan_and_host_form"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_line_capture", "line_capture_time.jsonl"))
    ap.add_argument("--step", choices=["capture"])
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    a = ap.parse_args()
    if a.step:
        return step_capture(a.codewords, a.out)
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", "capture",
                         "--codewords", str(a.codewords), "--out", a.out]).returncode
    if rc != 0:
        print("step capture failed with exit status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
