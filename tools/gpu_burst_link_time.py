"""Times of the burst-format link (README "Burst-format link").

    python tools/gpu_burst_link_time.py [--codewords 65536] [--out profiles/r24_burst_link/burst_link_time.jsonl]

The parent process starts the GPU step as a child under its own `timeout` (as tools/gpu_line_link_time.py) and stops at the first
failure:
  link     --codewords codewords resident in HBM as bursts of 8, the last codeword of burst j shortened by SHORT[j % 8] bits at the
           tail, DecodeMethod 2, 10 iterations.  The calls alternate in one process, 20 times each after 3 warm-up passes, host
           clock around the synchronising call:
             payload / encode / bsc_005 / soft_42 / counters    the burst calls of one pass of a sweep: lnsfaid_burst_payload_random_device,
                          lnsfaid_encode_burst_device (without bits), lnsfaid_burst_bsc_device at p = 0.005 and
                          lnsfaid_burst_soft_device at Eb/N0 4.2 dB (scale 13 / sqrt 2), both out of place with d_flips and
                          total_flips, lnsfaid_burst_count_errors_device on what decode_bsc returned (sent, stats, short_ones)
             decode_bsc / decode_soft   lnsfaid_decode_burst_device on the two channels' outputs (HARD at magnitude 4, LLR4)
             copy_line / copy_soft      device-to-device copies of the bytes the BSC and the soft channel read and write
             *_line / *_zero            each burst call beside its unchanged line twin: the same codewords unshortened, through
                          lnsfaid_line_* and through lnsfaid_burst_* with an explicit all-zero `shortened`; the bytes, flips and
                          counters of the two are compared
Prints one JSON line (median, minimum and maximum in ms, mean I / J of the decodes, the counters) and appends it to --out.  Exit
status 1 when a comparison fails or when payload + encode + channel + counters together take longer than the decode they feed,
median against median, for the BSC at p = 0.005 or for the soft channel at 4.2 dB: a burst sweep stays bound by the decoder.  The
difference to the line twins is reported, not gated."""
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
KEY = 0xB0257F0E5EED2026
SHORT = (0, 32, 224, 256, 288, 5760, 8288, 14560)
BURST = 8


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
    s = np.zeros(n, dtype=np.uint32)
    last_of_burst = np.arange(BURST - 1, n, BURST)
    s[last_of_burst] = [SHORT[(c // BURST) % len(SHORT)] for c in last_of_burst]
    zero = np.zeros(n, dtype=np.uint32)
    line_bits, payload_bits = pyabi.burst_words(code.code, s, n, lib)
    lwords, pwords = line_bits // 32, payload_bits // 32
    T, H = pyabi.SHORTEN_TAIL, pyabi.LINE_HARD
    thr = pyabi.line_bsc_threshold(0.005, lib)
    sigma = 1.0 / math.sqrt(2.0 * (K / L) * 10.0 ** 0.42)
    table = pyabi.line_awgn_table(sigma, 13.0 / math.sqrt(2.0), lib)

    def buf(words):
        return torch.zeros(words, dtype=torch.int32, device="cuda")
    # the burst workload
    d_pay, d_line, d_rx, d_soft = buf(pwords), buf(lwords), buf(lwords), buf(4 * lwords)
    d_back = {"bsc": buf(pwords), "soft": buf(pwords)}
    d_st = {"bsc": buf(4 * n), "soft": buf(4 * n)}
    d_ones = {"bsc": buf(n), "soft": buf(n)}
    d_flips = buf(n)
    d_copy_line, d_copy_soft = buf(lwords), buf(4 * lwords)
    # the line twins: the same codewords unshortened, a pair of outputs for each call
    d_lpay = [buf(n * kw), buf(n * kw)]
    d_lline = buf(n * lw)
    d_lrx = [buf(n * lw), buf(n * lw)]
    d_lsoft = [buf(4 * n * lw), buf(4 * n * lw)]
    d_lflips = [buf(n), buf(n), buf(n), buf(n)]
    d_lst = buf(4 * n)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    last = {}

    def keep(name, fn):
        def f():
            last[name] = fn()
        return f

    def copy(dst, src):
        def f():
            dst.copy_(src)
            torch.cuda.synchronize()
        return f
    calls = {
        "payload": lambda: dec.burst_payload_random_device(KEY, 0, s, T, n, p(d_pay)),
        "encode": lambda: dec.encode_burst_device(p(d_pay), s, T, n, p(d_line), None),
        "bsc_005": keep("flips_bsc", lambda: dec.burst_bsc_device(p(d_line), s, T, n, KEY, 0, thr, p(d_rx), p(d_flips))),
        "soft_42": keep("flips_soft", lambda: dec.burst_soft_device(p(d_line), s, T, n, KEY, 0, table, p(d_soft), p(d_flips))),
        "decode_bsc": lambda: dec.decode_burst_device(p(d_rx), H, s, T, n, p(d_back["bsc"]), None, p(d_st["bsc"]), p(d_ones["bsc"]), 4),
        "decode_soft": lambda: dec.decode_burst_device(p(d_soft), pyabi.LINE_LLR4, s, T, n, p(d_back["soft"]), None, p(d_st["soft"]),
                                                       p(d_ones["soft"])),
        "counters": keep("counters", lambda: dec.burst_count_errors_device(p(d_back["bsc"]), p(d_pay), p(d_st["bsc"]), p(d_ones["bsc"]), s, n,
                                                                           True, True, True)),
        "copy_line": copy(d_copy_line, d_line),
        "copy_soft": copy(d_copy_soft, d_soft),
        "payload_line": lambda: dec.line_payload_random_device(KEY, 0, n, p(d_lpay[0])),
        "payload_zero": lambda: dec.burst_payload_random_device(KEY, 0, zero, T, n, p(d_lpay[1])),
        "encode_line": lambda: dec.encode_line_device(p(d_lpay[0]), n, p(d_lline), None),
        "bsc_line": keep("t_bsc_line", lambda: dec.line_bsc_device(p(d_lline), n, KEY, 0, thr, p(d_lrx[0]), p(d_lflips[0]))),
        "bsc_zero": keep("t_bsc_zero", lambda: dec.burst_bsc_device(p(d_lline), zero, T, n, KEY, 0, thr, p(d_lrx[1]), p(d_lflips[1]))),
        "soft_line": keep("t_soft_line", lambda: dec.line_soft_device(p(d_lline), n, KEY, 0, table, p(d_lsoft[0]), p(d_lflips[2]))),
        "soft_zero": keep("t_soft_zero", lambda: dec.burst_soft_device(p(d_lline), zero, T, n, KEY, 0, table, p(d_lsoft[1]), p(d_lflips[3]))),
        "counters_line": keep("c_line", lambda: dec.line_count_errors_device(p(d_lrx[0]), p(d_lline), p(d_lst), n, True, True, True)),
        "counters_zero": keep("c_zero", lambda: dec.burst_count_errors_device(p(d_lrx[0]), p(d_lline), p(d_lst), None, zero, n, True, True, True)),
    }
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: all see the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    row = {"step": "link", "codewords": n, "bursts_of": BURST, "short": list(SHORT), "reps": reps, "line_bits": line_bits,
           "payload_bits": payload_bits}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"payload": payload_bits // 8, "bsc": 2 * line_bits // 8 + 4 * n, "soft": line_bits // 8 + line_bits // 2 + 4 * n,
                    "counters": 2 * payload_bits // 8 + 20 * n, "copy_line": 2 * line_bits // 8, "copy_soft": 2 * line_bits // 2,
                    "descriptors": 16 * n}
    for c in ("bsc", "soft"):
        st = d_st[c].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
        row["mean_I_J_" + c] = [round(float(st["iterations"].mean()), 3), round(float(st["bf_iterations"].mean()), 3)]
        row["flips_" + c] = last["flips_" + c]
        row["short_ones_codewords_" + c] = int((d_ones[c].cpu().numpy() > 0).sum())
    row["counters_bsc"] = {"errors": last["counters"][0], "fec": last["counters"][1], "vs_sent": last["counters"][2]}
    # the counters against the host form on what the device returned; a sample of bursts against the host forms
    st = d_st["bsc"].cpu().numpy().view(pyabi.line_stats_dtype()).reshape(-1)
    back, pay = d_back["bsc"].cpu().numpy().view(np.uint32), d_pay.cpu().numpy().view(np.uint32)
    ones = d_ones["bsc"].cpu().numpy().view(np.uint32)
    row["counters_equal_host_form"] = pyabi.burst_count_errors_host(code.code, back, pay, st, ones, s, n, True, True, True, lib) == last["counters"]
    loff = np.concatenate([[0], np.cumsum((L - s.astype(np.int64)) // 32)])
    poff = np.concatenate([[0], np.cumsum((K - s.astype(np.int64)) // 32)])
    line, rx, soft = (t.cpu().numpy().view(np.uint32) for t in (d_line, d_rx, d_soft))
    ok = True
    for i in range(SAMPLE // BURST):  # whole bursts, spread over the run, each through the host forms with its own first_codeword
        c0 = min((i * (n // (SAMPLE // BURST)) // BURST + i) * BURST, n // BURST * BURST - BURST)  # + i: every value of SHORT once
        sl, m = slice(c0, c0 + BURST), BURST
        ok &= np.array_equal(pay[poff[c0]:poff[c0 + m]], pyabi.burst_payload_random_host(code.code, KEY, c0, s[sl], T, m, lib))
        part = line[loff[c0]:loff[c0 + m]]
        ok &= np.array_equal(rx[loff[c0]:loff[c0 + m]], pyabi.burst_bsc_host(code.code, part, s[sl], T, m, KEY, c0, thr, lib=lib)[0])
        want = pyabi.burst_soft_host(code.code, part, s[sl], T, m, KEY, c0, table, lib=lib)[0]
        ok &= soft[4 * loff[c0]:4 * loff[c0 + m]].tobytes() == want.tobytes()
    row["sample_equals_host_form"] = bool(ok)
    # the line twins: equal bytes, flips, totals and counters
    same = all(torch.equal(a, b) for a, b in ((d_lpay[0], d_lpay[1]), (d_lrx[0], d_lrx[1]), (d_lsoft[0], d_lsoft[1]),
                                              (d_lflips[0], d_lflips[1]), (d_lflips[2], d_lflips[3])))
    same &= last["t_bsc_line"] == last["t_bsc_zero"] and last["t_soft_line"] == last["t_soft_zero"] and last["c_line"] == last["c_zero"]
    row["zero_equals_line_twins"] = bool(same)
    med = lambda k: row[k + "_ms"]["median"]
    row["over_line_twin_ms"] = {k: round(med(k + "_zero") - med(k + "_line"), 3) for k in ("payload", "bsc", "soft", "counters")}
    row["bsc_over_copy"] = round(med("bsc_005") / med("copy_line"), 2)
    row["soft_over_copy"] = round(med("soft_42") / med("copy_soft"), 2)
    for c, ch in (("bsc", "bsc_005"), ("soft", "soft_42")):
        feed = med("payload") + med("encode") + med(ch) + med("counters")
        row["feed_%s_ms" % c] = round(feed, 3)
        row["feed_over_decode_" + c] = round(feed / med("decode_" + c), 3)
    row["pass"] = row["feed_bsc_ms"] <= med("decode_bsc") and row["feed_soft_ms"] <= med("decode_soft")
    dec.close()
    text = json.dumps(row)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")
    return 0 if row["pass"] and row["sample_equals_host_form"] and row["counters_equal_host_form"] and row["zero_equals_line_twins"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_burst_link", "burst_link_time.jsonl"))
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
