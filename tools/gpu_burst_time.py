"""Times of the burst-format line calls against the line calls they extend (README "Burst-format line calls").

    python tools/gpu_burst_time.py [--codewords 65536] [--eb-n0 3.6] [--reps 10] [--out profiles/r20_burst/burst_time.jsonl]

The parent process starts each GPU step as a child under its own `timeout` (tools/gpu_capture_time.py).  Both steps: one process,
the batch resident in HBM, calls alternated, `--reps` timed calls each after two warm-up calls, the host clock around the
synchronising call - so the upload of the per-codeword descriptors, which lnsfaid_decode_burst_device / lnsfaid_encode_burst_device
do themselves, is inside the timed call.
  decode   DecodeMethod 2, 10 iterations, bench.py's synthetic LLRs re-laid with lnsfaid_line_from_fixinput (tools/gpu_line_time.py)
           into both line formats (HARD decoded at magnitude 4).  Per format:
             line      lnsfaid_decode_line_device (the parent commit's call; its kernel file is unchanged)
             burst0    lnsfaid_decode_burst_device on the same line with an explicit all-zero `shortened`: the same iterations,
                       and it must return equal bytes (payload and records are compared)
             burstS    a burst-shaped input: bursts of 8 codewords, the last of each shortened (LNSFAID_SHORTEN_TAIL) by a value
                       drawn from 0, 32, 224, 256, 288, 5760, 8288, 14560 bits; the line is the same LLRs with the known words
                       dropped (the synthetic frames are the all-zero codeword, so the dropped bits are zeros).  Reported only.
           gate: median(burst0) <= median(line) + 0.33 ms, the fixed share of a launch, in both formats.
  encode   random payloads.  groups_int8: lnsfaid_encode_device on the same messages as int8 groups (the gate of
           tools/gpu_encode_line_time.py carried over); line: lnsfaid_encode_line_device; burst0 / burstS as above, without bits.
           gate: median(burst0) <= median(groups_int8).  burst0 must equal line byte for byte; a sample of burstS is compared with
           lnsfaid_encode_burst_host.
Prints one JSON line per step and appends it to --out.  Exit status 1 when a gate or a comparison fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
FIXED_SHARE_MS = 0.33
SHORT = (0, 32, 224, 256, 288, 5760, 8288, 14560)
BURST = 8


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def _alternate(calls, reps, warm=2):
    times = {k: [] for k in calls}
    for rep in range(warm + reps):  # alternated: every call sees the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                times[k].append(t)
    return times


def _burst_shaped(np, n):
    """S = 0 except at the last codeword of every burst of 8"""
    s = np.zeros(n, dtype=np.uint32)
    last = np.arange(BURST - 1, n, BURST)
    s[last] = np.random.default_rng(20).choice(np.array(SHORT, dtype=np.uint32), size=last.size)
    return s


def _keep_words(np, s, X, K):
    """[n, X / 32] mask of the words of positions 0 .. X - 1 that stay when codeword c loses its last S_c information bits"""
    w = np.arange(X // 32)[None, :]
    k1 = K // 32
    return ~((w >= k1 - (s // 32)[:, None]) & (w < k1))


def _append(out_path, row):
    text = json.dumps(row)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")


def step_decode(n, eb, reps, out_path):
    import numpy as np
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    pyabi = _load("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    bench = _load("lnsfaid_bench", os.path.join(ROOT, "bench.py"))
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    N, K, L = code.N, code.K, code.N - code.code.puncture_tail
    assert n % 32 == 0 and n % BURST == 0
    ng = n // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, ng, lib)
    fix = bench.synth_llr(torch, "cuda", ng, eb, seed=3).reshape(-1).cpu().numpy()
    zero = np.zeros(n, dtype=np.uint32)
    shaped = _burst_shaped(np, n)
    line_bits, payload_bits = pyabi.burst_words(code.code, shaped, n, lib)
    keep = _keep_words(np, shaped, L, K)
    d_pay = [torch.empty(n * K // 32, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_st = [torch.empty((n, 4), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_ones = torch.empty(n, dtype=torch.int32, device="cuda")
    row = {"step": "decode", "eb_n0": eb, "codewords": n, "method": 2, "reps": reps, "bursts": n // BURST,
           "descriptor_upload_in_timed_call": True}
    ok = True
    for fmt, name, mag in ((pyabi.LINE_LLR4, "llr4", 0), (pyabi.LINE_HARD, "hard", 4)):
        line = pyabi.line_from_fixinput(code.code, fix, n, fmt, lib)
        unit = 16 if fmt == pyabi.LINE_LLR4 else 4  # bytes per 32 positions
        short_line = np.ascontiguousarray(line.view(np.uint8).reshape(n, L // 32, unit)[keep])
        assert short_line.size == line_bits // 32 * unit
        d_line = torch.from_numpy(line.view(np.uint8)).cuda()
        d_short = torch.from_numpy(short_line.reshape(-1)).cuda()
        torch.cuda.synchronize()
        calls = {
            "line": lambda: dec.decode_line_device(d_line.data_ptr(), fmt, n, d_pay[0].data_ptr(), None, d_st[0].data_ptr(), mag),
            "burst0": lambda: dec.decode_burst_device(d_line.data_ptr(), fmt, zero, pyabi.SHORTEN_TAIL, n, d_pay[1].data_ptr(), None,
                                                      d_st[1].data_ptr(), d_ones.data_ptr(), mag),
        }
        times = _alternate(calls, reps)
        equal = bool(torch.equal(d_pay[0], d_pay[1]) and torch.equal(d_st[0], d_st[1]) and not bool(d_ones.any()))
        st = d_st[0].cpu().numpy()
        r = {"line_ms": _summary(times["line"]), "burst0_ms": _summary(times["burst0"]),
             "mean_I_J": [round(float(st[:, 0].mean()), 3), round(float(st[:, 1].mean()), 3)],
             "bytes_read": n * L // 32 * unit, "burst0_equals_line": equal}
        r["burst0_minus_line_ms"] = round(r["burst0_ms"]["median"] - r["line_ms"]["median"], 3)
        r["pass"] = r["burst0_minus_line_ms"] <= FIXED_SHARE_MS and equal
        # the burst-shaped input, on its own (another input: reported, not gated)
        shaped_call = {"burstS": lambda: dec.decode_burst_device(d_short.data_ptr(), fmt, shaped, pyabi.SHORTEN_TAIL, n, d_pay[1].data_ptr(),
                                                                 None, d_st[1].data_ptr(), d_ones.data_ptr(), mag)}
        ts = _alternate(shaped_call, reps)
        st = d_st[1].cpu().numpy()
        r["burstS_ms"] = _summary(ts["burstS"])
        r["burstS_mean_I_J"] = [round(float(st[:, 0].mean()), 3), round(float(st[:, 1].mean()), 3)]
        r["burstS_bytes_read"] = line_bits // 32 * unit
        r["burstS_unsatisfied_codewords"] = int((st[:, 2] > 0).sum())
        r["burstS_short_ones_codewords"] = int((d_ones > 0).sum())
        row[name] = r
        ok &= r["pass"]
        del d_line, d_short
    dec.close()
    row["pass"] = bool(ok)
    _append(out_path, row)
    return 0 if ok else 1


def step_encode(n, reps, out_path):
    import numpy as np
    import torch
    torch.cuda.init()
    pyabi = _load("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    N, K, L = code.N, code.K, code.N - code.code.puncture_tail
    assert n % 32 == 0 and n % BURST == 0
    ng = n // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, ng, lib)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    d_pay = torch.randint(-2 ** 31, 2 ** 31, (n, K // 32), dtype=torch.int32, device="cuda", generator=gen)
    d_msg = torch.empty((n, K), dtype=torch.int8, device="cuda")  # the same messages one int8 per bit
    shifts = torch.arange(32, dtype=torch.int32, device="cuda")
    for c0 in range(0, n, 4096):
        d_msg[c0:c0 + 4096] = ((d_pay[c0:c0 + 4096].unsqueeze(-1) >> shifts) & 1).reshape(-1, K).to(torch.int8)
    zero = np.zeros(n, dtype=np.uint32)
    shaped = _burst_shaped(np, n)
    line_bits, payload_bits = pyabi.burst_words(code.code, shaped, n, lib)
    d_pay_s = torch.from_numpy(np.ascontiguousarray(d_pay.cpu().numpy()[_keep_words(np, shaped, K, K)])).cuda()
    assert d_pay_s.numel() == payload_bits // 32
    d_groups = torch.empty(n * N, dtype=torch.int8, device="cuda")
    d_line = [torch.empty(n * L // 32, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_line_s = torch.empty(line_bits // 32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = {
        "groups_int8": lambda: dec.encode_device(d_msg.data_ptr(), ng, d_groups.data_ptr()),
        "line": lambda: dec.encode_line_device(d_pay.data_ptr(), n, d_line[0].data_ptr(), None),
        "burst0": lambda: dec.encode_burst_device(d_pay.data_ptr(), zero, pyabi.SHORTEN_TAIL, n, d_line[1].data_ptr(), None),
        "burstS": lambda: dec.encode_burst_device(d_pay_s.data_ptr(), shaped, pyabi.SHORTEN_TAIL, n, d_line_s.data_ptr(), None),
    }
    times = _alternate(calls, reps)
    row = {"step": "encode", "codewords": n, "reps": reps, "bursts": n // BURST, "descriptor_upload_in_timed_call": True}
    for k in calls:
        row[k + "_ms"] = _summary(times[k])
    row["bytes"] = {"groups_int8": n * (K + N), "line": n * (K + L) // 8, "burst0": n * (K + L) // 8 + 16 * n,
                    "burstS": (payload_bits + line_bits) // 8 + 16 * n}
    row["burst0_equals_line"] = bool(torch.equal(d_line[0], d_line[1]))
    # the first 64 bursts of the shaped input against the host form
    m = 64 * BURST
    pw, lw = (int(x) // 32 for x in pyabi.burst_words(code.code, shaped[:m], m, lib)[::-1])
    want, _ = pyabi.encode_burst_host(code.code, d_pay_s[:pw].cpu().numpy().view(np.uint32), shaped[:m], pyabi.SHORTEN_TAIL, m, False, lib)
    row["burstS_sample_equals_host_form"] = bool(np.array_equal(d_line_s[:lw].cpu().numpy().view(np.uint32), want))
    row["burst0_over_line"] = round(row["burst0_ms"]["median"] / row["line_ms"]["median"], 3)
    row["burst0_over_groups_int8"] = round(row["burst0_ms"]["median"] / row["groups_int8_ms"]["median"], 3)
    row["pass"] = bool(row["burst0_ms"]["median"] <= row["groups_int8_ms"]["median"] and row["burst0_equals_line"]
                       and row["burstS_sample_equals_host_form"])
    dec.close()
    _append(out_path, row)
    return 0 if row["pass"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--eb-n0", type=float, default=3.6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_burst", "burst_time.jsonl"))
    ap.add_argument("--step", choices=["decode", "encode"])
    ap.add_argument("--timeout", type=int, default=420, help="seconds per step")
    a = ap.parse_args()
    if a.step == "decode":
        return step_decode(a.codewords, a.eb_n0, a.reps, a.out)
    if a.step == "encode":
        return step_encode(a.codewords, a.reps, a.out)
    worst = 0
    for step in ("decode", "encode"):
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--codewords", str(a.codewords), "--eb-n0", str(a.eb_n0), "--reps", str(a.reps), "--out", a.out]).returncode
        if rc != 0:
            print("step %s failed with exit status %d" % (step, rc), file=sys.stderr)
            worst = rc
        if rc not in (0, 1):  # 1 is a missed gate or comparison; anything else ends the run: nothing more is started on the GPU
            break
    return worst


if __name__ == "__main__":
    sys.exit(main() or 0)
