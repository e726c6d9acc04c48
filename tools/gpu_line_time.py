"""Line-format decode against the packed per-codeword decode it is defined by (README "Line-format decode").

    python tools/gpu_line_time.py [--codewords 65536] [--reps 10] [--out FILE]

One process, DecodeMethod 2, the batch resident in HBM.  Per Eb/N0 (3.0, 3.6, 4.2 dB): bench.py's synthetic LLRs, re-laid on the
host with lnsfaid_line_from_fixinput into both line formats (LNSFAID_LINE_HARD: their signs, decoded at magnitude 4) and, from
the LLR4 line, with lnsfaid_line_to_llr4 into the equivalent llr4.  Then, alternating, `--reps` times each after two warm-up
calls, with the host clock around the synchronising call:
  packed     lnsfaid_decode_codewords_packed_device on that llr4 (the call the parent commit has: it is unchanged in this tree)
  line_llr4  lnsfaid_decode_line_device, the same iterations on the same LLRs: expected level with `packed`
  line_hard  lnsfaid_decode_line_device on one bit per code bit: another input, reported with its mean I / J only
All three write per-codeword records.  Prints one JSON line per Eb/N0 with median, minimum and maximum in ms, the mean
iterations, and two checks: the LLR4 payloads equal the first K / 32 words of the packed decisions, and
  pass: median(line_llr4) <= median(packed) + 0.33 ms
(0.33 ms is the fixed share of a launch - staging, first syndrome, output, launch: DESIGN.md 7.1 - so a line call that is later
than that has broken staging or output, serialised loads for instance).  Exit status 1 when a check fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
FIXED_SHARE_MS = 0.33


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    pyabi = _load("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    bench = _load("lnsfaid_bench", os.path.join(ROOT, "bench.py"))
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    n, N, K = a.codewords, code.N, code.K
    assert n % 32 == 0, "--codewords: whole groups, so that the packed call decodes the same batch"
    ng = n // 32
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, ng, lib)
    d_pay = torch.empty(n * K // 32, dtype=torch.int32, device="cuda")
    d_bits = torch.empty(n * N // 32, dtype=torch.int32, device="cuda")
    d_cw = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    d_st = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    ok = True
    for eb in (3.0, 3.6, 4.2):
        fix = bench.synth_llr(torch, "cuda", ng, eb, seed=3).reshape(-1).cpu().numpy()
        soft = pyabi.line_from_fixinput(code.code, fix, n, pyabi.LINE_LLR4, lib)
        hard = pyabi.line_from_fixinput(code.code, fix, n, pyabi.LINE_HARD, lib)
        llr4 = pyabi.line_to_llr4(code.code, soft, pyabi.LINE_LLR4, 0, n, lib)
        del fix
        d_soft, d_hard, d_llr4 = (torch.from_numpy(x.view(np.uint8)).cuda() for x in (soft, hard, llr4))
        torch.cuda.synchronize()
        calls = {
            "packed": lambda: dec.decode_codewords_packed_device(d_llr4.data_ptr(), ng, d_bits.data_ptr(), d_cw.data_ptr()),
            "line_llr4": lambda: dec.decode_line_device(d_soft.data_ptr(), pyabi.LINE_LLR4, n, d_pay.data_ptr(), None, d_st.data_ptr()),
            "line_hard": lambda: dec.decode_line_device(d_hard.data_ptr(), pyabi.LINE_HARD, n, d_pay.data_ptr(), None, d_st.data_ptr(), 4),
        }
        times = {k: [] for k in calls}
        for rep in range(a.reps + 2):
            for k, fn in calls.items():
                t = _ms(fn)
                if rep >= 2:
                    times[k].append(t)
        row = {"eb_n0": eb, "codewords": n, "method": 2, "reps": a.reps}
        for k in calls:
            row[k + "_ms"] = _summary(times[k])
        # what each call decoded: mean I / J, and for the LLR4 line the payload against the packed decisions
        calls["packed"]()
        cw = d_cw.cpu().numpy()
        row["packed_mean_I_J"] = [round(float(cw[:, 0].mean()), 3), round(float(cw[:, 1].mean()), 3)]
        want = d_bits.reshape(n, N // 32)[:, :K // 32].contiguous()
        for k in ("line_llr4", "line_hard"):
            calls[k]()
            st = d_st.cpu().numpy()
            row[k + "_mean_I_J"] = [round(float(st[:, 0].mean()), 3), round(float(st[:, 1].mean()), 3)]
            row[k + "_unsatisfied_codewords"] = int((st[:, 2] > 0).sum())
            if k == "line_llr4":
                row["payload_equals_packed"] = bool(torch.equal(d_pay.reshape(n, K // 32), want))
                row["stats_equal_packed"] = bool((st[:, :3] == cw).all())
        row["line_llr4_minus_packed_ms"] = round(row["line_llr4_ms"]["median"] - row["packed_ms"]["median"], 3)
        row["pass"] = row["line_llr4_minus_packed_ms"] <= FIXED_SHARE_MS
        ok &= row["pass"] and row["payload_equals_packed"] and row["stats_equal_packed"]
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del d_soft, d_hard, d_llr4
    dec.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
