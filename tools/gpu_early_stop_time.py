"""Group rule against per-codeword rule (README "Early stop per codeword").

    python tools/gpu_early_stop_time.py [--out DIR]

The parent process starts every GPU step as a child under its own `timeout` and stops at the first step that fails:
  decode  65 536 codewords resident in HBM, bench.py's synthetic LLRs (seed 1234): DecodeMethod 2 at 3.0 / 3.6 / 4.2 dB (QPSK,
          scale 13), DecodeMethod 5 at its BASELINE point (16-QAM, scale 12.5, 8.1 dB) and at 3.6 dB QPSK: per point both rules
          alternated in one process, 3 warm-up + 10 timed decode + error-counter steps each (median ms, decoded Gb/s), the mean
          per-codeword I / J of lnsfaid_decode_codewords, and the same codewords' I / J from the CPU port decoding groups of 32
          copies (tests/early_stop_ref.py) for a fixed random subset of 256 codewords per point
  sim     lnsfaid_sim --streams 2048 --max-rounds 1 --device-frontend at 3.4 and 3.6 dB, once per --early-stop rule
Prints one JSON line per measurement and writes them to DIR/early_stop_time.jsonl."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
SIM = os.path.join(PKG, "host", "lnsfaid_sim")
POINTS = [(2, 3.0, 2, 13.0), (2, 3.6, 2, 13.0), (2, 4.2, 2, 13.0), (5, 8.1, 4, 12.5), (5, 3.6, 2, 13.0)]  # method, Eb/N0, modType, scale
ORACLE_SUBSET = 256


def step_decode():
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle_abi as oa
    from early_stop_ref import per_codeword_oracle
    pyabi = oa.pyabi
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    ng = 2048
    d_out = torch.empty(ng * 32 * code.N, dtype=torch.int8, device="cuda")
    d_st = torch.zeros((ng, 2), dtype=torch.int32, device="cuda")
    d_cw = torch.zeros((ng * 32, 3), dtype=torch.int32, device="cuda")
    for method, eb, mod_type, scale in POINTS:
        d_fix = bench.synth_llr(torch, "cuda", ng, eb, 1234, mod_type, scale)
        torch.cuda.synchronize()
        cfg = pyabi.default_cfg(method, 10, lib)
        dec = pyabi.Decoder(code, cfg, 0, ng, lib)
        times = {0: [], 1: []}
        for rep in range(13):
            for rule in (0, 1):
                dec.set_early_stop(rule)
                t0 = time.perf_counter()
                dec.decode_device(d_fix.data_ptr(), ng, d_out.data_ptr(), d_st.data_ptr())
                dec.count_errors_device(d_out.data_ptr(), None, ng)
                if rep >= 3:
                    times[rule].append((time.perf_counter() - t0) * 1e3)
        dec.decode_codewords_device(d_fix.data_ptr(), ng, d_out.data_ptr(), d_cw.data_ptr())
        cw = d_cw.cpu().numpy()
        dec.set_early_stop(0)
        dec.decode_device(d_fix.data_ptr(), ng, d_out.data_ptr(), d_st.data_ptr())
        st = d_st.cpu().numpy()
        dec.close()
        sub = np.sort(np.random.default_rng(7).choice(ng * 32, ORACLE_SUBSET, replace=False))
        _, ost = per_codeword_oracle(code, cfg, d_fix.cpu().numpy().reshape(-1), ng, kind="avx2", cws=sub)
        for rule in (0, 1):
            t = sorted(times[rule])[len(times[rule]) // 2]
            res = {"step": "decode", "method": method, "eb_n0_db": eb, "mod_type": mod_type, "scale": scale,
                   "rule": ["group", "codeword"][rule], "ms": round(t, 3),
                   "Gbps": round(ng * 32 * code.K / t / 1e6, 2)}
            if rule == 0:
                res.update(mean_I_per_group=round(float(st[:, 0].mean()), 3), mean_J_per_group=round(float(st[:, 1].mean()), 3))
            else:
                res.update(mean_I_per_codeword=round(float(cw[:, 0].mean()), 3), mean_J_per_codeword=round(float(cw[:, 1].mean()), 3),
                           codewords_unsatisfied=int((cw[:, 2] > 0).sum()),
                           subset_codewords=ORACLE_SUBSET, subset_mean_I_gpu=round(float(cw[sub, 0].mean()), 3),
                           subset_mean_J_gpu=round(float(cw[sub, 1].mean()), 3), subset_mean_I_oracle=round(float(ost[:, 0].mean()), 3),
                           subset_mean_J_oracle=round(float(ost[:, 1].mean()), 3),
                           subset_IJ_identical=bool(np.array_equal(cw[sub, :2], ost)))
            print(json.dumps(res), flush=True)


def step_sim(rule, eb):
    with tempfile.TemporaryDirectory() as tmp:
        prof = open(os.path.join(PKG, "host", "Profile.txt")).read()
        prof = prof.replace("StartSNR: 3.3", "StartSNR: %g" % eb).replace("EndSNR: 3.85", "EndSNR: %g" % (eb + 0.05))
        with open(os.path.join(tmp, "Profile.txt"), "w") as f:
            f.write(prof)
        out = subprocess.run([SIM, "--streams", "2048", "--gpus", "1", "--max-rounds", "1", "--device-frontend", "--early-stop", rule],
                             cwd=tmp, capture_output=True, text=True, check=True).stdout
    row = [l for l in out.splitlines() if re.match(r"\s*%g\s" % eb, l)][-1].split()
    print(json.dumps({"step": "sim", "rule": rule, "eb_n0_db": eb, "point_s": float(row[7]), "TestFrame": int(row[1]),
                      "ErrorFrame": int(row[2]), "ErrorBits": int(row[3])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    ap.add_argument("--rule", default=None)
    ap.add_argument("--eb", type=float, default=None)
    a = ap.parse_args()
    if a.step == "decode":
        return step_decode()
    if a.step == "sim":
        return step_sim(a.rule, a.eb)
    lines = []
    steps = [(["--step", "decode"], 900)] + [(["--step", "sim", "--rule", r, "--eb", str(eb)], 120) for eb in (3.4, 3.6)
                                             for r in ("group", "codeword")]
    for args, limit in steps:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args,
                           capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            print("step %s failed with status %d: stopping" % (" ".join(args), p.returncode), file=sys.stderr)
            break
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "early_stop_time.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(lines) >= 2 * len(POINTS) + 4 else 1


if __name__ == "__main__":
    sys.exit(main())
