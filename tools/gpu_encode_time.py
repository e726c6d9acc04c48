"""Times of the device encoder and of random-codeword sweep points (README "Random codewords on the device").

    python tools/gpu_encode_time.py [--streams 2048] [--out DIR]

The parent process starts every GPU step as a child under its own `timeout` and stops at the first step that fails:
  api     (a) lnsfaid_frontend_random_frames for 256 and for --streams streams, (b) lnsfaid_encode_device for --streams groups:
          host clock around the synchronising call, median of 20 calls after 3 warm-up calls
  zero    (c) one lnsfaid_sim sweep point, --streams streams, --max-rounds 1, 3.6 dB, --device-frontend (all-zero codeword)
  encode  (c) the same with --encode --device-frontend (rand() messages, host encoder, frames uploaded)
  device  (c) the same with --device-encode --device-frontend
Prints one JSON line per step."""
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
MODES = {"zero": ["--device-frontend"], "encode": ["--encode", "--device-frontend"], "device": ["--device-encode", "--device-frontend"]}


def _median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2]


def step_api(streams):
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import ctypes as C
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    pyabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pyabi)
    lib = pyabi.load()
    code = pyabi.Code50GPON(lib)
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, streams, lib)
    res = {"step": "api", "streams": streams}
    for n in sorted({256, streams}):
        keys = (C.c_uint64 * n)(*[(s * 0x9E3779B97F4A7C15 + 1) & ((1 << 64) - 1) for s in range(n)])

        def rf():
            rc = lib.lnsfaid_frontend_random_frames(dec.ctx, keys, n)
            assert rc == 0, lib.lnsfaid_last_hip_error()
        res["random_frames_ms_%d" % n] = round(_median_ms(rf), 3)
    d_in = torch.randint(0, 2, (streams * 32 * code.K,), dtype=torch.int8, device="cuda")
    d_out = torch.empty(streams * 32 * code.N, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    res["encode_device_ms_%d" % streams] = round(_median_ms(lambda: dec.encode_device(d_in.data_ptr(), streams, d_out.data_ptr())), 3)
    # bytes written per group: frames 32 N + message bits 32 K (random frames), frames only (encode_device)
    res["random_frames_GB_%d" % streams] = round(streams * 32 * (code.N + code.K) / 1e9, 3)
    dec.close()
    print(json.dumps(res), flush=True)


def step_sim(mode, streams):
    with tempfile.TemporaryDirectory() as tmp:
        prof = open(os.path.join(PKG, "host", "Profile.txt")).read()
        prof = prof.replace("StartSNR: 3.3", "StartSNR: 3.6").replace("EndSNR: 3.85", "EndSNR: 3.65")
        with open(os.path.join(tmp, "Profile.txt"), "w") as f:
            f.write(prof)
        t0 = time.perf_counter()
        out = subprocess.run([SIM, "--streams", str(streams), "--gpus", "1", "--max-rounds", "1"] + MODES[mode], cwd=tmp,
                             capture_output=True, text=True, check=True).stdout
        wall = time.perf_counter() - t0
    row = [l for l in out.splitlines() if re.match(r"\s*3\.6\s", l)][-1].split()
    print(json.dumps({"step": mode, "streams": streams, "point_s": float(row[7]), "process_s": round(wall, 3),
                      "TestFrame": int(row[1]), "ErrorFrame": int(row[2]), "ErrorBits": int(row[3])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--step", choices=["api"] + list(MODES))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per step")
    a = ap.parse_args()
    if a.step == "api":
        return step_api(a.streams)
    if a.step:
        return step_sim(a.step, a.streams)
    for step in ["api"] + list(MODES):
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--streams", str(a.streams)]).returncode
        if rc != 0:
            print("step %s failed with exit status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
