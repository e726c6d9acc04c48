"""Packed decode I/O against the int8 entry points (README "Packed decode I/O"), shaped like tools/gpu_host_path.py.

    python tools/gpu_packed_io_time.py --parent-lib OLD/liblnsfaid.so [--part host|device|all] [--runs 5] [--groups 2048]

OLD is a liblnsfaid.so built from the parent commit.  The parent process starts every GPU step as a child under its own
`timeout` and stops at the first step that fails (tools/gpu_encode_time.py).  One child = one process = one measurement:
  host    `--groups` groups of bench.py synth_llr LLRs at 3.0 and 3.6 dB, host buffers (pinned with torch, or pageable).  OLD's
          lnsfaid_decode (int8) alternates with this tree's lnsfaid_decode_packed, --runs processes each; host clock around the
          synchronous call, median of 3 calls after 2 warm-up calls; also the kernel time of the decode pieces.
  device  the same batch resident in HBM at 3.0, 3.6 and 4.2 dB: OLD's lnsfaid_decode_device + lnsfaid_count_errors_device
          against lnsfaid_decode_packed_device + lnsfaid_count_errors_packed_device, median of 5 calls after 2 warm-up calls.
Every child prints a JSON line with a hash of its decisions in packed form (int8 output: bit b of word w = byte 32 w + b); the
parent checks that the hashes of both libraries agree per Eb/N0, and prints the pass conditions:
  host: slowest packed pinned run < fastest int8 pinned run; device: packed median <= int8 median + int8 spread (max - min).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd")
NEW_LIB = os.path.join(PKG, "csrc", "liblnsfaid.so")


def _pyabi():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_pyabi", os.path.join(PKG, "pyabi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lnsfaid_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _packed_hash(torch, dec_bytes_or_words, packed):
    """sha256 (16 hex digits) of the decisions as packed words"""
    t = dec_bytes_or_words.to("cuda")
    if not packed:
        assert int(t.min()) >= 0 and int(t.max()) <= 1
        w = torch.tensor([1 << b for b in range(32)], dtype=torch.int64, device=t.device)
        t = (t.reshape(-1, 32).to(torch.int64) * w).sum(1).to(torch.int64)
        arr = t.cpu().numpy().astype("<u4")
    else:
        arr = t.cpu().numpy().view("<u4")
    return hashlib.sha256(arr.tobytes()).hexdigest()[:16]


def _pack_llr4(torch, x):
    """int8 LLRs -> llr4 bytes (element e in byte e / 2, low nibble for even e), on x's device"""
    u = x.reshape(-1).to(torch.int16) & 15
    return (u[0::2] | (u[1::2] << 4)).to(torch.uint8)


def _timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def child(a):
    import torch
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    pyabi = _pyabi()
    raw = C.CDLL(a.lib)
    lib = pyabi.bind(raw, {k: v for k, v in pyabi.SYMBOLS.items() if hasattr(raw, k)})
    code = pyabi.Code50GPON(lib)
    ng, N, K = a.groups, code.N, code.K
    dec = pyabi.Decoder(code, pyabi.default_cfg(2, 10, lib), 0, ng, lib)
    x = _bench().synth_llr(torch, "cuda", ng, a.eb, seed=3)
    packed = a.api == "packed"
    res = {"part": a.part, "api": a.api, "lib": "new" if os.path.abspath(a.lib) == NEW_LIB else "parent", "eb_n0": a.eb,
           "groups": ng}
    if a.part == "host":
        src = (_pack_llr4(torch, x) if packed else x.reshape(-1)).cpu()
        dst = torch.empty(ng * N if packed else ng * 32 * N, dtype=torch.int32 if packed else torch.int8)
        if a.mem == "pinned":
            src, dst = src.pin_memory(), dst.pin_memory()
        res["mem"] = a.mem
        stats = (C.c_int32 * (2 * ng))()
        fn = lib.lnsfaid_decode_packed if packed else lib.lnsfaid_decode

        def call():
            assert fn(dec.ctx, src.data_ptr(), ng, dst.data_ptr(), stats) == 0, lib.lnsfaid_last_hip_error()
        dec.kernel_time(reset=True)
        res["ms"] = round(_timed(call, 3, 2), 3)
        ms, launches = dec.kernel_time(reset=True)
        res["kernel_ms_per_call"] = round(ms / 5, 3)
        res["bytes_in_out"] = src.numel() * src.element_size() + dst.numel() * dst.element_size()
        res["hash"] = _packed_hash(torch, dst, packed)
    else:
        d_in = _pack_llr4(torch, x) if packed else x.reshape(-1)
        d_out = torch.empty(ng * N if packed else ng * 32 * N, dtype=torch.int32 if packed else torch.int8, device="cuda")
        torch.cuda.synchronize()
        counters = (C.c_uint64 * 4)()

        def call():
            for i in range(4):
                counters[i] = 0
            if packed:
                assert lib.lnsfaid_decode_packed_device(dec.ctx, d_in.data_ptr(), ng, d_out.data_ptr(), None) == 0
                assert lib.lnsfaid_count_errors_packed_device(dec.ctx, d_out.data_ptr(), None, ng, counters) == 0
            else:
                assert lib.lnsfaid_decode_device(dec.ctx, d_in.data_ptr(), ng, d_out.data_ptr(), None) == 0
                assert lib.lnsfaid_count_errors_device(dec.ctx, d_out.data_ptr(), None, ng, counters) == 0
        res["ms"] = round(_timed(call, 5, 2), 3)
        res["counters"] = list(counters)
        res["hash"] = _packed_hash(torch, d_out, packed)
    dec.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--part", choices=["host", "device", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per step")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=NEW_LIB)
    ap.add_argument("--api", choices=["int8", "packed"])
    ap.add_argument("--mem", choices=["pinned", "pageable"], default="pinned")
    ap.add_argument("--eb", type=float, default=3.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    old = os.path.abspath(a.parent_lib)
    plan = []
    if a.part in ("host", "all"):
        for eb in (3.0, 3.6):
            for _ in range(a.runs):
                plan += [("host", old, "int8", "pinned", eb), ("host", NEW_LIB, "packed", "pinned", eb)]
            plan += [("host", old, "int8", "pageable", eb), ("host", NEW_LIB, "packed", "pageable", eb)]
    if a.part in ("device", "all"):
        for eb in (3.0, 3.6, 4.2):
            for _ in range(a.runs):
                plan += [("device", old, "int8", "pinned", eb), ("device", NEW_LIB, "packed", "pinned", eb)]
    rows = []
    for part, lib, api, mem, eb in plan:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--part", part, "--lib", lib,
               "--api", api, "--mem", mem, "--eb", str(eb), "--groups", str(a.groups)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print("step %s %s %s %s failed with exit status %d: stopping" % (part, api, mem, eb, p.returncode), file=sys.stderr)
            return p.returncode
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    ok = True
    for part in ("host", "device"):
        for eb in sorted({r["eb_n0"] for r in rows if r["part"] == part}):
            sel = [r for r in rows if r["part"] == part and r["eb_n0"] == eb]
            hashes = {r["hash"] for r in sel}
            same = len(hashes) == 1
            ok &= same
            pin = [r for r in sel if r.get("mem", "pinned") == "pinned"]
            old_ms = [r["ms"] for r in pin if r["api"] == "int8"]
            new_ms = [r["ms"] for r in pin if r["api"] == "packed"]
            summ = {"summary": part, "eb_n0": eb, "decisions_equal": same, "int8_ms": old_ms, "packed_ms": new_ms,
                    "int8_median": statistics.median(old_ms), "packed_median": statistics.median(new_ms),
                    "ratio_of_medians": round(statistics.median(old_ms) / statistics.median(new_ms), 3)}
            if part == "host":
                summ["pass"] = max(new_ms) < min(old_ms)
                summ["pageable_ms"] = {r["api"]: r["ms"] for r in sel if r.get("mem") == "pageable"}
                summ["packed_kernel_ms"] = [r["kernel_ms_per_call"] for r in pin if r["api"] == "packed"]
            else:
                summ["pass"] = statistics.median(new_ms) <= statistics.median(old_ms) + (max(old_ms) - min(old_ms))
                summ["counters_equal"] = len({tuple(r["counters"]) for r in sel}) == 1
                ok &= summ["counters_equal"]
            ok &= summ["pass"]
            print(json.dumps(summ), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
