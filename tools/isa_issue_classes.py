#!/usr/bin/env python3
"""Cost accounting of ONE straight-line layer of the window-free kernel lnsfaid_decode4w_kernel<2>: the opcode
histogram of the layer, every opcode's issue class by the measured table (tools/ubench/issue_mix.hip, two waves per SIMD:
profiles/r23_class_moves/ubench_issue_classes.txt), and every VALU instruction that reads an SGPR or VCC, with the source line it was
compiled from.  A classification by opcode and operand kind, nothing else.

usage: isa_issue_classes.py [--form middle|first] [--layer N] [--extra "-DFLAG ..."] [--asm file.s]

Without --asm the tool compiles lnsfaid_kernel4w.hip for gfx950 with the Makefile's flags plus -gline-tables-only, which adds the
.loc lines the source column is read from and leaves the instructions alone.  measure() is what tests/test_class_moves_isa.py calls.
"""
import argparse
import collections
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mod-interleaveavx_multithreads-faid_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lnsfaid_decode4w_kernelILi2EE"

# SIMD cycles per wave64 instruction at two waves per SIMD, one class per kernel (profiles/r23_class_moves/ubench_issue_classes.txt;
# the older rows: profiles/r03/ubench_issue_mix_vs_occupancy.txt, profiles/r18_mask_pairs/ubench_shift_forms.txt)
FULL, SLOW = 3.4, 6.0
SLOW_OPS = ("v_perm_b32", "v_alignbyte_b32", "v_alignbit_b32", "v_add3_u32", "v_and_or_b32", "v_lshl_or_b32", "v_lshl_add_u32", "v_add_lshl_u32",
            "v_or3_b32", "v_bfi_b32", "v_bfe_", "v_lshlrev_b32", "v_lshlrev_b64", "v_lshrrev_b64", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_u32_u24",
            "v_mul_i32_i24", "v_mad_", "v_cndmask_b32", "v_readlane_b32", "v_readfirstlane_b32", "v_writelane_b32", "v_pk_", "v_xad_u32")
SGPR = re.compile(r"^(s\d+|s\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?|m0|ttmp\d+)$")


def compile_asm(extra=""):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernel4w.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-gline-tables-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
                       + shlex.split(extra) + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "lnsfaid_kernel4w.hip")],
                       check=True, capture_output=True)
        return open(out).read()


def kernel_body(text, want=HEADLINE):
    parts = re.split(r"^(_Z\w+):", text, flags=re.M)
    bodies = [parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if want in parts[i]]
    assert len(bodies) == 1, len(bodies)
    return bodies[0]


def layer_lines(text, form="middle", layer=0):
    """[(instruction, (file number, line) or None)] of one layer of one form of the headline instance"""
    body = kernel_body(text)
    region = body[body.index("; lf4w %s begin" % form):body.index("; lf4w %s end" % form)]
    out, cur, loc = [], None, None
    for raw in region.split("\n"):
        m = re.search(r";\s*lf4w layer (\d+)", raw)
        if m:
            cur = int(m.group(1))
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", raw)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        ins = raw.split(";")[0].strip()
        if cur == layer and re.match(r"^[a-z]", ins):
            out.append((ins, loc))
    return out


def operands(ins):
    parts = ins.split(None, 1)
    if len(parts) < 2:
        return parts[0], [], []
    ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", parts[1])]
    ops = [o.split()[0] if o else o for o in ops]  # modifiers (bitop3:0x96, op_sel ...) follow the last operand
    ndst = 2 if "_co_" in parts[0] else 1
    return parts[0], ops[:ndst], ops[ndst:]


def cost_class(op, srcs):
    """("full" | "slow" | "slow(sgpr)", cycles): the opcode's class, or the slow class for a full-rate opcode with a scalar source"""
    if not op.startswith("v_"):
        return "other", 0.0
    if any(op.startswith(s) for s in SLOW_OPS):
        return "slow", SLOW
    if any(SGPR.match(s) for s in srcs) and not op.startswith("v_cmp"):
        return "slow(sgpr)", SLOW
    return "full", FULL


def measure(text, form="middle", layer=0):
    lines = layer_lines(text, form, layer)
    hist, cls_of, sgpr_readers = collections.Counter(), {}, []
    cycles = collections.Counter()
    for ins, loc in lines:
        op, _, srcs = operands(ins)
        cls, cyc = cost_class(op, srcs)
        hist[op] += 1
        cycles[cls] += cyc
        cls_of.setdefault(op, set()).add(cls)
        if op.startswith("v_") and any(SGPR.match(s) for s in srcs):
            sgpr_readers.append((ins, loc, cls))
    return {
        "instructions": len(lines),
        "valu": sum(n for op, n in hist.items() if op.startswith("v_")),
        "hist": hist,
        "classes": cls_of,
        "cycles": dict(cycles),
        "sgpr_readers": sgpr_readers,
        "shl_b32": hist["v_lshlrev_b32_e32"] + hist["v_lshlrev_b32_e64"] + hist["v_lshlrev_b32"],
        "full_rate_with_sgpr": sum(1 for _, _, c in sgpr_readers if c == "slow(sgpr)"),
        "s_nop": sum(n for op, n in hist.items() if op.startswith("s_nop")),
    }


def source_files(text):
    files = {}
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', text, flags=re.M):
        files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="middle")
    ap.add_argument("--layer", type=int, default=0)
    ap.add_argument("--extra", default="")
    ap.add_argument("--asm")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_asm(a.extra)
    r = measure(text, a.form, a.layer)
    files, cache = source_files(text), {}

    def src_line(loc):
        if loc is None or loc[0] not in files:
            return "?"
        path = files[loc[0]]
        if path not in cache:
            try:
                cache[path] = open(path if os.path.isabs(path) else os.path.join(CSRC, path)).read().split("\n")
            except OSError:
                cache[path] = []
        body = cache[path][loc[1] - 1].strip() if 0 < loc[1] <= len(cache[path]) else ""
        return "%s:%d  %s" % (os.path.basename(path), loc[1], body[:110])

    print("lnsfaid_decode4w_kernel<2>, %s form, layer %d%s: %d instructions, %d VALU" % (a.form, a.layer, " (%s)" % a.extra if a.extra else "",
                                                                                       r["instructions"], r["valu"]))
    print("\nopcode histogram (class by tools/ubench/issue_mix, two waves per SIMD: full %.1f, slow %.1f SIMD cycles):" % (FULL, SLOW))
    for op, n in r["hist"].most_common():
        print("  %-24s %4d  %s" % (op, n, " + ".join(sorted(r["classes"][op]))))
    print("\nclass-weighted VALU issue cycles: %s = %.0f" % (", ".join("%s %.0f" % kv for kv in sorted(r["cycles"].items()) if kv[1]),
                                                           sum(r["cycles"].values())))
    print("single v_lshlrev_b32: %d; full-rate opcodes with an SGPR / VCC source: %d; s_nop: %d" % (r["shl_b32"], r["full_rate_with_sgpr"], r["s_nop"]))
    print("\nVALU instructions with an SGPR or VCC source (%d):" % len(r["sgpr_readers"]))
    for ins, loc, cls in r["sgpr_readers"]:
        print("  %-62s %-10s %s" % (ins, cls, src_line(loc)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
