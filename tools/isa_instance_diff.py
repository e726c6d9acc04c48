#!/usr/bin/env python3
"""Compare the instruction text of every kernel instance of one source file between two source trees.

    python tools/isa_instance_diff.py [--rename OLD=NEW ...] OLD_CSRC NEW_CSRC lnsfaid_kernel4.hip [lnsfaid_kernel4cw.hip ...]

Each file is compiled for gfx950 with the Makefile's flags (-O3 -std=c++17, device code only) in both trees.  Labels,
comments, directives and blank lines are dropped; what is left of every kernel body is counted and hashed.  Prints one line per
instance (old count / hash, new count / hash, same or DIFFERENT) and exits 1 when an instance differs or exists in one tree only.

Instances are paired by mangled name.  --rename OLD=NEW (repeatable) replaces OLD by NEW in the old tree's names first, for a type in
a kernel's signature that was renamed: --rename 7LsTable=8LnkTable.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def instances(csrc, name, tmp):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    out = os.path.join(tmp, name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + inc, "-I" + csrc, "-S", "--cuda-device-only",
                    "-o", out, os.path.join(csrc, name)], check=True)
    asm = open(out).read()
    parts = re.split(r"^(_Z\w+):", asm, flags=re.M)
    res = {}
    for i in range(1, len(parts) - 1, 2):
        body = parts[i + 1].split(".Lfunc_end")[0]
        ins = []
        for line in body.split("\n"):
            s = line.split(";")[0].strip()
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            ins.append(re.sub(r"\.LBB\d+_\d+", "L", s))  # branch targets by position, not by label number
        res[parts[i]] = ins
    return res


def main():
    args, renames = sys.argv[1:], []
    while args and args[0] == "--rename":
        renames.append(args[1].split("=", 1))
        args = args[2:]
    old_dir, new_dir, files = args[0], args[1], args[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            os.makedirs(os.path.join(tmp, "old"), exist_ok=True)
            os.makedirs(os.path.join(tmp, "new"), exist_ok=True)
            a = instances(old_dir, f, os.path.join(tmp, "old"))
            for old, new in renames:
                a = {name.replace(old, new): ins for name, ins in a.items()}
            b = instances(new_dir, f, os.path.join(tmp, "new"))
            print("# %s" % f)
            for name in sorted(set(a) | set(b)):
                ha = hashlib.sha256("\n".join(a[name]).encode()).hexdigest()[:16] if name in a else "-"
                hb = hashlib.sha256("\n".join(b[name]).encode()).hexdigest()[:16] if name in b else "-"
                same = name in a and name in b and a[name] == b[name]
                bad += 0 if same else 1
                print("%-60s old %6s %s  new %6s %s  %s" % (name, len(a.get(name, [])), ha, len(b.get(name, [])), hb,
                                                            "same" if same else "DIFFERENT"))
    print("instances that differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
