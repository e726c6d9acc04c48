#!/usr/bin/env python3
"""What one iteration of the bit-flipping stage issues in the layer-static kernel lnsfaid_decode4s_kernel<2>: the
stage's loop on the cached path is the loop of the kernel, outside the layered loop, that holds both a population count (the
syndrome's unsatisfied checks) and v_alignbit_b32 on three or more LDS words per lane before a ds_write (the flip); it is found as
the innermost loop with the most v_alignbit_b32 among those with a v_bcnt_u32_b32.

usage: isa_bf_stage.py <kernel4s.s> [kernel-name-substring]

Printed as JSON: the instructions of all pieces that lie on a way from the loop's header back to it (classes of tools/isa_layer_trip.py) and the
conditional branches among them.  Laid out, not issued: an iteration skips the bodies of the thresholds it does not have."""
import importlib.util
import json
import os
import re
import sys

HEADLINE = "lnsfaid_decode4s_kernelILi2EE"


def _trip_tool():
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_layer_trip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reach(succ, start):
    seen, todo = set(), list(start)
    while todo:
        i = todo.pop()
        if i not in seen:
            seen.add(i)
            todo.extend(succ[i])
    return seen


def measure(text, want=HEADLINE):
    tool = _trip_tool()
    body = tool.kernel_body(text, want)
    ps = tool.pieces(body)
    inner = re.findall(r"^(\.LBB\d+_\d+):\s*; =>This Inner Loop Header", body, flags=re.M)  # loops that hold no other
    succ = [p["succ"] for p in ps]
    pred = [[] for _ in ps]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    best = None
    for label in inner:
        head = [i for i, p in enumerate(ps) if label in p["labels"]][0]
        loop = sorted(_reach(succ, succ[head]) & _reach(pred, pred[head]) | {head})  # the pieces on a way from the header back to it
        ins = [x for i in loop for x in ps[i]["ins"]]
        if not any(x.startswith("v_bcnt_u32_b32") for x in ins):
            continue
        n_align = sum(1 for x in ins if x.startswith("v_alignbit_b32"))
        if best is None or n_align > best[0]:
            best = (n_align, label, ins, len(loop))
    assert best, "no innermost loop with a population count"
    _, label, ins, n = best
    return {"header": label, "pieces": n, "laid_out": tool.classes(ins), "cond_branches": sum(1 for x in ins if x.startswith("s_cbranch"))}


if __name__ == "__main__":
    print(json.dumps(measure(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else HEADLINE), indent=1))
