#!/usr/bin/env python3
"""What one layered iteration of the layer-static kernel lnsfaid_decode4s_kernel<2> issues OUTSIDE its twelve layers (DESIGN.md
3.1f): from the kernel's comment line "lf4s layers end" over the loop's back edge, the decision point and the iteration's set-up to
"lf4s layers begin".

usage: isa_decision_point.py <kernel4s.s> [kernel-name-substring]

The way walked is the one an iteration after the first takes outside the error-floor window on the group's front with the first
stage of the cheap "certainly dirty" test (comment line "lf4s check stage 1") reporting dirty: the way with the fewest issued
instructions from the end of the layers to stage 1, stage 1 itself, and the way with the fewest instructions from there to the
layers - which leaves out stage 2 ("lf4s check stage 2"), the plane build and the full syndrome.  The kernel's assembly is cut
into straight-line pieces by tools/isa_layer_trip.py, with the four comment lines as additional cuts.
Printed as JSON: instructions in all and per class on the way, inside stage 1, the scalar loads on the way with their operands, and
how many of them are directly followed by a wait for the scalar / LDS counter.  tests/test_decision_point_isa.py pins these.
"""
import importlib.util
import json
import os
import re
import sys

HEADLINE = "lnsfaid_decode4s_kernelILi2EE"
MARKS = {"end": "lf4s layers end", "stage1": "lf4s check stage 1", "stage2": "lf4s check stage 2", "begin": "lf4s layers begin"}


def _trip_tool():
    spec = importlib.util.spec_from_file_location("isa_layer_trip", os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_layer_trip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def marked_pieces(body, tool):
    """the kernel's straight-line pieces with every comment line of MARKS turned into a cut; returns (pieces, {mark: piece index})"""
    lines, names = [], {}
    for raw in body.split("\n"):
        for key, text in MARKS.items():
            if re.match(r"^\s*;\s*%s\s*$" % re.escape(text), raw):
                assert key not in names, "comment line '%s' more than once in the kernel" % text
                names[key] = ".LBB99999_%d" % len(names)
                lines.append(names[key] + ":")
        lines.append(raw)
    ps = tool.pieces("\n".join(lines))
    at = {key: [i for i, p in enumerate(ps) if lab in p["labels"]] for key, lab in names.items()}
    assert all(len(v) == 1 for v in at.values()), at
    return ps, {key: v[0] for key, v in at.items()}


def waited_alone(ins):
    """scalar loads directly followed by a wait for the scalar / LDS counter to drain: a round trip nothing else is in flight with"""
    return sum(1 for a, b in zip(ins, ins[1:]) if a.startswith(("s_load", "s_buffer_load")) and re.match(r"s_waitcnt\s.*lgkmcnt\(0\)", b))


def measure(text, want=HEADLINE):
    tool = _trip_tool()
    ps, at = marked_pieces(tool.kernel_body(text, want), tool)
    assert set(at) == set(MARKS), sorted(at)
    way = [at["end"]] + tool.shortest(ps, at["end"], at["stage1"]) + [at["stage1"]] + tool.shortest(ps, at["stage1"], at["begin"])
    assert at["stage2"] not in way and at["begin"] not in way
    # stage 1 is straight-line: from its comment line to the branch on its ballot
    assert ps[at["stage1"]]["ins"][-1].startswith("s_cbranch"), ps[at["stage1"]]["ins"][-1]
    ins = [x for i in way for x in ps[i]["ins"]]
    stage1 = ps[at["stage1"]]["ins"]
    return {"way": tool.classes(ins), "way_pieces": len(way), "cond_branches": sum(1 for x in ins if x.startswith("s_cbranch")),
            "scalar_loads": [x for x in ins if x.startswith(("s_load", "s_buffer_load"))], "waited_alone": waited_alone(ins),
            "stage1": tool.classes(stage1), "stage1_waited_alone": waited_alone(stage1),
            "stage2": tool.classes(ps[at["stage2"]]["ins"])}


def loop_span(text, want):
    """the kernels that run their layers through a loop (lnsfaid_kernel4.hip, lnsfaid_kernel4z.hip): the instructions laid out from
    the header of the layered loop (the loop around the layer loop) to the header of the layer loop - the decision point with its
    cheap test and syndrome stage, and the iteration's set-up"""
    tool = _trip_tool()
    body = tool.kernel_body(text, want)
    ps = tool.pieces(body)
    blk = max(range(len(ps)), key=lambda i: tool.classes(ps[i]["ins"])["valu"])  # an instance of the layer step
    inner = ps[tool.loop_header(ps, blk)]["labels"]
    lines = body.split("\n")
    at = [n for n, raw in enumerate(lines) if re.match(r"^(%s):" % "|".join(re.escape(x) for x in inner), raw)]
    assert at, inner
    parent = re.search(r"Parent Loop (BB\d+_\d+)", lines[at[0]])
    assert parent, "the layer loop is not inside another loop: %s" % lines[at[0]]
    top = [n for n, raw in enumerate(lines) if raw.startswith(".L" + parent.group(1) + ":")]
    assert len(top) == 1 and top[0] < at[0], (top, at)
    ins = [raw.split(";")[0].strip() for raw in lines[top[0]:at[0]]]
    ins = [x for x in ins if re.match(r"^[a-z]", x)]
    return {"span": tool.classes(ins), "waited_alone": waited_alone(ins)}


if __name__ == "__main__":
    print(json.dumps(measure(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else HEADLINE), indent=1))
