#!/usr/bin/env python3
"""What one trip of the layer loop issues in the headline kernel lnsfaid_decode4_kernel<2, true, false>: the per-degree layer
block and everything around it (at two waves per SIMD the launch time follows the NUMBER of issued instructions).

usage: isa_layer_trip.py <kernel4.s> [kernel-name-substring]

The kernel's assembly is cut into straight-line pieces (a piece ends at a branch or in front of a label).  The two pieces with the
most VALU instructions are the degree-23 and degree-22 instances of the layer step; the one with 2 x degree v_alignbyte_b32 is
the instance of that degree.  The trip of a degree is the walk from the header of the innermost loop around that piece to the
piece and on to the loop's back edge:
  - pieces right in front of the block that a branch skips straight into it are counted (the patch of the old arg-min nodes,
    which only the first iteration skips);
  - everywhere else the walk takes the way that issues the fewest instructions (the other instances of the layer step and the
    rows' syndrome bits, wanted inside the error-floor window only, lie on longer ways).
Printed per degree as JSON: the block's VALU / LDS / s_waitcnt counts and, for the rest of the trip ("around"), the number of
instructions issued in all and per class.  tests/test_layer_trip_count.py pins these numbers.
"""
import heapq
import json
import re
import sys

HEADLINE = "lnsfaid_decode4_kernelILi2ELb1ELb0E"


def kernel_body(text, want=HEADLINE):
    parts = re.split(r"^(_Z\w+):", text, flags=re.M)
    bodies = [parts[i + 1].split(".end_amdhsa_kernel")[0] for i in range(1, len(parts) - 1, 2) if want in parts[i]]
    assert len(bodies) == 1, len(bodies)
    return bodies[0]


def pieces(body):
    """straight-line pieces: {"labels": [...], "ins": [...], "succ": [piece indices]}"""
    out, cur = [], {"labels": [], "ins": []}
    for raw in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):", raw)
        if m:
            if cur["ins"]:
                out.append(cur)
                cur = {"labels": [], "ins": []}
            cur["labels"].append(m.group(1))
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", raw)  # the compiler's own note on the label: innermost loop
            if h:
                cur["loop"] = ".L" + h.group(1)
            continue
        ins = raw.split(";")[0].strip()
        if not re.match(r"^[a-z]", ins):
            continue
        cur["ins"].append(ins)
        if ins.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            out.append(cur)
            cur = {"labels": [], "ins": []}
    if cur["ins"] or cur["labels"]:
        out.append(cur)
    where = {l: i for i, p in enumerate(out) for l in p["labels"]}
    for i, p in enumerate(out):
        last = p["ins"][-1] if p["ins"] else ""
        succ = []
        if last.startswith("s_cbranch"):
            succ = [i + 1, where[last.split()[1]]]  # fall through first
        elif last.startswith("s_branch"):
            succ = [where[last.split()[1]]]
        elif not last.startswith(("s_endpgm", "s_setpc")) and i + 1 < len(out):
            succ = [i + 1]
        p["succ"] = succ
    return out


def classes(ins):
    c = {"all": len(ins), "valu": 0, "salu": 0, "lds": 0, "vmem": 0, "smem": 0, "waitcnt": 0, "branch": 0, "rotates": 0}
    for i in ins:
        if i.startswith("v_"):
            c["valu"] += 1
            c["rotates"] += i.startswith("v_alignbyte_b32")
        elif i.startswith("ds_"):
            c["lds"] += 1
        elif re.match(r"(global|flat|buffer|scratch)_", i):
            c["vmem"] += 1
        elif i.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif i.startswith("s_waitcnt"):
            c["waitcnt"] += 1
        elif i.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif i.startswith("s_"):
            c["salu"] += 1
    return c


def loop_header(ps, blk):
    """header of the innermost loop around piece blk, as the compiler notes it on the piece's label"""
    note = ps[blk].get("loop")
    assert note is not None, "the layer block %s carries no 'in Loop: Header=' note: the compiler's label comments changed, " \
                             "this walk needs another way to find the layer loop" % ps[blk]["labels"]
    head = [i for i, p in enumerate(ps) if note in p["labels"]]
    assert len(head) == 1, "loop header %s of the layer block not found among the kernel's labels" % note
    return head[0]


def shortest(ps, src, dst):
    """pieces strictly between src and dst on the way that issues the fewest instructions"""
    cost = lambda i: 0 if i == dst else len(ps[i]["ins"])
    prev, heap = {}, [(cost(s), s, src) for s in ps[src]["succ"]]
    heapq.heapify(heap)
    while heap:
        d, i, frm = heapq.heappop(heap)
        if i in prev:
            continue
        prev[i] = frm
        if i == dst:
            break
        for s in ps[i]["succ"]:
            if s not in prev:
                heapq.heappush(heap, (d + cost(s), s, i))
    way, i = [], prev[dst]
    while i != src:
        way.append(i)
        i = prev[i]
    return way[::-1]


def trip(ps, blk):
    head = loop_header(ps, blk)
    first = blk  # pieces in front of the block that a branch skips straight into it: counted
    while first > head and ps[first - 1]["succ"][:1] == [first] and set(ps[first - 1]["succ"][1:]) <= set(range(first, blk + 1)):
        first -= 1
    front = list(range(first, blk))
    lead = ([head] + shortest(ps, head, first)) if first != head else []
    return lead + front + shortest(ps, blk, head)


def measure(text, want=HEADLINE):
    ps = pieces(kernel_body(text, want))
    big = sorted(range(len(ps)), key=lambda i: -classes(ps[i]["ins"])["valu"])[:2]
    out = {}
    for b in big:
        cb = classes(ps[b]["ins"])
        assert cb["rotates"] % 2 == 0
        around = trip(ps, b)
        ins = [x for i in around for x in ps[i]["ins"]]
        out[cb["rotates"] // 2] = {"block": cb, "around": classes(ins), "around_pieces": len(around),
                                   "gpr_idx_on": sum(1 for x in ins if x.startswith("s_set_gpr_idx_on"))}
    return out


if __name__ == "__main__":
    res = measure(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else HEADLINE)
    for deg in sorted(res, reverse=True):
        print(json.dumps({"degree": deg, **res[deg]}))
