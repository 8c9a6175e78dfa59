#!/usr/bin/env python3
"""Compare the gfx950 kernels of two assembly files that `hipcc -S --cuda-device-only` wrote for the same source at two
revisions:  tools/isa_diff.py old.s new.s

A kernel is the text from its `_Z...:` label to `.Lfunc_end`, without comments and empty lines, with the basic-block labels'
function index dropped and their numbers replaced by the order of first appearance (.LBB<n>_<m> -> .LBB_<k>: the same
instructions in the same order are the same kernel, whatever numbers the compiler gave its blocks) and every mangled name
replaced by a token.  Bodies are matched as a multiset, not by
name (a removed template parameter changes the mangled name): per kernel `same` / `DIFF` (same name, other body) / `gone` /
`new`, then the register and LDS / scratch sizes of each side.  Exit status 1 if anything is DIFF or new."""
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    out, name, body = [], None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and line.startswith(".Lfunc_end"):
            text = "\n".join(body)
            res = tuple(int(re.search(r"\.amdhsa_%s (\d+)" % k, text).group(1)) for k in RES)
            order = {}                  # a block label's number is a name: the n-th label to appear in the text is block n
            text = re.sub(r"\.LBB_\d+", lambda m: ".LBB_%d" % order.setdefault(m.group(0), len(order)), text)
            out.append((name, text, res))
            name = None
        elif name is not None:
            line = re.sub(r"_Z\w+", "<sym>", re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0])).strip()
            if line:
                body.append(line)
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
left = list(new)
count = {"same": 0, "DIFF": 0, "gone": 0, "new": 0}
for name, body, res in old:
    hit = next((k for k in left if k[1] == body), None) or next((k for k in left if k[0] == name), None)
    verdict = "gone" if hit is None else ("same" if hit[1] == body else "DIFF")
    if hit is not None:
        left.remove(hit)
    count[verdict] += 1
    print("%-4s %s  %s%s" % (verdict, name, res, "" if hit is None or hit[2] == res else " -> %s" % (hit[2],)))
for name, body, res in left:
    count["new"] += 1
    print("new  %s  %s" % (name, res))
print("%d -> %d kernels (%s): " % (len(old), len(new), ", ".join(RES)) + ", ".join("%d %s" % (v, k) for k, v in count.items()))
sys.exit(1 if count["DIFF"] or count["new"] else 0)
