#!/usr/bin/env python3
"""Static instruction count of one node step of the traversal loop of a kernel.
usage: python scripts/node_step_count.py julia-raytracer_amd/build/jt_kv0.s <mangled kernel name substring> [show]
A step = the text between the last stack write of one unrolled pop and the last stack write of the
next (the four unrolled pops repeat the same text). Counted: VALU (v_*), SALU (s_* without
s_waitcnt / s_nop), LDS (ds_*), exec branches (s_cbranch_*), waits/nops apart."""
import re, sys
path, kern = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and kern in l and l.rstrip().split(":")[0].endswith("E"))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end]
w = [i for i, l in enumerate(body) if re.match(r"\s+ds_write_b32 v\d+, v\d+$", l)]
# runs of equal spacing: the unrolled pops
best = None
for a in range(len(w)):
    for b in range(a + 1, len(w)):
        d = w[b] - w[a]
        if d < 60 or d > 400: continue
        if w[a] + 2 * d in w and w[a] + 3 * d in w:
            best = (w[a], d); break
    if best: break
if not best:
    sys.exit("no unrolled steps found")
a, d = best
seg = body[a + d + 1: a + 2 * d + 1]
c = dict(valu=0, salu=0, lds=0, branch=0, wait=0, other=0)
for l in seg:
    t = l.strip()
    if not t or t.startswith((";", ".")) or t.endswith(":"): continue
    op = t.split()[0]
    if op in ("s_waitcnt", "s_nop"): c["wait"] += 1
    elif op.startswith("s_cbranch"): c["branch"] += 1; c["salu"] += 1
    elif op.startswith("v_"): c["valu"] += 1
    elif op.startswith("s_"): c["salu"] += 1
    elif op.startswith("ds_"): c["lds"] += 1
    else: c["other"] += 1
print(f"{kern}: step of {d} lines at +{a + d + 1}: VALU {c['valu']} SALU {c['salu']} (of them exec branches {c['branch']}) LDS {c['lds']} waits/nops {c['wait']} other {c['other']}")
if len(sys.argv) > 3:
    print("\n".join(seg))
