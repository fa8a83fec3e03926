#!/usr/bin/env python3
"""Kernel by kernel, the ISA listings of two builds: identical or not, with static instruction counts.
usage: python scripts/isa_compare.py PARENT_DIR NEW_DIR
Each directory holds listings (*.s) of the same units, made with the Makefile's flags and
`--cuda-device-only -S` (what `make quick-usage` writes for one configuration). A kernel's text runs
from its label to its .Lfunc_end; the __hip_cuid_* symbol, which differs from compile to compile, is
masked. For every kernel: `identical`, or both builds' counts of VALU instructions (v_*), IEEE float
divisions (v_div_fmas_f32: one per division), square roots (v_sqrt_f32), reciprocals (v_rcp_f32) and
LDS instructions (ds_*), of the whole kernel and of its text after the second s_barrier (in an LDS-mode
kernel that bakes: the main body, without the staging and bake passes that run once per workgroup)."""
import re
import sys
from pathlib import Path


def kernels(path):
    out, name, body = {}, None, []
    for line in path.read_text().split("\n"):
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)
        if name is None:
            m = re.match(r"(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[name], name = body, None
        else:
            body.append(line)
    return out


def counts(body):
    ops = [l.split()[0] for l in body if l.startswith("\t") and not l.strip().startswith((";", "."))]
    n = lambda pred: sum(1 for o in ops if pred(o))
    return (f"VALU {n(lambda o: o.startswith('v_'))} div {n(lambda o: o == 'v_div_fmas_f32')} "
            f"sqrt {n(lambda o: o.startswith('v_sqrt_f32'))} rcp {n(lambda o: o.startswith('v_rcp_f32'))} "
            f"LDS {n(lambda o: o.startswith('ds_'))}")


def main():
    parent, new = Path(sys.argv[1]), Path(sys.argv[2])
    same = diff = 0
    for f in sorted(parent.glob("*.s"), key=lambda p: (len(p.name), p.name)):
        a, b = kernels(f), kernels(new / f.name)
        assert a.keys() == b.keys(), f.name
        for k in a:
            if a[k] == b[k]:
                same += 1
                print(f"{f.stem:10s} {k[:96]:96s} identical")
            else:
                diff += 1
                print(f"{f.stem:10s} {k[:96]:96s} DIFFERS")
                for who, body in (("new", b[k]), ("parent", a[k])):
                    bars = [i for i, l in enumerate(body) if "s_barrier" in l]
                    main_body = body[bars[1]:] if len(bars) > 1 else body
                    print(f"{'':12s}{who:7s} whole: {counts(body)};  after the 2nd barrier: {counts(main_body)}")
    print(f"{same} kernels identical, {diff} differ")


if __name__ == "__main__":
    main()
