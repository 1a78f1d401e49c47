#!/usr/bin/env python3
"""asm_diff.py -- compare the device assembly of two builds of render_hip.hip, kernel by kernel.

    make -C ceres-raytracer_amd/csrc asm          # in both trees: build/asm/render_hip.s + resource-usage.txt
    tools/asm_diff.py OLD/build/asm NEW/build/asm [--may-differ ceres_trace_rays_k]
    tools/asm_diff.py OLD/build/asm64 NEW/build/asm64 --unit render64 [--may-differ ceres_trace_rays64_k]
    tools/asm_diff.py OLD/build/asm_order NEW/build/asm_order --unit ray_order

For every kernel symbol the function body in render_hip.s (label to end-of-function label) and
its block in resource-usage.txt (source positions stripped) must be equal line for line, except
for the kernels whose name contains a --may-differ string: for those the resource usage of both
builds is printed side by side instead.  Exit status 1 when any other kernel differs or is missing
on one side.  A text comparison only: a refactor that claims to leave kernels alone shows it here."""
import argparse
import os
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")   # local labels carry the function's running number
LOOP_NOTE = re.compile(r"\bBB\d+_")                          # ... and so do the loop comments ("Header=BB128_5"): kernels
                                                            # emitted behind a new one are renumbered, nothing else
LABEL_PAD = re.compile(r"^(\.LBB_\d+:)\s+;")                 # ... and a number that gains a digit (99 -> 100) moves the
                                                            # label's comment column by one space


def bodies(path):
    """{symbol: [lines]} for every global function of an AMDGPU .s file."""
    out, cur = {}, None
    for line in open(path):
        line = line.rstrip("\n")
        if cur is None:
            m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
            if m and not line.startswith(".L"):
                cur = m.group(1)
                out[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = LOOP_NOTE.sub("BB_", LOCAL.sub(lambda m: ".L" + m.group(1), line))
        out[cur].append(LABEL_PAD.sub(r"\1 ;", line))
    return out


def usage(path):
    """{symbol: {field: value}} from a -Rpass-analysis=kernel-resource-usage log."""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--may-differ", action="append", default=[], help="substring of kernel names allowed to differ")
    ap.add_argument("--unit", default="render_hip", help="the translation unit: <dir>/<unit>.s (render_hip, render64)")
    a = ap.parse_args()
    b0, b1 = (bodies(os.path.join(d, a.unit + ".s")) for d in (a.old, a.new))
    u0, u1 = (usage(os.path.join(d, "resource-usage.txt")) for d in (a.old, a.new))
    kernels = sorted(set(u0) | set(u1))
    bad, free, same = [], [], 0
    for k in kernels:
        if any(s in k for s in a.may_differ):
            free.append(k)
        elif k not in b0 or k not in b1 or b0[k] != b1[k] or u0.get(k) != u1.get(k):
            bad.append(k)
        else:
            same += 1
    print(f"{len(kernels)} kernels: {same} equal (body and resource usage), {len(free)} allowed to differ, {len(bad)} DIFFER")
    for k in bad:
        print("  DIFFERS:", k)
    fields = ["VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
              "Occupancy [waves/SIMD]"]
    for k in free:
        o, n = u0.get(k, {}), u1.get(k, {})
        body = "body equal" if b0.get(k) == b1.get(k) else f"body {len(b0.get(k, []))} -> {len(b1.get(k, []))} lines"
        print(f"  {k}: {body}")
        print("     " + "  ".join(f"{f.split(' [')[0]} {o.get(f, '-')} -> {n.get(f, '-')}" for f in fields))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
