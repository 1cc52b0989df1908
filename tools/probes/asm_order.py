#!/usr/bin/env python3
"""Development probe: instruction order of one kernel in `hipcc -S` output, as run lengths by class and basic block.

usage: asm_order.py FILE.s KERNEL_SUBSTRING
M fp32/bf16 MFMA, T transcendental, V other vector ALU, R LDS read, W LDS write, G global memory, S scalar, B s_barrier,
w s_waitcnt.  "M1 V1" x 80 reads as eighty pairs of one MFMA and one vector instruction.
"""
import re, sys


def cls(op):
    if op.startswith("v_mfma"): return "M"
    if re.match(r"v_(exp|rcp|log|sqrt|rsq|sin|cos)_", op): return "T"
    if op.startswith("v_"): return "V"
    if op.startswith("ds_read") or op.startswith("ds_load"): return "R"
    if op.startswith("ds_"): return "W"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "G"
    if op == "s_barrier": return "B"
    if op == "s_waitcnt": return "w"
    if op.startswith("s_"): return "S"
    return "?"


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_\S*%s\S*:" % re.escape(key), l))
    blocks, cur = [], ("entry", [])
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"): break
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            blocks.append(cur); cur = (m.group(1), [])
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)", l)
        if m and not l.lstrip().startswith("."): cur[1].append(cls(m.group(1)))
    blocks.append(cur)
    for name, seq in blocks:
        if not seq: continue
        runs = []
        for c in seq:
            if c in "wS": continue
            if runs and runs[-1][0] == c: runs[-1][1] += 1
            else: runs.append([c, 1])
        toks = ["%s%d" % (c, k) for c, k in runs]
        # fold repeated pairs
        out, i = [], 0
        while i < len(toks):
            k = 1
            while i + 2 * k + 1 < len(toks) and toks[i + 2 * k:i + 2 * k + 2] == toks[i:i + 2]: k += 1
            if k > 1: out.append("(%s %s)x%d" % (toks[i], toks[i + 1], k)); i += 2 * k
            else: out.append(toks[i]); i += 1
        n = {c: seq.count(c) for c in "MTVRWGB"}
        print("%s: %s\n    %s" % (name, " ".join("%s=%d" % kv for kv in n.items() if kv[1]), " ".join(out)))


if __name__ == "__main__":
    main()
