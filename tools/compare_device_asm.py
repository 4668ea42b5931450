#!/usr/bin/env python3
"""Are two device-assembly files (hipcc -cuid=0 --cuda-device-only -S) the same kernels?  Compares function by function, so that
functions and constant tables emitted in another order do not count: the function ordinal in local labels is normalised, everything
else -- symbols, instructions, kernel descriptors, metadata entries -- must match.  Usage: compare_device_asm.py A.s B.s [...pairs]"""
import re, sys

def functions(path):
    text = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+", r".\1N", open(path).read())
    text = re.sub(r"[ \t]+;", " ;", text)      # (comments are aligned behind labels of different width)
    out, last = {}, "head"
    # a constant table (they follow the last function, in the order of their first use): one entry each
    def table(m): out["data:" + m.group(1)] = m.group(2); return ""
    text = re.sub(r"\t\.type\t(\S+),@object[^\n]*\n(?:\t\.section\t\.rodata[^\n]*\n)?(\t\.p2align[^\n]*\n\1:\n.*?\t\.size\t\1, \d+\n)", table, text, flags=re.S)
    # a function's text, its descriptor and its statistics: one section each (a function that is no template instantiation lies in plain
    # .text and is named by its "Begin function" line); metadata: one YAML item per kernel
    for chunk in re.split(r"\n(?=\t\.section\t|\t\.text\n|  - \.agpr_count:)", text):
        m = re.search(r"\.amdhsa_kernel (\S+)|\.section\t(\.text\.\S+?),|\.name:\s+(\S+)|^\t\.text\n.*; -- Begin function (\S+)", chunk)
        if m: last = key = m.group(1) and "desc:" + m.group(1) or m.group(2) or m.group(3) and "meta:" + m.group(3) or ".text." + m.group(4)
        else: key = "after:" + last + chunk.split(",")[0]      # (the sections that follow a function belong to it)
        out[key] = out.get(key, "") + chunk
    return out

bad = 0
for a, b in zip(sys.argv[1::2], sys.argv[2::2]):
    if open(a).read() == open(b).read(): print("identical   ", a); continue
    fa, fb = functions(a), functions(b)
    diff = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
    print("same kernels, other order" if not diff else "DIFFERENT   ", a, *diff[:5])
    bad += bool(diff)
sys.exit(1 if bad else 0)
