#!/usr/bin/env python3
"""Are two sets of device-assembly files (hipcc -cuid=0 --cuda-device-only -S) the same kernels?  Compares function by function, so that
functions and constant tables emitted in another order, or in another file of the set, do not count: the function ordinal in local labels is
normalised, everything else -- symbols, instructions, kernel descriptors, metadata entries -- must match.

Functions are keyed by their demangled names with the qualifier of the two band-LU namespaces (lu_fma:: / lu_nofma::) dropped, and every
symbol in the text is written that way too: a kernel that moved between translation units, or out of the namespaces, still meets itself.
Where several functions of a side share a key (the two roundings of one kernel) the key stands for the SET of their texts, and the sets
must be equal -- so a kernel compiled in both namespaces to the same instructions equals one that is compiled once.

Usage: compare_device_asm.py A.s B.s [...pairs]                       file by file
       compare_device_asm.py A1.s [A2.s ...] --against B1.s [B2.s ...]   one set against another
Prints every key that differs (-: only in A, +: only in B, !: in both, other text); exit status 1 if any does."""
import re, subprocess, sys

def demangled(text):
    """text with every mangled symbol replaced by its demangled name, spaces removed, lu_fma:: / lu_nofma:: dropped"""
    names = sorted(set(re.findall(r"\b_Z\w+", text)), key=len, reverse=True)
    if not names: return text
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    table = {n: re.sub(r"\blu_(no)?fma::", "", d).replace(" ", "") for n, d in zip(names, plain)}
    return re.sub(r"\b_Z\w+", lambda m: table[m.group(0)], text)

def functions(path):
    text = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+", r".\1N", open(path).read())
    text = re.sub(r"\bBB\d+_(\d+)", r"BBN_\1", text)      # (the same ordinal in the comments that name a loop's header block)
    text = re.sub(r"[ \t]+;", " ;", text)      # (comments are aligned behind labels of different width)
    text = demangled(text)
    out, last = {}, "head"
    # a constant table (they follow the last function, in the order of their first use): one entry each
    def table(m): out["data:" + m.group(1)] = m.group(2); return ""
    text = re.sub(r"\t\.type\t(\S+),@object[^\n]*\n(?:\t\.section\t\.rodata[^\n]*\n)?(\t\.p2align[^\n]*\n\1:\n.*?\t\.size\t\1, \d+\n)", table, text, flags=re.S)
    # what follows the last function (register maxima over the file's kernels, the compilation-unit id, section markers) and what closes
    # the metadata belong to the file, not to the kernel that happens to come last
    text = re.sub(r"\n((?:\t\.text\n\t\.p2alignl[^\n]*\n\t\.fill[^\n]*\n)?\t\.section\t\.AMDGPU\.gpr_maximums)", "\n\t.section\tfile trailer,\"\n\\1", text, count=1)
    text = text.replace("\n\t.amdgpu_metadata\n", "\n\t.section\tfile metadata,\"\n\t.amdgpu_metadata\n", 1)
    text = text.replace("\namdhsa.target:", "\n  - .agpr_count: file metadata end\namdhsa.target:")
    # a function's text, its descriptor and its statistics: one section each (a function that is no template instantiation lies in plain
    # .text and is named by its "Begin function" line); metadata: one YAML item per kernel
    for chunk in re.split(r"\n(?=\t\.section\t|\t\.text\n|  - \.agpr_count:)", text):
        m = re.search(r"\.amdhsa_kernel (\S+)|\.section\t(\.text\.\S+?),\"|\.name:\s+(\S+)|^\t\.text\n.*; -- Begin function (\S+)|(file [a-z ]+)", chunk)
        if m: last = key = m.group(1) and "desc:" + m.group(1) or m.group(2) or m.group(3) and "meta:" + m.group(3) or m.group(4) and ".text." + m.group(4) or "file:" + m.group(5)
        else: key = "after:" + last + chunk.split(",")[0]      # (the sections that follow a function belong to it)
        out[key] = out.get(key, "") + chunk
    return out

def side(paths):
    """key -> the set of texts the functions of that key have in the files of one side"""
    out = {}
    for path in paths:
        for key, chunk in functions(path).items(): out.setdefault(key, set()).add(chunk)
    return out

def compare(a, b):
    fa, fb = side(a), side(b)
    if len(a) + len(b) > 2: fa, fb = ({k: v for k, v in f.items() if "file:" not in k and k != "head"} for f in (fa, fb))      # sets of files: kernels only
    return ["-+!"[(k in fb) + (k in fa and k in fb)] + " " + k for k in sorted(set(fa) | set(fb)) if fa.get(k) != fb.get(k)]

if __name__ == "__main__":
    args, bad = sys.argv[1:], 0
    if "--against" in args:
        cut = args.index("--against")
        groups = [(args[:cut], args[cut + 1:])]
    else:
        groups = [([a], [b]) for a, b in zip(args[0::2], args[1::2])]
    for a, b in groups:
        if len(a) == len(b) == 1 and open(a[0]).read() == open(b[0]).read(): print("identical   ", a[0]); continue
        diff = compare(a, b)
        print("same kernels, other order or files" if not diff else "DIFFERENT   ", *a, "--against", *b)
        for d in diff: print("   ", d)
        bad += bool(diff)
    sys.exit(1 if bad else 0)
