#!/usr/bin/env python3
"""Instruction classes of the chain kernels, per barrier-to-barrier segment, from compiler assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++20 --cuda-device-only -S -I include gaussianvi_amd/csrc/gvi_hip.hip -o new.s
    tools/chain_isa_classes.py parent.s new.s [--kernel SUBSTRING ...]

Each named kernel (substring of the mangled symbol; default: the N = 6 chain kernels) is cut at its s_barrier instructions in
code order, and per segment the instructions are counted by mnemonic prefix:

    fp64    v_*_f64 (also in DPP / SDWA form)
    valu    every other v_* but the lane moves
    lane    v_readlane_b32, v_writelane_b32, v_readfirstlane_b32
    salu    s_* that is none of: wait, scalar load, barrier, end of program
    ds      ds_*
    vmem    global_*, buffer_*, flat_*, scratch_*
    smem    s_load_*, s_buffer_load_*
    wait    s_waitcnt*, s_nop, s_sleep

The counts are STATIC: code order, not execution order, and a loop body counts once.  With two files the segments are printed
side by side (parent, new, difference); a segment keeps its position only as long as the compiler lays the bodies out in the
same order, so the rcp / ds_add columns (v_rcp_f64 and ds_add_f64 alone: 6 reciprocals per Gauss-Jordan, the accumulator adds of
an elimination) are printed to recognise a body by.  The tool counts mnemonics and looks for nothing else."""
import argparse
import re
import sys

DEFAULT = ("chain_forward_kernelILi6ELb0E", "chain_forward_kernelILi6ELb1E", "chain_top_back_kernelILi6E",
           "chain_forward_readlane_kernelILb0E", "chain_forward_readlane_kernelILb1E", "chain_top_back_readlane_kernel",
           "chain_backward_kernelILi6E")
CLASSES = ("fp64", "valu", "lane", "salu", "ds", "vmem", "smem", "wait")
LANE = ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32")
MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(mn):
    if mn in ("s_barrier", "s_endpgm", "s_code_end"):
        return None
    if mn.startswith(LANE):
        return "lane"
    if mn.startswith("v_"):
        return "fp64" if re.search(r"_f64(_|$)", mn) else "valu"
    if mn.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if mn.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "ds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return None


def kernels(path):
    """symbol -> list of mnemonics between the symbol's label and its .Lfunc_end"""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur is None:
                continue
            m = MNEMONIC.match(line)
            if m and not line.lstrip().startswith((".", ";")):
                cur.append(m.group(1))
    return out


def segments(ins):
    segs, cur = [], dict.fromkeys(CLASSES + ("rcp", "ds_add", "writelane"), 0)
    for mn in ins:
        if mn == "s_barrier":
            segs.append(cur)
            cur = dict.fromkeys(CLASSES + ("rcp", "ds_add", "writelane"), 0)
            continue
        c = classify(mn)
        if c:
            cur[c] += 1
        cur["rcp"] += mn.startswith("v_rcp_f64")
        cur["ds_add"] += mn.startswith("ds_add_f64")
        cur["writelane"] += mn.startswith("v_writelane_b32")
    segs.append(cur)
    return segs


def find(ks, sub):
    hit = [k for k in ks if sub in k]
    return hit[0] if len(hit) == 1 else None


def row(s):
    return " ".join(f"{s[c]:5d}" for c in CLASSES) + f" | {s['rcp']:3d} {s['ds_add']:4d} {s['writelane']:4d}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", nargs="+", help="one or two assembly files (parent, new)")
    ap.add_argument("--kernel", action="append", help="substring of a mangled kernel symbol (repeatable)")
    a = ap.parse_args()
    if len(a.asm) > 2:
        ap.error("one or two assembly files")
    files = [kernels(p) for p in a.asm]
    head = " ".join(f"{c:>5s}" for c in CLASSES) + " | rcp dadd wlan"
    for sub in a.kernel or DEFAULT:
        names = [find(ks, sub) for ks in files]
        if not all(names):
            print(f"== {sub}: not found exactly once in every file ==")
            continue
        segs = [segments(ks[n]) for ks, n in zip(files, names)]
        print(f"== {sub} ({' / '.join(str(len(s)) for s in segs)} segments) ==")
        print(f"{'seg':>4s} {'':6s} {head}    valu+lane")
        for i in range(max(len(s) for s in segs)):
            for tag, s in zip(("parent", "new") if len(segs) == 2 else ("",), segs):
                if i < len(s):
                    print(f"{i:4d} {tag:6s} {row(s[i])}    {s[i]['valu'] + s[i]['lane']:5d}")
        for tag, s in zip(("parent", "new") if len(segs) == 2 else ("",), segs):
            tot = {c: sum(x[c] for x in s) for c in s[0]}
            print(f" all {tag:6s} {row(tot)}    {tot['valu'] + tot['lane']:5d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
