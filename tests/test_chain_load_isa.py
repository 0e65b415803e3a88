"""The first chain pass issues its assemble-on-load as one batch of loads (CPU only: disassembles the in-tree library the
way test_handover_isa.py does).

kernels_chain.hpp, forward_body, dense path (ChainArgs::asm_on == ASM_DENSE): one binary factor set (d = 2n) and one unary
set (d = n).  A thread of the load phase handles two elements (r, c) per round, and per element it needs

    binary set   Vddmu[t][r][c], Vddmu[t-1][n+r][n+c]  (V_D: own factor, left neighbour's)  and  Vddmu[t][r][n+c]  (V_U)   3
    unary set    Vddmu[t][r][c]                                                                                           1
    factorisation body only: the chain's own D[t][r][c] and U[t][r][c] (the matrix the assembled one is mixed into)       2

so a factorisation thread needs B_FACT = 2 x (3 + 1 + 2) = 12 loads in one round.  The solve operates ON the assembled
matrix (no D, no U), and its round also carries the thread's entry of the right-hand side, g[t][r] = binary set's
Vdmu[t][r] + Vdmu[t-1][n+r] + unary set's Vdmu[t][r]: B_SOLVE = 2 x (3 + 1) + 3 = 11.  None of these loads depends on
another, so all of a round's loads must be in flight together: in the code of every chain_forward_kernel<N, false> there must
be a run of at least B_FACT vector loads with no s_waitcnt on vmcnt and no branch between them, and a second, disjoint run of
at least B_SOLVE.  Before the batched path the longest run was 2 (N = 6: 1 -- forty load sites, each behind its own branch and
wait).

The batch must not cost registers where there are none: no instantiation's private segment (scratch) may be larger than it
was before the batched path (PARENT_SCRATCH, bytes per lane, read from the code object's metadata)."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

import test_handover_isa as isa

B_FACT = 2 * (3 + 1 + 2)
B_SOLVE = 2 * (3 + 1) + 3
SIZES = (1, 2, 3, 4, 6, 8, 12, 16)

VMEM_LOAD = re.compile(r"^(global|buffer|flat)_load_")
BRANCH = ("s_branch", "s_cbranch", "s_setpc_b64", "s_swappc_b64", "s_endpgm")

# .private_segment_fixed_size of the chain kernels before this path existed
PARENT_SCRATCH = {}
for _n in SIZES:
    PARENT_SCRATCH[f"chain_forward_kernel<{_n}, false>"] = 0
    PARENT_SCRATCH[f"chain_forward_kernel<{_n}, true>"] = 0
    PARENT_SCRATCH[f"chain_top_back_kernel<{_n}>"] = 0
    PARENT_SCRATCH[f"chain_backward_kernel<{_n}>"] = 0
PARENT_SCRATCH["chain_top_back_kernel<6>"] = 40
PARENT_SCRATCH["chain_forward_kernel<6, true>"] = 16


def load_runs(k, first_barrier_only=False):
    """Lengths of the runs of vector loads in the kernel's code, longest first; a wait on vmcnt or a branch ends a run (a
    label does not: only a branch, which is an instruction, leaves the straight line).  first_barrier_only: the code in
    front of the first s_barrier in code order -- the load phase of whichever of the two bodies (factorisation, solve) the
    compiler laid out first."""
    runs, cur = [], 0
    for mn, op, _ in k.ins:
        if mn == "s_barrier" and first_barrier_only:
            break
        if VMEM_LOAD.match(mn):
            cur += 1
        elif (mn == "s_waitcnt" and "vmcnt" in op) or mn.startswith(BRANCH):
            runs.append(cur)
            cur = 0
    runs.append(cur)
    return sorted((r for r in runs if r), reverse=True)


def test_the_run_rule():
    """The checker itself: a wait on vmcnt or a branch ends a run; other waits and arithmetic do not."""
    def k(lines):
        return load_runs(isa._tiny(lines))
    ld = "global_load_dwordx2 v[0:1], v[2:3], off"
    assert k([ld, ld, ld, "s_waitcnt vmcnt(3)", ld, "s_waitcnt vmcnt(0)"]) == [3, 1]
    assert k([ld, ld, "s_cbranch_execz L1", ld, "L1:", ld]) == [2, 2]
    assert k([ld, "s_waitcnt lgkmcnt(0)", ld, "v_add_f64 v[0:1], v[0:1], 0", ld]) == [3]


def _kernel(pattern):
    found = [k for name, k in isa.kernels().items() if pattern in name]
    assert len(found) == 1, f"{pattern}: {len(found)} kernels"
    return found[0]


@pytest.mark.parametrize("n", SIZES)
def test_the_first_pass_issues_a_rounds_loads_in_one_batch(n):
    """chain_forward_kernel<N, false> holds both bodies, each with its own load phase and barrier: in front of the first
    barrier in code order there is the batch of the body laid out first (at least B_SOLVE, the smaller of the two), and over
    the whole kernel the two longest runs are the two batches.  (Behind its load phase a segmented pass reads no global
    memory, so no other part of the kernel can supply such a run.)"""
    k = _kernel(f"gvi::chain_forward_kernel<{n}, false>(")
    assert any(mn == "s_barrier" for mn, _, _ in k.ins)
    head, runs = load_runs(k, True), load_runs(k)
    print(f"chain_forward_kernel<{n}, false>: runs of vector loads before the first barrier {head[:4]}, in the kernel {runs[:4]}")
    assert head and head[0] >= B_SOLVE, head
    assert len(runs) >= 2 and runs[0] >= B_FACT and runs[1] >= B_SOLVE, runs


@pytest.mark.parametrize("n", SIZES)
def test_the_one_launch_and_merged_top_passes_use_the_same_batch(n):
    """The same load phase in the TOP instance (chains that fit one launch) and in the top body of chain_top_back_kernel."""
    for pattern in (f"gvi::chain_forward_kernel<{n}, true>(", f"gvi::chain_top_back_kernel<{n}>("):
        runs = load_runs(_kernel(pattern))
        print(f"{pattern} runs of vector loads {runs[:4]}")
        assert len(runs) >= 2 and runs[0] >= B_FACT and runs[1] >= B_SOLVE, (pattern, runs)


MANGLED = re.compile(r"_ZN3gvi(?:20chain_forward_kernelILi(\d+)ELb([01])EEE|21chain_top_back_kernelILi(\d+)EEE|"
                     r"21chain_backward_kernelILi(\d+)EEE)v")


def _chain_scratch():
    """kernel -> .private_segment_fixed_size from the metadata note of the gfx950 code objects (within a kernel's map the
    keys are sorted, so .name comes before .private_segment_fixed_size)"""
    lib = isa._lib.LIB_PATH
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([isa._tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "copy.so")],
                       check=True, capture_output=True)
        with open(fat, "rb") as f:
            data = f.read()
        pos, nco = data.find(isa.BUNDLE_MAGIC), 0
        while pos >= 0:
            (count,) = struct.unpack_from("<Q", data, pos + 24)
            off, end = pos + 32, pos + 32
            for _ in range(count):
                eoff, esize, tlen = struct.unpack_from("<QQQ", data, off)
                triple = data[off + 24:off + 24 + tlen].decode()
                off += 24 + tlen
                end = max(end, pos + eoff + esize)
                if esize and triple.split("-")[-1].split(":")[0] == isa.TARGET:
                    co = os.path.join(tmp, f"co{nco}.o")
                    nco += 1
                    with open(co, "wb") as f:
                        f.write(data[pos + eoff:pos + eoff + esize])
                    r = subprocess.run([isa._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True)
                    name = None
                    for line in r.stdout.splitlines():
                        m = re.match(r"[\s-]*\.name:\s+(\S+)", line)
                        if m:
                            name = m.group(1)
                        m = re.match(r"[\s-]*\.private_segment_fixed_size:\s+(\d+)", line)
                        if m and name:
                            g = MANGLED.match(name)
                            if g:
                                if g.group(1):
                                    key = f"chain_forward_kernel<{g.group(1)}, {'true' if g.group(2) == '1' else 'false'}>"
                                elif g.group(3):
                                    key = f"chain_top_back_kernel<{g.group(3)}>"
                                else:
                                    key = f"chain_backward_kernel<{g.group(4)}>"
                                out[key] = int(m.group(1))
            pos = data.find(isa.BUNDLE_MAGIC, end)
    return out


def test_no_chain_kernel_gained_scratch():
    now = _chain_scratch()
    for key in sorted(now):
        print(f"{key}: scratch {now[key]} bytes per lane (before: {PARENT_SCRATCH.get(key)})")
    assert set(now) == set(PARENT_SCRATCH), sorted(set(PARENT_SCRATCH) ^ set(now))
    grew = [f"{key}: {PARENT_SCRATCH[key]} -> {now[key]}" for key in sorted(now) if now[key] > PARENT_SCRATCH[key]]
    assert not grew, grew
