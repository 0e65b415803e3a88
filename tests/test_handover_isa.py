"""Hand-over ordering in the built gfx950 code object (CPU only: disassembles the in-tree library).

A kernel that hands global data to another wave or workgroup inside ONE launch must drain its vector-memory stores
(s_waitcnt vmcnt(0)) before the barrier or the flag that publishes them: __syncthreads() is a workgroup-scope release, and on
gfx950 (outside threadgroup-split mode) it lowers to s_waitcnt lgkmcnt(0) + s_barrier, without vmcnt(0).  This file extracts
the gfx950 code object from the library's .hip_fatbin section, disassembles it, splits it per (demangled) kernel and checks
every site of SITES with one rule: on every path into the site, walking backwards, an s_waitcnt with vmcnt(0) comes before
any vector-memory write (store or atomic).  Each row also fixes how many sites every instantiation has, so a renamed kernel
or a change in code generation cannot make the check pass vacuously.  A new hand-over needs one row."""
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile

from gaussianvi_amd import _lib, build

TARGET = "gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
VMEM_WRITE = re.compile(r"^(global|buffer|flat|scratch)_(store|atomic)")
END = ("s_branch", "s_endpgm", "s_setpc_b64")             # no fall-through into the next instruction
CALL = ("s_swappc_b64", "s_setpc_b64")                    # unknown code: never credited with a wait


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError(f"{name} not found: ROCm's LLVM tools disassemble the code object")


class Kernel:
    def __init__(self, name):
        self.name, self.ins, self.labels = name, [], {}     # ins: (mnemonic, operands, address); labels: name -> index

    def preds(self, i):
        if not hasattr(self, "_from"):
            self._from = {}
            for j, (mn, op, _) in enumerate(self.ins):
                if mn.startswith(("s_branch", "s_cbranch")) and op in self.labels:
                    self._from.setdefault(self.labels[op], []).append(j)
        p = list(self._from.get(i, ()))
        if i > 0 and self.ins[i - 1][0] not in END:
            p.append(i - 1)
        return p

    def first_events(self, i, kind):
        """Walk every path into instruction i backwards; per path, the first instruction for which kind() is not None.
        Returns the set of (kind, index) met, with ("entry", -1) for a path that reaches the kernel's entry.
        Branch conditions are not tracked, so paths that cannot run are walked too: the check errs on the safe side, and a
        site it reports may be a false alarm.  (factor_block3_kernel: the s_endpgm after the trial-mean stores is reached
        through a flag-driven branch, so the walk also follows a path from those stores into the obstacle set's phase-1
        barrier -- a row on that barrier would fail for no real reason.)"""
        out, seen, todo = set(), set(), [i]
        while todo:
            j = todo.pop()
            if j == 0:
                out.add(("entry", -1))
            for p in self.preds(j):
                if p in seen:
                    continue
                seen.add(p)
                k = kind(self.ins[p])
                if k is None:
                    todo.append(p)
                else:
                    out.add((k, p))
        return out


def _is_wait0(ins):
    return ins[0] == "s_waitcnt" and re.search(r"\bvmcnt\(0\)", ins[1]) is not None


def _drain_kind(ins):
    if _is_wait0(ins):
        return "wait"
    if VMEM_WRITE.match(ins[0]) or ins[0] in CALL:
        return "write"
    return None


def drained(k, i):
    """The rule: no path into instruction i meets a vector-memory write (walking backwards) before a vmcnt(0) wait."""
    return all(e != "write" for e, _ in k.first_events(i, _drain_kind))


# ---- site selectors: kernel -> indices of the instructions the rule is applied to ----
def barrier_before_word(k):
    """The s_barrier in front of each 32-bit agent-scope store (the hand-over word; every data store there is 64-bit)."""
    out = []
    for i, (mn, op, _) in enumerate(k.ins):
        if mn == "global_store_dword" and re.search(r"\bsc1\b", op):
            j = i - 1
            while j >= 0 and k.ins[j][0] != "s_barrier":
                j -= 1
            assert j >= 0, f"{k.name}: no barrier in front of the word store at {k.ins[i][2]}"
            out.append(j)
    return sorted(set(out))


def _write_or_barrier(ins):
    if ins[0] == "s_barrier":
        return "barrier"
    if VMEM_WRITE.match(ins[0]):
        return "write"
    return None


def barrier_after_store(k):
    """Every s_barrier that some path reaches from a vector-memory write without another barrier in between."""
    return [i for i, ins in enumerate(k.ins)
            if ins[0] == "s_barrier" and any(e == "write" for e, _ in k.first_events(i, _write_or_barrier))]


def barrier_before_scalar_operands(k):
    """The s_barrier(s) that every 16-dword scalar load of psi operands is behind: barriers on every path from the kernel's
    entry to each such load (block3: H of the priors, written by the products phase of the same launch and read through
    the constant address space by sreg_body / sreg_pipe_body).  A load hoisted above its barrier drops the barrier from
    this set, and the row's count fails."""
    loads = [i for i, ins in enumerate(k.ins) if ins[0] == "s_load_dwordx16"]
    bars = [i for i, ins in enumerate(k.ins) if ins[0] == "s_barrier"]
    return [b for b in bars if loads and all(
        ("entry", -1) not in k.first_events(i, lambda x, b=b: None if x is not k.ins[b] else "barrier") for i in loads)]


def _first_write(ins):
    return "dx2sc1" if (ins[0] == "global_store_dwordx2" and re.search(r"\bsc1\b", ins[1])) else (
        "write" if VMEM_WRITE.match(ins[0]) else None)


def tail_arrival(k):
    """The arrival-counter atomics whose path back meets the agent-scope 64-bit store of the factor's cost first
    (epi_tail_arrive: its relaxed and its release / acquire form)."""
    return [i for i, (mn, _, _) in enumerate(k.ins)
            if mn.startswith("global_atomic_add") and any(e == "dx2sc1" for e, _ in k.first_events(i, _first_write))]


# One row per hand-over: what it is, the kernels (a regex on the demangled name; group 1 names the instantiation), the
# site selector, and the number of sites of every instantiation in the library.
SITES = [
    ("chain hand-over word (chain_signal)", r"gvi::chain_top_back_kernel<(\d+)>\(", barrier_before_word,
     {n: 2 for n in ("1", "2", "3", "4", "6", "8", "12", "16")}),
    ("sampling sweep, y in global memory", r"gvi::sample_sweep_kernel<(\d+), false>\(", barrier_after_store,
     {"4": 2, "8": 2, "16": 2}),
    ("factor-pass cost tail (epi_tail_arrive)",
     r"gvi::(epilogue_all_kernel|factor_block3_kernel|factor_fused_kernel<[\d, ]+>)\(", tail_arrival,
     {"epilogue_all_kernel": 2, "factor_block3_kernel": 6, "factor_fused_kernel<6, 4, 4, 12, 6>": 4,
      "factor_fused_kernel<6, 6, 2, 12, 6>": 4, "factor_fused_kernel<2, 4, 4, 4, 2>": 4}),
    ("block3 products -> scalar H loads (block_products_drain)", r"gvi::(factor_block3_kernel)\(",
     barrier_before_scalar_operands, {"factor_block3_kernel": 1}),
]


@functools.lru_cache(maxsize=None)
def kernels():
    lib = _lib.LIB_PATH                            # read as it is: this test only disassembles (conftest builds it if absent)
    assert os.path.exists(lib), f"{lib} is missing"
    if os.path.realpath(lib) == os.path.realpath(build.LIB):
        assert not build._stale(lib, build.lib_sources()), f"{lib} is older than its sources: rebuild it first"
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "copy.so")],
                       check=True, capture_output=True)
        with open(fat, "rb") as f:
            data = f.read()
        objs = []
        pos = data.find(BUNDLE_MAGIC)
        while pos >= 0:                            # one bundle per translation unit with device code
            (count,) = struct.unpack_from("<Q", data, pos + 24)
            off, end = pos + 32, pos + 32
            for _ in range(count):
                eoff, esize, tlen = struct.unpack_from("<QQQ", data, off)
                triple = data[off + 24:off + 24 + tlen].decode()
                off += 24 + tlen
                end = max(end, pos + eoff + esize)
                if esize and triple.split("-")[-1].split(":")[0] == TARGET:
                    objs.append(data[pos + eoff:pos + eoff + esize])
            pos = data.find(BUNDLE_MAGIC, end)
        assert objs, f"no {TARGET} code object in {lib}"
        text = []
        for n, blob in enumerate(objs):
            co = os.path.join(tmp, f"co{n}.o")
            with open(co, "wb") as f:
                f.write(blob)
            r = subprocess.run([_tool("llvm-objdump"), "-d", "-C", f"--mcpu={TARGET}", "--symbolize-operands", co],
                               check=True, capture_output=True, text=True)
            text.extend(r.stdout.splitlines())
    out, cur = {}, None
    for line in text:
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            if re.fullmatch(r"L\d+", m.group(2)):
                cur.labels[m.group(2)] = len(cur.ins)
            else:
                cur = out[m.group(2)] = Kernel(m.group(2))
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]*)\s*(.*?)\s*//\s*([0-9A-F]+):", line)
        if m and cur is not None:
            cur.ins.append((m.group(1), m.group(2), m.group(3)))
    return out


def test_the_code_object_is_found_and_split_per_kernel():
    ks = kernels()
    assert len(ks) > 50
    k = next(v for name, v in ks.items() if "chain_top_back_kernel<6>" in name)
    assert any(mn == "s_barrier" for mn, _, _ in k.ins) and k.labels


def test_every_hand_over_waits_for_its_writes_before_publishing():
    ks = kernels()
    problems = []
    for what, pattern, select, expect in SITES:
        found = {}
        for name, k in ks.items():
            m = re.search(pattern, name)
            if m:
                found[m.group(1)] = (k, select(k))
        assert set(found) == set(expect), f"{what}: instantiations {sorted(found)}, expected {sorted(expect)}"
        for inst, (k, sites) in sorted(found.items()):
            assert len(sites) == expect[inst], f"{what}: {inst} has {len(sites)} sites, expected {expect[inst]}"
            bad = [k.ins[i][2] for i in sites if not drained(k, i)]
            if bad:
                problems.append(f"{what}: {inst} at {', '.join('0x' + b.lstrip('0') for b in bad)}")
    assert not problems, "no s_waitcnt vmcnt(0) on some path in front of:\n  " + "\n  ".join(problems)


def _tiny(lines):
    k = Kernel("t")
    for ln in lines:
        if ln.endswith(":"):
            k.labels[ln[:-1]] = len(k.ins)
        else:
            mn, _, op = ln.partition(" ")
            k.ins.append((mn, op, format(len(k.ins), "X")))
    return k


def test_the_rule_follows_every_path_into_the_site():
    """The checker itself: a wait on one branch does not cover the other; a write behind the wait is caught."""
    ok = _tiny(["global_store_dwordx2 v[0:1], v[2:3], off sc1", "s_waitcnt vmcnt(0)", "s_cbranch_scc1 L1",
                "v_mov_b32 v0, 0", "L1:", "s_barrier"])
    assert drained(ok, 4)
    one_side = _tiny(["global_store_dwordx2 v[0:1], v[2:3], off", "s_cbranch_scc1 L1", "s_waitcnt vmcnt(0)", "L1:",
                      "s_barrier"])
    assert not drained(one_side, 3)
    late = _tiny(["s_waitcnt vmcnt(0)", "global_store_dwordx2 v[0:1], v[2:3], off", "s_waitcnt lgkmcnt(0)", "s_barrier"])
    assert not drained(late, 3)
    loop = _tiny(["L0:", "s_waitcnt vmcnt(0)", "s_barrier", "global_store_dword v0, v1, off", "s_cbranch_scc1 L0",
                  "s_endpgm"])
    assert drained(loop, 1) and barrier_before_word(loop) == []
