"""The row-broadcast eliminations are in the built gfx950 code object where they belong (CPU only: disassembles the in-tree
library the way test_handover_isa.py does).

The N = 6 instantiations of the three kernels that run forward eliminations -- chain_forward_kernel<6, false|true> and
chain_top_back_kernel<6>, the ones test_chain_load_isa.py and test_handover_isa.py look at -- hold the two-row form: they must
contain the DPP row broadcast (row_newbcast) in all three shapes the Gauss-Jordan uses (v_mov_b64_dpp for the pivot,
v_fmac_f64_dpp for the update, v_mov_b32_dpp for the row choice of the pivoted solve) and fewer v_readlane_b32 than the
v_readlane form of the same bodies.  Every other block size, and the backward kernel, must contain none.

Wait states: inline asm gets none from the compiler, and a vector write of a register needs two before a DPP read of it.  For
every row_newbcast instruction of the library, no vector instruction within the two wait states in front of it may write a
register it reads through DPP.

The v_readlane form of the N = 6 bodies (option chain_pair 0, and passes without a crowded level) lives in kernels of its own,
chain_forward_readlane_kernel<false|true> and chain_top_back_readlane_kernel, which the two yardstick files do not match by
name.  Their rules are applied to them here: no DPP broadcast, no more scratch than the parent's N = 6 kernels had
(test_chain_load_isa.PARENT_SCRATCH), the two load batches of the first pass, and the drained hand-over."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

import test_chain_load_isa as loads
import test_handover_isa as isa

SIZES = ("1", "2", "3", "4", "6", "8", "12", "16")
PLAIN = re.compile(r"gvi::(chain_forward_kernel<(\d+), (?:false|true)>|chain_top_back_kernel<(\d+)>|chain_backward_kernel<(\d+)>)\(")
# v_readlane kernel -> the kernel whose N = 6 bodies it holds in the other form
READLANE = {"gvi::chain_forward_readlane_kernel<false>(": "chain_forward_kernel<6, false>",
            "gvi::chain_forward_readlane_kernel<true>(": "chain_forward_kernel<6, true>",
            "gvi::chain_top_back_readlane_kernel(": "chain_top_back_kernel<6>"}
N_STEPS = 6                                   # Gauss-Jordan steps of an N = 6 elimination
DPP_WAIT_STATES = 2                           # vector write of a register -> DPP read of it


def _dpp(k):
    """mnemonic -> number of instructions of the kernel with a row_newbcast control"""
    out = {}
    for mn, op, _ in k.ins:
        if "row_newbcast" in op:
            out[mn] = out.get(mn, 0) + 1
    return out


def _one(pattern):
    found = [k for name, k in isa.kernels().items() if pattern in name]
    assert len(found) == 1, f"{pattern}: {len(found)} kernels"
    return found[0]


def _readlanes(k):
    return sum(1 for mn, _, _ in k.ins if mn == "v_readlane_b32")


def test_the_n6_forward_kernels_hold_the_row_broadcast_form():
    for pattern, plain in sorted(READLANE.items()):
        k, kr = _one(f"gvi::{plain}("), _one(pattern)
        d = _dpp(k)
        print(f"{plain}: row_newbcast operations {d}, v_readlane_b32 {_readlanes(k)} (the v_readlane form: {_readlanes(kr)})")
        # per elimination site and body (factorisation, solve): one pivot move per step and N - 1 updates per step; the solve
        # broadcasts its row choice in every step that has a choice (the last one has none)
        assert d.get("v_mov_b64_dpp", 0) >= 2 * N_STEPS, (plain, d)
        assert d.get("v_fmac_f64_dpp", 0) >= 2 * N_STEPS * (N_STEPS - 1), (plain, d)
        assert d.get("v_mov_b32_dpp", 0) >= N_STEPS - 1, (plain, d)
        assert _readlanes(k) < _readlanes(kr), (plain, _readlanes(k), _readlanes(kr))


def test_the_other_kernels_hold_none():
    seen = []
    for name, k in sorted(isa.kernels().items()):
        m = PLAIN.search(name)
        if m:
            n = m.group(2) or m.group(3) or m.group(4)
            seen.append(n)
            if n != "6" or "chain_backward_kernel" in name:
                assert _dpp(k) == {}, (name, _dpp(k))
    assert sorted(seen) == sorted(SIZES * 4), sorted(seen)
    for pattern in READLANE:
        assert _dpp(_one(pattern)) == {}, pattern


# ---- wait states in front of the DPP reads ----
def _regs(operand):
    """vector registers an operand names: 'v3' -> {3}, 'v[4:5]' -> {4, 5}, anything else -> {}"""
    m = re.fullmatch(r"-?\|?v(\d+)\|?", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"-?\|?v\[(\d+):(\d+)\]\|?", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def _operands(op):
    return [o.strip() for o in re.split(r",\s*(?![^\[]*\])", op.split(" row_newbcast")[0]) if o.strip()]


def dpp_hazards(k):
    """(address of the DPP instruction, address of the writer) for every row_newbcast instruction with a vector write of its
    DPP-read operand (src0: the second operand) fewer than DPP_WAIT_STATES wait states in front of it, in code order.  An
    instruction is one wait state, s_nop N is N + 1.  (Code order across a label is the fall-through path; a branch target is
    reached behind the branch instruction and whatever preceded it, which is never closer.)"""
    out = []
    for i, (mn, op, addr) in enumerate(k.ins):
        if "row_newbcast" not in op:
            continue
        src = _regs(_operands(op)[1])
        assert src, (mn, op)
        states, j = 0, i - 1
        while j >= 0 and states < DPP_WAIT_STATES:
            pmn, pop, paddr = k.ins[j]
            if pmn == "s_nop":
                states += int(pop, 0) + 1
            else:
                if pmn.startswith("v_") and _operands(pop) and _regs(_operands(pop)[0]) & src:
                    out.append((addr, paddr))
                states += 1
            j -= 1
    return out


def test_the_hazard_checker_itself():
    mov = "v_mov_b64_dpp v[8:9], v[2:3] row_newbcast:1 row_mask:0xf bank_mask:0xf"
    fmac = "v_fmac_f64_dpp v[4:5], v[4:5], v[6:7] row_newbcast:0 row_mask:0xf bank_mask:0xf"
    assert dpp_hazards(isa._tiny(["v_add_f64 v[2:3], v[0:1], v[0:1]", mov])) == [("1", "0")]
    assert dpp_hazards(isa._tiny(["v_add_f64 v[2:3], v[0:1], v[0:1]", "s_nop 0", mov])) == [("2", "0")]
    assert dpp_hazards(isa._tiny(["v_add_f64 v[2:3], v[0:1], v[0:1]", "s_nop 1", mov])) == []
    assert dpp_hazards(isa._tiny(["v_add_f64 v[2:3], v[0:1], v[0:1]", "v_mov_b32 v9, v1", "v_mov_b32 v10, v1", mov])) == []
    assert dpp_hazards(isa._tiny(["v_mov_b32 v5, v1", "v_mov_b32 v10, v1", fmac])) == [("2", "0")]
    assert dpp_hazards(isa._tiny(["v_mul_f64 v[6:7], v[0:1], v[0:1]", fmac])) == []          # (the plain operand: no hazard)
    assert dpp_hazards(isa._tiny([fmac, fmac.replace("row_newbcast:0", "row_newbcast:1")])) == [("1", "0")]


def test_no_vector_write_within_two_wait_states_of_its_dpp_read():
    n = 0
    for name, k in sorted(isa.kernels().items()):
        if not _dpp(k):
            continue
        n += 1
        bad = dpp_hazards(k)
        assert not bad, f"{name}: DPP read at / writer at {bad[:8]}"
    assert n >= 3


# ---- the yardsticks' rules on the v_readlane kernels ----
def _scratch_of(mangled_part):
    """.private_segment_fixed_size of the kernels whose mangled name contains mangled_part (metadata note, as in
    test_chain_load_isa._chain_scratch)"""
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
                        if m and name and mangled_part in name:
                            out[name] = int(m.group(1))
            pos = data.find(isa.BUNDLE_MAGIC, end)
    return out


def test_the_readlane_kernels_have_no_more_scratch_than_the_parent():
    now = {}
    now.update(_scratch_of("chain_forward_readlane_kernel"))
    now.update(_scratch_of("chain_top_back_readlane_kernel"))
    assert len(now) == 3, sorted(now)
    for name, size in sorted(now.items()):
        if "top_back" in name:
            key = "chain_top_back_kernel<6>"
        else:
            key = f"chain_forward_kernel<6, {'true' if 'ILb1E' in name else 'false'}>"
        print(f"{name}: scratch {size} bytes per lane (parent's {key}: {loads.PARENT_SCRATCH[key]})")
        assert size <= loads.PARENT_SCRATCH[key], (name, size)


@pytest.mark.parametrize("pattern", sorted(READLANE))
def test_the_readlane_kernels_issue_a_rounds_loads_in_one_batch(pattern):
    runs = loads.load_runs(_one(pattern))
    print(f"{pattern} runs of vector loads {runs[:4]}")
    assert len(runs) >= 2 and runs[0] >= loads.B_FACT and runs[1] >= loads.B_SOLVE, runs


def test_the_merged_readlane_kernel_drains_its_stores_before_the_hand_over_word():
    k = _one("gvi::chain_top_back_readlane_kernel(")
    sites = isa.barrier_before_word(k)
    assert len(sites) == 2, sites
    bad = [k.ins[i][2] for i in sites if not isa.drained(k, i)]
    assert not bad, bad
