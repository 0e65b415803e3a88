"""The walk's priority bands in the built gfx950 code object (CPU only; the code object is found and disassembled the way
test_handover_isa.py and test_orbit_walk_isa.py do it).

orbit_wave sets a walking wave's priority from the share of its modelled walk cost still ahead of it (walk_prio.hpp), behind
a compile-time switch that factor_fused_kernel alone turns on.  s_setprio takes an immediate and ignores EXEC, so the bands
must be four constant instructions behind scalar branches: each fused instance holds s_setprio with every immediate 0 .. 3,
and each of them is reached through a scalar conditional branch (a band test compiled as a lane mask would leave the
instructions unconditional, one behind the other).  The stand-alone walk kernels run several residency rounds and hold none.
Registers: no fused instance needs more vector registers or scratch than at the parent commit fcbf162 (figures read from a
build of it, by the same reader)."""
import collections

import pytest

import test_handover_isa as isa
import test_orbit_walk_isa as walk

# (VGPRs, scratch bytes per lane) at fcbf162
PARENT = {"factor_fused_kernel<6, 4, 4, 12, 6>": (128, 12), "factor_fused_kernel<6, 6, 2, 12, 6>": (166, 0),
          "factor_fused_kernel<2, 4, 4, 4, 2>": (128, 20)}


def _family(prefix):
    found = {name: k for name, k in isa.kernels().items() if name.startswith("gvi::" + prefix) or name.startswith("void gvi::" + prefix)}
    assert found, prefix
    return found


def _immediates(k):
    return collections.Counter(int(op, 0) for mn, op, _ in k.ins if mn == "s_setprio")


def test_every_fused_instance_sets_all_four_priorities():
    fused = _family("factor_fused_kernel<")
    assert len(fused) == 3, sorted(fused)
    for name, k in sorted(fused.items()):
        imm = _immediates(k)
        print(f"{name.split('(')[0]}: s_setprio immediates {dict(sorted(imm.items()))}")
        assert set(imm) == {0, 1, 2, 3}, (name, imm)


def test_the_raised_priorities_sit_behind_scalar_branches():
    """Walking back from every s_setprio 1 / 2 / 3 over straight-line code, a scalar conditional branch (or the label such a
    branch jumps to) comes before any other s_setprio: no band's instruction runs unconditionally behind another's."""
    for name, k in sorted(_family("factor_fused_kernel<").items()):
        targets = set(k.labels.values())
        for i, (mn, op, _) in enumerate(k.ins):
            if mn != "s_setprio" or int(op, 0) == 0:
                continue
            j, guarded = i, False
            while j > 0 and not guarded:
                if j in targets and j != i:
                    guarded = True                 # reached by a jump: the branch is elsewhere
                    break
                j -= 1
                if k.ins[j][0].startswith("s_cbranch"):
                    guarded = True
                elif k.ins[j][0] == "s_setprio":
                    break
            assert guarded or i in targets, (name, k.ins[i][2])


def test_the_stand_alone_walk_kernels_set_no_priority():
    alone = {**_family("moments_orbit_pair_kernel<"), **_family("moments_orbit_kernel<")}
    assert len(alone) >= 30, len(alone)
    for name, k in alone.items():
        assert not _immediates(k), name


@pytest.mark.parametrize("name", sorted(PARENT))
def test_no_more_registers_or_scratch_than_the_parent(name):
    vgpr, scratch = walk.resources()[name]
    print(f"{name}: VGPRs {vgpr} (parent {PARENT[name][0]}), scratch {scratch} bytes per lane (parent {PARENT[name][1]})")
    assert vgpr <= PARENT[name][0] and scratch <= PARENT[name][1]
