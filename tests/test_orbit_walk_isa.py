"""Registers and scratch of every kernel that holds the sign-orbit walk (kernels_orbit.hpp), read from the built gfx950 code
object (CPU only: the kernel descriptors' metadata of the in-tree library, found the way test_handover_isa.py finds the code).

The walk evaluates the even scalar of psi only -- the odd one, its Walsh butterfly and its sums left with the closed form of
m1 (orbit_wave) -- so no instance may need more vector registers or more scratch per lane than it did with them.  PARENT: the
figures of commit 86298f3 (the last one whose walk carried the odd scalar), from its -Rpass-analysis=kernel-resource-usage
remarks and its code object's metadata alike.  The fused pass additionally stays at four blocks per CU: <= 128 registers in
the instances built for four waves per SIMD."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

import test_handover_isa as isa
from gaussianvi_amd import _lib, build

# (VGPRs, scratch bytes per lane) at 86298f3
PARENT = {
    "factor_fused_kernel<6, 4, 4, 12, 6>": (128, 12), "factor_fused_kernel<6, 6, 2, 12, 6>": (182, 0), "factor_fused_kernel<2, 4, 4, 4, 2>": (128, 20),
    "moments_orbit_pair_kernel<2, 4, true, false, 4>": (98, 0), "moments_orbit_pair_kernel<2, 4, false, false, 4>": (44, 0),
    "moments_orbit_pair_kernel<6, 4, true, false, 4>": (128, 8), "moments_orbit_pair_kernel<6, 4, false, false, 4>": (70, 0),
    "moments_orbit_pair_kernel<6, 6, true, false, 2>": (192, 0), "moments_orbit_pair_kernel<6, 6, false, false, 2>": (75, 0),
    "moments_orbit_pair_kernel<12, 4, true, false, 3>": (168, 40), "moments_orbit_pair_kernel<12, 4, false, false, 3>": (122, 0),
    "moments_orbit_pair_kernel<12, 6, true, false, 2>": (236, 0), "moments_orbit_pair_kernel<12, 6, false, false, 2>": (118, 0),
    "moments_orbit_kernel<2, 4, true, false, 4>": (94, 0), "moments_orbit_kernel<2, 4, true, true, 4>": (98, 0),
    "moments_orbit_kernel<2, 4, false, false, 4>": (44, 0), "moments_orbit_kernel<2, 4, false, true, 4>": (44, 0),
    "moments_orbit_kernel<14, 4, true, false, 2>": (150, 0), "moments_orbit_kernel<14, 4, true, true, 2>": (166, 0),
    "moments_orbit_kernel<14, 4, false, false, 2>": (100, 0), "moments_orbit_kernel<14, 4, false, true, 2>": (88, 0),
    "moments_orbit_kernel<6, 4, true, false, 4>": (118, 0), "moments_orbit_kernel<6, 4, true, true, 4>": (128, 8),
    "moments_orbit_kernel<6, 4, false, false, 4>": (68, 0), "moments_orbit_kernel<6, 4, false, true, 4>": (72, 0),
    "moments_orbit_kernel<6, 6, true, false, 2>": (172, 0), "moments_orbit_kernel<6, 6, true, true, 2>": (194, 0),
    "moments_orbit_kernel<6, 6, false, false, 2>": (74, 0), "moments_orbit_kernel<6, 6, false, true, 2>": (74, 0),
    "moments_orbit_kernel<12, 4, true, false, 3>": (154, 0), "moments_orbit_kernel<12, 4, true, true, 3>": (168, 100),
    "moments_orbit_kernel<12, 4, false, false, 3>": (120, 0), "moments_orbit_kernel<12, 4, false, true, 3>": (108, 0),
    "moments_orbit_kernel<12, 6, true, false, 2>": (226, 0), "moments_orbit_kernel<12, 6, true, true, 2>": (209, 0),
    "moments_orbit_kernel<12, 6, false, false, 2>": (116, 0), "moments_orbit_kernel<12, 6, false, true, 2>": (110, 0),
}
FAMILIES = ("factor_fused_kernel<", "moments_orbit_pair_kernel<", "moments_orbit_kernel<")
FOUR_BLOCKS = ("factor_fused_kernel<6, 4, 4, 12, 6>", "factor_fused_kernel<2, 4, 4, 4, 2>")


def resources():
    """{kernel name without namespace and arguments: (VGPRs, scratch bytes per lane)} of the library's gfx950 code objects"""
    lib = _lib.LIB_PATH
    assert os.path.exists(lib), f"{lib} is missing"
    if os.path.realpath(lib) == os.path.realpath(build.LIB):
        assert not build._stale(lib, build.lib_sources()), f"{lib} is older than its sources: rebuild it first"
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([isa._tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "copy.so")],
                       check=True, capture_output=True)
        with open(fat, "rb") as f:
            data = f.read()
        pos, n = data.find(isa.BUNDLE_MAGIC), 0
        while pos >= 0:
            (count,) = struct.unpack_from("<Q", data, pos + 24)
            off, end = pos + 32, pos + 32
            for _ in range(count):
                eoff, esize, tlen = struct.unpack_from("<QQQ", data, off)
                triple = data[off + 24:off + 24 + tlen].decode()
                off += 24 + tlen
                end = max(end, pos + eoff + esize)
                if esize and triple.split("-")[-1].split(":")[0] == isa.TARGET:
                    co = os.path.join(tmp, f"co{n}.o")
                    n += 1
                    with open(co, "wb") as f:
                        f.write(data[pos + eoff:pos + eoff + esize])
                    notes = subprocess.run([isa._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
                    for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                        name = re.search(r"\n\s*\.name:\s*(\S+)", entry).group(1)
                        found[name] = (int(re.search(r"\n\s*\.vgpr_count:\s*(\d+)", entry).group(1)),
                                       int(re.search(r"\n\s*\.private_segment_fixed_size:\s*(\d+)", entry).group(1)))
            pos = data.find(isa.BUNDLE_MAGIC, end)
    assert found, f"no {isa.TARGET} kernel metadata in {lib}"
    out = {}
    for mangled, figures in found.items():
        # _ZN3gvi<len><name>I<L i|b value E ...>E...: integer and bool template arguments only in these families
        m = re.match(r"^_ZN3gvi(\d+)", mangled)
        if not m:
            continue
        name = mangled[m.end():m.end() + int(m.group(1))]
        args = re.match(r"^I((?:L[ib]\d+E)+)E", mangled[m.end() + int(m.group(1)):])
        if not args:
            continue
        plain = ", ".join(v if t == "i" else ("true" if v == "1" else "false") for t, v in re.findall(r"L([ib])(\d+)E", args.group(1)))
        if f"{name}<".startswith(FAMILIES):
            out[f"{name}<{plain}>"] = figures
    return out


@pytest.fixture(scope="module")
def built():
    return resources()


def test_every_instance_with_the_walk_is_covered(built):
    assert sorted(built) == sorted(PARENT), sorted(set(built) ^ set(PARENT))


@pytest.mark.parametrize("name", sorted(PARENT))
def test_no_more_registers_or_scratch_than_with_the_odd_scalar(built, name):
    vgpr, scratch = built[name]
    print(f"{name}: VGPRs {vgpr} (parent {PARENT[name][0]}), scratch {scratch} bytes per lane (parent {PARENT[name][1]})")
    assert vgpr <= PARENT[name][0] and scratch <= PARENT[name][1]
    if name in FOUR_BLOCKS:
        assert vgpr <= 128
