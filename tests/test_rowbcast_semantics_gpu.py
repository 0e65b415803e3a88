"""The 64-bit DPP row broadcast the n = 6 chain eliminations rely on (kernels_chain.hpp, chain::eliminate, option chain_pair):
`row_newbcast:n` makes every lane read the operand from lane n of its OWN 16-lane row.  tests/rowbcast_probe.hip is compiled
here and applies the three forms the library uses (the 32-bit builtin on both halves, v_mov_b64_dpp, and the fused
v_fmac_f64_dpp  c += bcast_n(c) * b  with destination == broadcast operand) to a known lane pattern, for every n in 0..15.

Expected values are formed on the host.  All inputs are multiples of 1/8 below 2^10, so every product and sum is exact in
float64 and the comparison is bit for bit (no fused-multiply-add needed on the host).

With lanes switched off in EXEC: a lane that is off keeps what it had; an active lane whose SOURCE lane is off is, by the DPP
rules of the ISA manual (bound_ctrl clear), not written either -- the move forms keep their old value and the fused form keeps
c.  The library never depends on that case (every lane runs the Gauss-Jordan); the test pins it so that it is known."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -777.125
FORMS = ("builtin pair", "v_mov_b64_dpp", "v_fmac_f64_dpp")
FULL = (1 << 64) - 1
# lanes off: one per row at different positions, two in row 0, and the whole upper half of row 2
PARTIAL = FULL & ~((1 << 3) | (1 << 7) | (1 << (16 + 5)) | (0xFF << (32 + 8)) | (1 << (48 + 15)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("rowbcast") / "librowbcast_probe.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared",
                    os.path.join(HERE, "rowbcast_probe.hip"), "-o", out], check=True, capture_output=True, text=True)
    lib = C.CDLL(out)
    lib.rowbcast_probe.restype = C.c_int
    lib.rowbcast_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_double]
    return lib


def inputs():
    lane = np.arange(64)
    v = (lane * 8 + 1 + (lane % 5) * 0.125) * np.where(lane % 3 == 0, -1.0, 1.0)      # distinct per lane
    b = ((lane * 7) % 13 - 6) * 0.25 + 0.125
    return v.astype(np.float64), b.astype(np.float64)


def expected(v, b, mask):
    exp = np.full((3, 16, 64), SENTINEL)
    for n in range(16):
        for lane in range(64):
            if not (mask >> lane) & 1:
                continue                                        # lane off: keeps the sentinel
            src = (lane // 16) * 16 + n
            src_on = (mask >> src) & 1
            exp[0, n, lane] = exp[1, n, lane] = v[src] if src_on else SENTINEL
            exp[2, n, lane] = v[lane] + v[src] * b[lane] if src_on else v[lane]
    return exp


@pytest.mark.parametrize("mask", [FULL, PARTIAL], ids=["all_lanes", "lanes_off"])
def test_row_newbcast_reads_lane_n_of_the_own_row(probe, mask):
    v, b = inputs()
    out = np.zeros((3, 16, 64))
    rc = probe.rowbcast_probe(v.ctypes.data, b.ctypes.data, out.ctypes.data, mask, SENTINEL)
    assert rc == 0, f"HIP error {rc}"
    exp = expected(v, b, mask)
    for f, name in enumerate(FORMS):
        diff = np.argwhere(out[f] != exp[f])
        print(f"{name}: {len(diff)} of {16 * 64} (n, lane) differ from 'lane n of the own row'"
              + "".join(f"\n    n {n} lane {lane}: got {out[f, n, lane]!r}, expected {exp[f, n, lane]!r}" for n, lane in diff[:12]))
    assert np.array_equal(out, exp)
