"""The row-broadcast multiply-add of the Cholesky products (csrc/dpp_rowb.hpp rowb_fma, used by prep_chol_body):

    v_fmac_f64_dpp acc, src, -mul row_newbcast:n        acc += (src of lane n of the own 16-lane row) * (-mul)

Unlike the Gauss-Jordan update of the chain (tests/test_rowbcast_semantics_gpu.py: destination == broadcast operand) the
destination is a register of its own and the plain multiplier carries a negation modifier.  tests/rowb_fma_probe.hip is compiled
here and applies the form to a known lane pattern for every n in 0..15, every lane active as in the library.

Expected values are formed on the host.  All inputs are multiples of 1/8 below 2^10, so every product and sum is exact in
float64 and the comparison is bit for bit (no fused multiply-add needed on the host).  The three inputs differ in every lane,
so a result that took the wrong operand from the row, dropped the negation or used the destination as the broadcast operand
differs from the expected one."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("rowb_fma") / "librowb_fma_probe.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared",
                    os.path.join(HERE, "rowb_fma_probe.hip"), "-o", out], check=True, capture_output=True, text=True)
    lib = C.CDLL(out)
    lib.rowb_fma_probe.restype = C.c_int
    lib.rowb_fma_probe.argtypes = [C.c_void_p] * 4
    return lib


def inputs():
    lane = np.arange(64)
    acc = (lane * 3 + 2 + (lane % 7) * 0.125) * np.where(lane % 4 == 1, -1.0, 1.0)
    src = (lane * 8 + 1 + (lane % 5) * 0.125) * np.where(lane % 3 == 0, -1.0, 1.0)      # distinct per lane
    mul = ((lane * 7) % 13 - 6) * 0.25 + 0.125                                          # never zero, both signs
    return acc.astype(np.float64), src.astype(np.float64), mul.astype(np.float64)


def test_rowb_fma_adds_the_rows_lane_n_times_the_negated_multiplier(probe):
    acc, src, mul = inputs()
    out = np.zeros((16, 64))
    rc = probe.rowb_fma_probe(acc.ctypes.data, src.ctypes.data, mul.ctypes.data, out.ctypes.data)
    assert rc == 0, f"HIP error {rc}"
    lane = np.arange(64)
    exp = np.stack([acc + src[(lane // 16) * 16 + n] * (-mul) for n in range(16)])
    # the readings the form must NOT have: no negation; destination as the broadcast operand; the multiplier broadcast instead
    wrong = {"no negation": np.stack([acc + src[(lane // 16) * 16 + n] * mul for n in range(16)]),
             "dst broadcast": np.stack([acc + acc[(lane // 16) * 16 + n] * (-mul) for n in range(16)]),
             "multiplier broadcast": np.stack([acc + src * (-mul[(lane // 16) * 16 + n]) for n in range(16)])}
    for name, w in wrong.items():
        assert not np.array_equal(w, exp), name                 # (the inputs tell the readings apart)
        print(f"device result equals the '{name}' reading: {np.array_equal(out, w)}")
    diff = np.argwhere(out != exp)
    print(f"{len(diff)} of {16 * 64} (n, lane) differ from acc - mul * src[lane n of the own row]"
          + "".join(f"\n    n {n} lane {ln}: got {out[n, ln]!r}, expected {exp[n, ln]!r}" for n, ln in diff[:12]))
    assert np.array_equal(out, exp)
