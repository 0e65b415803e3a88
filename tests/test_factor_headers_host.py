"""The factor stage's headers (gaussianvi_amd/csrc): every stage header and every header that builds on them compiles as a
translation unit of its own, so its include list is the whole of its inputs; kernels_factor.hpp is the index of the stage and
nothing else, included by the library's translation unit alone.  CPU only: a device-side syntax pass of hipcc, nothing runs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
STAGE = ("factor_math.hpp", "kernels_prep.hpp", "mom_args.hpp", "kernels_closed.hpp", "kernels_reg.hpp", "kernels_split.hpp",
         "kernels_sreg.hpp", "kernels_epilogue.hpp")
USERS = ("kernels_readout.hpp", "kernels_sample_cost.hpp", "kernels_orbit.hpp", "kernels_orbit_psi.hpp", "kernels_fused.hpp",
         "kernels_block.hpp")


def _hipcc():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "bin", "hipcc"), shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError("hipcc not found: the library itself is built with it")


@pytest.mark.parametrize("header", STAGE + USERS)
def test_header_compiles_alone(header, tmp_path):
    tu = tmp_path / "tu.hip"
    tu.write_text(f'#include "{header}"\n')
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++20", "--cuda-device-only", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(tu)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_umbrella_is_an_index():
    """kernels_factor.hpp defines nothing and names every stage header; under csrc only gvi_hip.hip includes it"""
    umbrella = open(os.path.join(CSRC, "kernels_factor.hpp")).read()
    assert "__global__" not in umbrella and "__device__" not in umbrella
    assert re.findall(r'^#include "([^"]+)"', umbrella, re.M) == ["factor_math.hpp", "kernels_prep.hpp", "mom_args.hpp", "kernels_closed.hpp",
                                                                 "kernels_reg.hpp", "kernels_split.hpp", "kernels_sreg.hpp",
                                                                 "kernels_epilogue.hpp"]
    includers = [name for name in sorted(os.listdir(CSRC))
                 if re.search(r'^\s*#\s*include\s*"kernels_factor\.hpp"', open(os.path.join(CSRC, name), errors="replace").read(), re.M)]
    assert includers == ["gvi_hip.hip"]
