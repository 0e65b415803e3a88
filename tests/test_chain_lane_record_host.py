"""The lane records of the chain eliminations (gaussianvi_amd/csrc/chain_lane_record.hpp) as plain C++ (CPU only).

tests/stubs/chain_lane_record_check.cpp restates the expressions `eliminate` used to form per call -- the roles isD / isE / isA /
isB / isY, the column cc, the operands p0 / s0 / p1 of the column load with the select of the identity columns, the places of
the factor store and of the accumulator adds -- and compares them with what the record gives, for every lane 0 .. 63 of the
two layouts the kernels use it for (factorisation and solve, two-row form, N = 6), with and without either neighbour, on a
stand-in for the pass's LDS whose contents are never 0 or 1 outside the zero and identity blocks.  The column values are compared as bits.  The program runs as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "chain_lane_record_check.cpp")
INC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
LAYOUTS = 2          # the calls in the stub's main
LANES = 64


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_lane_of_every_layout(build, tmp_path):
    exe = str(tmp_path / "chain_lane_record_check")
    r = subprocess.run(BUILDS[build] + ["-I", INC, STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    word, n = r.stdout.split()
    print(f"    {build}: {n} comparisons")
    # per lane: roles, cc, offsets (3) and per (slot, has_a, has_b) at least the N column rows
    assert word == "ok" and int(n) >= LAYOUTS * LANES * (3 + 3 * 4 * 4)
