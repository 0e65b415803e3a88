"""Host side of the walk's priority bands (gaussianvi_amd/csrc/walk_prio.hpp, orbits.hpp::walk_prio_costs) and of the switch
"walk_prio" (options.hpp, OPTION_ROWS_LATER), through a stand-alone program (tests/stubs/walk_prio_check.cpp) built plain and
under AddressSanitizer / UndefinedBehaviorSanitizer.

For the tables the fused factor pass walks -- (12,5), (6,5), (4,5), (12,7), (6,7) -- split into four chunks, the program walks
every chunk as orbit_wave does: the wave's remaining modelled cost starts at the chunk's total, the priority is taken from it in
front of every tile and once behind the last one, and the tile's cost leaves it.  Checked here: every chunk's tile costs are
those of the model that places the chunk bounds (orbit_tile_cost: 300 / 800 / 1300 / 2500 / 5200 / 10800 cycles per orbit of a
lane at s = 1 .. 6, plus 600 per tile; asserted in the program against the table's own tile list) and sum to the chunk's
total; the priority never rises along a chunk, starts at 3 wherever a chunk has more than one tile (and in fact wherever it has
a tile), and ends at 0; the four bands are the geometric ones (remaining > 1/2, > 1/4, > 1/8 of the total)."""
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "walk_prio_check.cpp")
CASES = [(12, 5), (6, 5), (4, 5), (12, 7), (6, 7)]
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
WALK = {1: 300, 2: 800, 3: 1300, 4: 2500, 5: 5200, 6: 10800}          # orbits.hpp, orbit_tile_cost
DEFAULT = 1                                                            # Options::walk_prio


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("walk_prio_" + request.param) / "walk_prio_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def _chunks(exe, tmp_path, d, p):
    Z, w = o.nwspgr_cached(d, p)
    Z, w = np.ascontiguousarray(Z, dtype="<f8"), np.ascontiguousarray(w, dtype="<f8")
    path = tmp_path / f"table_{d}_{p}.bin"
    path.write_bytes(Z.tobytes() + w.tobytes())
    r = subprocess.run([exe, "table", str(path), str(d), str(len(w))], capture_output=True, text=True, env=ENV, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1].startswith(f"ok {d} {len(w)} "), r.stdout[-2000:] + r.stderr[-4000:]
    out = []
    for ln in lines[:-1]:
        f = ln.split()
        assert f[0] == "chunk" and f[2] == "total" and f[4] == "tiles" and f[6] == "costs", ln
        n = int(f[5])
        costs, prio = [int(v) for v in f[7:7 + n]], [int(v) for v in f[8 + n:]]
        assert f[7 + n] == "prio" and len(prio) == n + 1, ln
        out.append((int(f[3]), costs, prio))
    assert len(out) == 4
    return out, int(lines[-1].split()[3])


@pytest.mark.parametrize("d,p", CASES)
def test_bands_along_every_chunk(exe, tmp_path, d, p):
    chunks, smax = _chunks(exe, tmp_path, d, p)
    assert sum(len(c) for _, c, _ in chunks) > 0
    for w, (total, costs, prio) in enumerate(chunks):
        print(f"({d},{p}) chunk {w}: total {total}, tile costs {costs}, priorities {prio}")
        assert sum(costs) == total
        for c in costs:                                  # g orbits of one support size per lane + the tile's own 600 cycles
            assert any((c - 600) % WALK[s] == 0 and c > 600 for s in range(1, smax + 1)), c
        assert all(a >= b for a, b in zip(prio, prio[1:])), prio
        assert prio[-1] == 0
        if costs:
            assert prio[0] == 3
        rem = total
        for c, q in zip(costs + [0], prio):              # the geometric bands themselves
            assert q == (3 if rem > total // 2 else 2 if rem > total // 4 else 1 if rem > total // 8 else 0)
            rem -= c
    assert max(t for t, _, _ in chunks) < 2 ** 20        # (four items of a block: far inside 32 bits)


def test_the_switch_is_a_row_of_the_options_table(exe):
    r = subprocess.run([exe, "option"], capture_output=True, text=True, env=ENV, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == [f"default {DEFAULT}", "env 0 0", "set 0 0", "env 1 1", "set 1 1",
                                     "unknown 0 unknown option: walk_priority"]


def test_the_header_describes_the_switch():
    text = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    assert f"walk_prio (default {DEFAULT}; environment GVI_WALK_PRIO" in text
