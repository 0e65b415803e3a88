"""The decisions of the chain stage (gaussianvi_amd/csrc/chain_plan.hpp) through a stand-alone program
(tests/stubs/chain_plan_check.cpp), as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer: the shape
functions, the LDS footprints, the shape test of the batched assemble load, and chain_decide -- which launches a chain operation
goes out as, in which form, with how many workgroups and how much LDS, and when it is refused.  The pinned plans are written out
here; the sweep compares every plan with tests/chain_plan_model.py and then checks, on the program's own answer, that no
supported shape is refused, that every launch fits LDS, that the passes cover every level once, that the grids are
ceil(T / stride) and that the merged launch is taken exactly when it fits.  Nothing expected is read back from the header."""
import itertools
import os
import subprocess

import pytest

import chain_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "chain_plan_check.cpp")
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
BOTH = dict(on0=1, back0=1, on1=1)


def _cmd(T, n, **kv):
    return f"plan T={T} n={n} " + " ".join(f"{k}={int(v)}" for k, v in kv.items())


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("chain_plan_" + request.param)
    exe = str(tmp / "chain_plan_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return tmp, exe


def _ask(program, name, commands):
    tmp, exe = program
    script = tmp / (name + ".txt")
    script.write_text("\n".join(commands) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(commands), r.stdout[-2000:]
    return lines


def _plans(program, name, cases):
    """cases: [(T, n, facts and rules)] -> parsed plans, each first compared with the model's line"""
    lines = _ask(program, name, [_cmd(T, n, **kv) for T, n, kv in cases])
    wrong = [(c, M.line(M.plan(c[0], c[1], **c[2])), got) for c, got in zip(cases, lines) if got != M.line(M.plan(c[0], c[1], **c[2]))]
    assert not wrong, wrong[:3]
    return [M.parse(l) for l in lines]


def _brief(p):
    """(kernel, form, S of its pass, top?, nb0, nb) per launch"""
    return [(l["kernel"], l["form"]) + ((l["pass_"]["S"], l["pass_"]["top"]) if l["pass_"] else ()) + (l["nb0"], l["nb"]) for l in p[4]]


# ---- the pinned plans ----
def test_pinned_plans(program):
    cases = [
        (48, 6, dict(BOTH)),                        # 0  the last n = 6 chain that fits the top pass
        (49, 6, dict(BOTH)),                        # 1
        (49, 6, dict(BOTH, merge=1)),               # 2
        (49, 6, dict(on0=1, merge=1)),              # 3  log-det only: nothing to carry
        (1025, 6, dict(BOTH, merge=1)),             # 4
        (1025, 6, dict(BOTH)),                      # 5
        (17, 6, dict(BOTH)),                        # 6  a pass is crowded from 18 states on
        (18, 6, dict(BOTH)),                        # 7
        (1025, 6, dict(BOTH, merge=1, pair=0)),     # 8
        (48, 5, dict(BOTH, pair=0)),                # 9
        (1025, 5, dict(on1=1, merge=1)),            # 10 the solve alone
        (1025, 6, dict(on0=1, back0=1, merge=1)),   # 11 the factorisation alone
    ]
    p = _plans(program, "pinned", cases)
    assert all(q[0] == "Ok" and q[1] == "Off" and q[2] == 1024 for q in p)
    assert _brief(p[0]) == [("Forward", "TwoRow", 48, 1, 1, 2)] and p[0][4][0]["pass_"]["m"] == 6
    seg49 = ("Forward", "TwoRow", 32, 0, 2, 4)
    assert _brief(p[1]) == [seg49, ("Forward", "Readlane", 2, 1, 1, 2), ("Backward", "Own", 32, 0, 2, 4)]
    assert p[1][4][0]["pass_"] == dict(level0=0, m=5, S=32, top=0, first=1, par=0, lp_off=0, blocks=2)
    assert p[1][4][1]["pass_"] == dict(level0=5, m=1, S=2, top=1, first=0, par=1, lp_off=32, blocks=1)
    assert _brief(p[2]) == [seg49, ("TopBack", "Readlane", 2, 1, 1, 2 + 4)]
    assert p[2][4][1]["carried"] == p[2][4][0]["pass_"] and (p[2][4][1]["nbt"], p[2][4][1]["nb0c"]) == (2, 2)
    assert _brief(p[3]) == [("Forward", "TwoRow", 32, 0, 2, 2), ("Forward", "Readlane", 2, 1, 1, 1)]
    assert _brief(p[4]) == [("Forward", "TwoRow", 32, 0, 33, 66), ("TopBack", "TwoRow", 33, 1, 1, 2 + 66)]
    assert (p[4][4][1]["nbt"], p[4][4][1]["nb0c"], p[4][4][1]["carried"]["blocks"]) == (2, 33, 33)
    assert _brief(p[5]) == [("Forward", "TwoRow", 32, 0, 33, 66), ("Forward", "TwoRow", 33, 1, 1, 2), ("Backward", "Own", 32, 0, 33, 66)]
    assert _brief(p[6]) == [("Forward", "Readlane", 17, 1, 1, 2)] and _brief(p[7]) == [("Forward", "TwoRow", 18, 1, 1, 2)]
    assert _brief(p[8]) == [("Forward", "Readlane", 32, 0, 33, 66), ("TopBack", "Readlane", 33, 1, 1, 2 + 66)]
    assert _brief(p[9]) == [("Forward", "Readlane", 48, 1, 1, 2)]
    assert _brief(p[10]) == [("Forward", "TwoRow", 32, 0, 0, 33), ("TopBack", "TwoRow", 33, 1, 0, 1 + 33)]
    assert (p[10][4][1]["nbt"], p[10][4][1]["nb0c"]) == (1, 0)
    assert _brief(p[11]) == [("Forward", "TwoRow", 32, 0, 33, 33), ("TopBack", "TwoRow", 33, 1, 1, 1 + 33)]
    assert (p[11][4][1]["nbt"], p[11][4][1]["nb0c"]) == (1, 33)
    # the two-row form pays for its lane records, identity and zero block and its log-pivot slots: (96 + 128 + 2 * 36) doubles
    assert p[4][4][0]["lds"] - p[8][4][0]["lds"] == 8 * (96 + 128 + 72)
    # T = 1025, n = 6, written out: top pass of 33 nodes, factorisation body, two-row; backward pass of 32, selected inverse
    top_e = 2 * 34 * 36 + 2 * 33 * 36 + 3 * 33 * 36 + 33 * 36 + 6 + 128 + 96 + 128 + 72
    assert p[5][4][1]["lds"] == 8 * top_e == 80048
    assert p[5][4][2]["lds"] == 8 * (5 * 33 * 36 + 3 * 32 * 36 + 2) == 75184
    assert p[4][4][1]["lds"] == max(p[5][4][1]["lds"], p[5][4][2]["lds"])


def test_forms_and_the_wave_kernel(program):
    generic = dict(BOTH, merge=1)
    # n != 6: never the readlane family, always the kernel's own form, whatever chain_pair says
    cases = [(T, n, dict(generic, pair=pair, wave=0)) for n in range(1, 17) if M.padded(n) != 6 for T in (1, 2, 17, 18, 66, 129, 1025) for pair in (0, 1)]
    for (T, n, kv), p in zip(cases, _plans(program, "own", cases)):
        assert p[0] == "Ok" and {l["form"] for l in p[4]} == {"Own"}, (T, n)
    # chain_pair off: readlane everywhere (the backward kernel has one form)
    cases = [(T, n, dict(generic, pair=0)) for n in (5, 6) for T in (1, 17, 18, 48, 49, 1025, 40000)]
    for p in _plans(program, "pair_off", cases):
        assert {l["form"] for l in p[4] if l["kernel"] != "Backward"} == {"Readlane"} and {l["form"] for l in p[4] if l["kernel"] == "Backward"} <= {"Own"}
    # n <= 2, T <= 65, chain_wave on: one Wave launch of one block per operation
    cases = [(T, n, dict(ops, merge=1)) for n in (1, 2) for T in (1, 2, 64, 65) for ops in (BOTH, dict(on0=1), dict(on1=1))]
    for (T, n, kv), p in zip(cases, _plans(program, "wave", cases)):
        ops = kv.get("on0", 0) + kv.get("on1", 0)
        assert p[:4] == ("Ok", "Off", 64, 0) and _brief(p) == [("Wave", "Own", kv.get("on0", 0), ops)] and p[4][0]["lds"] == 0
    # T = 66, n = 3, or chain_wave off: the generic plan; n = 2, T <= 128: a single top launch
    cases = [(66, 2, generic), (66, 1, generic), (64, 3, generic), (65, 2, dict(generic, wave=0)), (5, 1, dict(generic, wave=0)), (128, 2, generic)]
    for (T, n, kv), p in zip(cases, _plans(program, "no_wave", cases)):
        assert _brief(p) == [("Forward", "Own", T, 1, 1, 2)] and p[2] == 1024, (T, n)
    p129, p65 = _plans(program, "two_passes", [(129, 2, generic), (65, 3, generic)])         # one state past the top pass of n <= 2 / n = 3
    assert _brief(p129) == [("Forward", "Own", 32, 0, 5, 10), ("TopBack", "Own", 5, 1, 1, 2 + 10)]
    assert _brief(p65) == [("Forward", "Own", 32, 0, 3, 6), ("TopBack", "Own", 3, 1, 1, 2 + 6)]


def test_nothing_to_do_and_refusals(program):
    p = _plans(program, "edge", [(100, 6, dict()), (100, 0, BOTH), (100, 17, BOTH), (100, -3, BOTH), (3, 17, dict(BOTH, list=1, shape=1)),
                                 (100, 17, dict(on0=1, wave=0, merge=1))])
    assert p[0] == ("Ok", "Off", 0, 0, [])
    assert [q[0] for q in p[1:]] == ["BlockSize"] * 5 and all(q[4] == [] for q in p[1:])         # unsupported before any launch


def test_assemble_mode(program):
    n = 6
    B, U = (4, 2 * n, 0, 1), (5, n, 0, 1)                  # (K, d, sparse states, data): a binary and a unary dense set
    sets = {
        "binary": [B], "unary": [U], "binary + unary": [B, U], "unary + binary": [U, B],
        "none": [], "two binary": [B, B], "two unary": [U, U], "a third set": [B, U, U], "sparse": [B, (2, n, 2, 1)], "sparse alone": [(2, n, 2, 1)],
        "another d": [B, (5, 4, 0, 1)], "another d alone": [(5, 3 * n, 0, 1)], "empty set": [B, (0, n, 0, 1)], "no data": [(4, 2 * n, 0, 0), U],
    }
    dense = {"binary", "unary", "binary + unary", "unary + binary"}
    got = _ask(program, "dense", [f"dense {n} " + " ".join(f"; {K} {d} {nsp} {data}" for K, d, nsp, data in s) for s in sets.values()])
    assert got == [f"dense {int(name in dense)}" for name in sets]
    assert all(M.asm_dense_shape(s, n) == (name in dense) for name, s in sets.items())
    # the same sets at another block size are no chain pattern
    assert _ask(program, "dense_n", [f"dense 3 ; {B[0]} {B[1]} 0 1 ; {U[0]} {U[1]} 0 1", "dense 12 ; 5 12 0 1", "dense 12 ; 5 24 0 1 ; 5 12 0 1"]) == ["dense 0", "dense 1", "dense 1"]
    cases = [(T, nn, dict(BOTH, merge=1, **kv)) for T, nn in ((5, 2), (70, 6), (1025, 6)) for kv in
             (dict(list=1, shape=1), dict(list=1, shape=0), dict(list=1, shape=1, asm_dense=0), dict(list=0, shape=1), dict())]
    p = _plans(program, "assemble", cases)
    assert [q[1] for q in p] == ["Dense", "Generic", "Generic", "Off", "Off"] * 3
    one = _plans(program, "assemble_T1", [(1, 6, dict(BOTH, list=1, shape=1)), (1, 2, dict(BOTH, list=1, shape=1)), (2, 2, dict(BOTH, list=1, shape=1))])
    assert [q[1] for q in one] == ["Generic", "Generic", "Dense"]
    # the assemble mode changes no launch
    assert all(p[base + j][2:] == p[base][2:] for base in (0, 5, 10) for j in range(1, 5))


def test_shape_functions_and_lds(program):
    Ts = (1, 2, 3, 4, 5, 64, 65, 1024, 1025, 2 ** 20 + 1, 2 ** 31 - 1)
    cmds = [f"shape {T} {n}" for T in Ts for n in range(-1, 19)]
    want = []
    for T in Ts:
        for n in range(-1, 19):
            N = M.padded(n)
            lp = 2 * T + 1024
            want.append(f"shape {N} {int(N != 0)} {M.levels(T)} {M.threads(N) if N else 0} {lp} {10 * T * N * N + 5 * T * N + lp}")
    assert _ask(program, "shape", cmds) == want
    assert [M.padded(n) for n in range(0, 18)] == [0, 1, 2, 3, 4, 6, 6, 8, 8, 12, 12, 12, 12, 16, 16, 16, 16, 0]
    assert [M.levels(T) for T in (1, 2, 3, 4, 5, 1025, 2 ** 31 - 1)] == [0, 1, 2, 2, 3, 11, 31]
    combos = list(itertools.product((0, 1), (0, 1), (0, 1), M.PADDED, (1, 2, 8, 17, 32, 48, 128), (0, 1)))
    got = _ask(program, "fwd", [f"fwd {e} {y} {top} {N} {S} {rowb}" for e, y, top, N, S, rowb in combos])
    assert got == [f"fwd {M.fwd_doubles(e, y, top, N, S, rowb)}" for e, y, top, N, S, rowb in combos]
    combos = list(itertools.product((0, 1), M.PADDED, (1, 8, 16, 32)))
    got = _ask(program, "bwd", [f"bwd {e} {N} {S}" for e, N, S in combos])
    assert got == [f"bwd {M.bwd_doubles(e, N, S)}" for e, N, S in combos]
    # written out: a segmented pass of 32 nodes at N = 6, the solve's body, readlane form
    assert M.fwd_doubles(0, 1, 0, 6, 32, 0) == 2 * 33 * 36 + 2 * 32 * 36 + 2 * 33 * 6 + 6 + 128 == 5210
    assert M.bwd_doubles(0, 6, 32) == 33 * 6 + 32 * 6 + 2 * 32 * 36 + 2 == 2696


# ---- the sweep ----
SWEEP_T = list(range(1, 3001)) + [4097, 40000, 2 ** 20 + 1]
THIN_T = [T for T in SWEEP_T if T <= 200 or T % 37 == 0 or T > 3000]
LEGS = {
    "both merged": (dict(BOTH, merge=1, wave=0), SWEEP_T),
    "both merged, wave": (dict(BOTH, merge=1), THIN_T),
    "both separate": (dict(BOTH, wave=0), THIN_T),
    "log-det only": (dict(on0=1, merge=1, wave=0), THIN_T),
    "solve only, pair off": (dict(on1=1, merge=1, wave=0, pair=0), THIN_T),
}


@pytest.mark.parametrize("leg", list(LEGS))
def test_sweep(program, leg):
    kv, Ts = LEGS[leg]
    cases = [(T, n, kv) for n in range(1, 17) for T in Ts]
    plans = _plans(program, "sweep", cases)
    on0, back0, on1 = kv.get("on0", 0), kv.get("back0", 0), kv.get("on1", 0)
    back = bool(back0 or on1)
    nmerged = nwave = 0
    for (T, n, _), (status, assemble, thr, npass, launches) in zip(cases, plans):
        N = M.padded(n)
        assert status == "Ok" and launches, (T, n)                          # no supported shape is refused
        assert all(0 <= l["lds"] <= M.LDS_LIMIT for l in launches), (T, n)
        if launches[0]["kernel"] == "Wave":
            assert kv.get("wave", 1) and n <= 2 and T <= 65 and len(launches) == 1
            nwave += 1
            continue
        fwd = [l for l in launches if l["kernel"] in ("Forward", "TopBack")]
        bwd = [l for l in launches if l["kernel"] == "Backward"]
        assert launches == fwd + bwd and len(fwd) == npass and thr == (1024 if N <= 8 else 512)
        # the forward passes cover the levels 0 .. chain_levels(T) without gap or overlap, the top pass last
        level = 0
        for i, l in enumerate(fwd):
            q = l["pass_"]
            assert q["level0"] == level and q["first"] == int(i == 0) and q["par"] == i % 2 and q["top"] == int(i == npass - 1), (T, n)
            assert q["m"] >= (0 if q["top"] else 3) and (q["top"] or q["S"] == 1 << q["m"])
            level += q["m"]
            stride = q["S"] << q["level0"]
            blocks = 1 if q["top"] else -(-T // stride)
            assert q["blocks"] == blocks and (q["top"] == 0 or q["S"] == -(-T // (1 << q["level0"])))
            if l["kernel"] == "Forward":
                assert (l["nb0"], l["nb"]) == (blocks * on0, blocks * (on0 + on1)), (T, n)
        assert level == M.levels(T), (T, n)
        assert all(l["kernel"] == "Forward" for l in fwd[:-1])
        # log-pivot entries: one per wave of every workgroup of the earlier passes, inside the workspace's 2 T + 1024
        assert [l["pass_"]["lp_off"] for l in fwd] == [sum(g["pass_"]["blocks"] for g in fwd[:i]) * (thr // 64) for i in range(npass)]
        assert fwd[-1]["pass_"]["lp_off"] + thr // 64 <= 2 * T + 1024
        # the merged launch exactly when it is asked for, has something to carry and fits (its LDS from the model's size functions)
        top = fwd[-1]
        if npass >= 2:
            two = top["form"] == "TwoRow"
            c = fwd[-2]["pass_"]
            need = 8 * max(M.fwd_doubles(1, 0, 1, N, top["pass_"]["S"], two) if on0 else 0, M.fwd_doubles(0, 1, 1, N, top["pass_"]["S"], two) if on1 else 0,
                           M.bwd_doubles(1, N, c["S"]) if back0 else 0, M.bwd_doubles(0, N, c["S"]) if on1 else 0)
            fits = need <= M.LDS_LIMIT
        want_merged = bool(kv.get("merge", 0)) and back and npass >= 2 and fits
        assert (top["kernel"] == "TopBack") == want_merged, (T, n)
        # the backward launches: every segmented pass once, last first, the carried one inside the merged launch
        carried = [top["carried"]] if want_merged else []
        assert carried + [l["pass_"] for l in bwd] == ([g["pass_"] for g in reversed(fwd[:-1])] if back else []), (T, n)
        assert all((l["nb0"], l["nb"]) == (l["pass_"]["blocks"] * back0, l["pass_"]["blocks"] * (back0 + on1)) for l in bwd)
        if want_merged:
            nmerged += 1
            assert top["lds"] == need and (top["nb0"], top["nbt"], top["nb0c"]) == (on0, on0 + on1, c["blocks"] * back0)
            assert top["nb"] == top["nbt"] + c["blocks"] * (back0 + on1)
        # N = 6: two-row exactly on the crowded passes with chain_pair on; else the kernel's own form
        for l in fwd:
            crowded = l["pass_"]["S"] // 2 > thr // 128
            assert l["form"] == ("Own" if N != 6 else "TwoRow" if crowded and kv.get("pair", 1) else "Readlane"), (T, n)
    print(f"    {leg}: {len(cases)} plans, {nmerged} with a merged launch, {nwave} on the lane-per-node kernel")
    assert (nmerged > 0) == bool(kv.get("merge", 0) and back) and (nwave > 0) == bool(kv.get("wave", 1))


def test_capacities_hold_the_longest_chain(program):
    """At most 12 passes and 23 launches (the static_assert of the header).  The model, which the sweep holds equal to the header,
    counts the passes of 2^31 - 1 states; the program answers for 2^27 (beyond that the log-pivot offsets of ChainArgs, 32-bit,
    would overflow long before the capacities matter)."""
    assert max(len(M.passes(2 ** 31 - 1, N)) for N in M.PADDED) == 11 and len(M.passes(2 ** 31 - 1, 16)) == 11
    cases = [(2 ** 27, n, dict(BOTH, merge=merge, wave=0)) for n in (1, 6, 8, 12, 16) for merge in (0, 1)]
    for (T, n, kv), p in zip(cases, _plans(program, "longest", cases)):
        assert p[0] == "Ok" and p[3] == len(M.passes(T, M.padded(n))) <= 12 and len(p[4]) == 2 * p[3] - 1 - kv["merge"] <= 23
    assert max(p[3] for p in _plans(program, "longest", cases)) == 9


def test_the_headers_keep_no_second_copy_and_no_heap():
    """what the issue asks of the text: the plan header and the launcher allocate nothing, the launcher decides nothing on LDS
    sizes, and the kernel headers take their sizes from chain_plan.hpp"""
    read = lambda name: open(os.path.join(CSRC, name)).read()
    plan, launch = read("chain_plan.hpp"), read("chain_launch.hpp")
    for text in (plan, launch):
        assert "std::vector" not in text and "<vector>" not in text and "malloc" not in text and "new " not in text.replace("a new ", "")
    assert "#include <hip" not in plan and "__global__" not in plan
    assert "lds_doubles" not in launch and "_enabled()" not in launch
    for name in ("kernels_chain.hpp", "kernels_chain_wave.hpp", "chain_lane_record.hpp"):
        text = read(name)
        assert '#include "chain_plan.hpp"' in text
        for word in ("size_t fwd_lds_doubles", "size_t bwd_lds_doubles", "128 + 2 * N * N", "int chain_threads", "int WT_MAX", "bool chain_asm_dense",
                     "size_t chain_ws_doubles"):
            assert word not in text, (name, word)
    assert "process" not in read("options.hpp").replace("in-process", "")
