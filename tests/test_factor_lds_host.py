"""The LDS layouts of the factor stage (gaussianvi_amd/csrc/factor_lds.hpp) through a stand-alone program
(tests/stubs/factor_lds_check.cpp), as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer: where every
kernel that carves its dynamic LDS by hand puts its regions, and how many bytes its launch asks for.  The pinned sizes are
written out here by hand from the formulas the launches have always used; the sweep compares every layout with
tests/factor_lds_model.py and then checks, on the program's own answer, that the regions ascend without overlap, start on whole
doubles, and that every view ends inside its area.  Nothing expected is read back from the header."""
import os
import subprocess

import pytest

import factor_lds_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "factor_lds_check.cpp")
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
DS = range(1, 33)


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("factor_lds_" + request.param)
    exe = str(tmp / "factor_lds_check")
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
    return [M.parse(l) for l in lines]


# ---- pinned by hand ----
def test_pinned_products_area_and_host_sizes(program):
    # d: (area, Sl, ml, staged_end, bytes of prep_kernel, bytes of prep_all_kernel); odd d (dp != d), the instantiated shapes, the
    # arm graph's d = 28, the limit
    want = {1: (12, 13, 14, 15, 112, 136), 3: (55, 56, 65, 68, 456, 560), 6: (177, 178, 214, 220, 1432, 1776),
            12: (642, 643, 787, 799, 5152, 6408), 28: (3290, 3291, 4075, 4103, 26336, 32840), 32: (4272, 4273, 5297, 5329, 34192, 42648)}
    got = _ask(program, "pinned_products", [f"products {d}" for d in want])
    for d, g in zip(want, got):
        assert (g["doubles"], g["Sl"], g["ml"], g["staged_end"], g["prep_bytes"], g["prep_all_bytes"]) == want[d], d
    g = got[1]                     # d = 3, written out: dd = 9, dp = 4
    assert (g["A0"], g["A1"], g["V0"], g["V1"], g["al"], g["be"], g["lam"], g["pa"], g["jacobi_end"]) == (0, 9, 18, 27, 36, 40, 44, 53, 55)
    assert (g["Ll"], g["Xl"], g["Al"], g["chol_end"]) == (0, 9, 18, 27)


def test_pinned_item_area_and_fused_sizes(program):
    got = _ask(program, "pinned_item", [f"item {d}" for d in (4, 6, 8, 12)] + ["fixed 8"])
    assert [g["item"] for g in got[:4]] == [110, 222, 376, 802]
    assert got[4]["block3"] == 376                                      # factor_block3_kernel: the item area at d = 8, per wave
    # fused_lds_doubles = 4 regions + items (keep + 4 npairs(dmax)) for the three instances of with_fused_instance: <6, 4, 4, 12, 6>
    # and <6, 6, 2, 12, 6> share (dmax, M) = (12, 6); <2, 4, 4, 4, 2> has (4, 2).  A chain of T states has T - 1 binary and T unary
    # factors, so a block holds at most 3 items.  copies: 1, and the 8 the launch takes by default (orbit_copies = 8 fits the LDS cap
    # of each instance's occupancy: 4 waves x (72 + 8 x 91) doubles = 25.6 KB <= 40 KB at WAVES = 4, <= 64 KB at WAVES = 2).
    # walk = (d hstride(M) + copies npairs(d) + 1) & ~1; keep = dmax^2 + dmax hstride(M) + M + (M & 1)
    cases = [(12, 164, 222, 3), (12, 800, 222, 3), (4, 24, 26, 3), (4, 128, 26, 3), (12, 800, 222, 1)]
    got = _ask(program, "pinned_fused", [f"fused {dmax} {walk} {keep} {items}" for dmax, walk, keep, items in cases])
    assert [(g["region"], g["lds"]) for g in got] == [(802, 4966), (802, 4966), (110, 698), (128, 770), (802, 3794)]
    assert 4966 == 4 * 802 + 3 * (222 + 4 * 91) and 698 == 4 * 110 + 3 * (26 + 4 * 15)
    assert (M.walk(12, 6, 1), M.walk(12, 6, 8), M.keep(12, 6), M.walk(4, 2, 1), M.walk(4, 2, 8), M.keep(4, 2)) == (164, 800, 222, 24, 128, 26)


def test_pinned_generic_kernel(program):
    # (2 256 (d + 1) + 256 + dd + d + m d + 2 m) 8 bytes, refused above 160 KB = 163840
    got = _ask(program, "pinned_generic", ["generic 32 32", "generic 34 30", "generic 34 31"])
    assert [(g["bytes"], g["refused"]) for g in got] == [(154368, 0), (163568, 0), (163856, 1)]
    # (34, 31) is the first refusal in the order d ascending, then m = 0 .. d ascending
    pairs = [(d, m) for d in range(1, 36) for m in range(0, d + 1)]
    got = _ask(program, "first_refusal", [f"generic {d} {m}" for d, m in pairs])
    refused = [p for p, g in zip(pairs, got) if g["refused"]]
    assert refused[0] == (34, 31) and pairs[pairs.index((34, 31)) - 1] == (34, 30)


def test_pinned_epilogue_and_fixed_sizes(program):
    e = _ask(program, "pinned_epilogue", ["epilogue 6", "epilogue 12"])
    assert (e[0]["doubles"], e[0]["all_doubles"], e[0]["last"]) == (28 + 144, 28 + 144 + 256, 172)           # (npairs + 4dd) 8 bytes
    assert (e[1]["doubles"], e[1]["tree"], e[1]["all_doubles"]) == (91 + 576, 667, 667 + 256)
    f = _ask(program, "pinned_fixed", ["fixed 3", "fixed 89", "fixed 90", "fixed 24"])
    assert (f[0]["box"], f[0]["halfspace"]) == (9 + 6, 64 * 3 + 128)
    assert (f[1]["box_refused"], f[2]["box_refused"]) == (0, 1)                                             # 64 KB: d <= 89
    assert f[3]["split"] == 256 + 48 + 8 + 512 + 4160 + 768
    assert _ask(program, "pinned_jko", ["jko 18"])[0] == dict(M=0, Sg=324, Tm=648, end=972, bytes=7776)


# ---- the sweep ----
def _ordered(bounds):
    return all(a <= b for a, b in zip(bounds, bounds[1:])) and bounds[0] >= 0


def test_sweep_against_the_model(program):
    cmds, want = [], []
    for d in DS:
        for name, args, model in (("products", (d,), M.products(d)), ("epilogue", (d,), M.epilogue(d)), ("item", (d,), M.item(d)),
                                  ("jko", (d,), M.jko(d)), ("fixed", (d,), M.fixed(d))):
            cmds.append(f"{name} " + " ".join(map(str, args)))
            want.append(model)
        for m in range(0, d + 1):
            cmds += [f"generic {d} {m}", f"chol {d} {m}", f"helper {d} {m}"]
            want += [M.generic(d, m), M.chol(d, m), M.helper(d, m)]
        for Mw in (2, 6, 12, 14):
            for copies in (1, 2, 8, 16):
                for items in (1, 3, 4):
                    cmds.append(f"fused {d} {M.walk(d, Mw, copies)} {M.keep(d, Mw)} {items}")
                    want.append(M.fused(d, M.walk(d, Mw, copies), M.keep(d, Mw), items))
    got = _ask(program, "sweep", cmds)
    wrong = [(c, w, g) for c, w, g in zip(cmds, want, got) if w != g]
    assert not wrong, wrong[:3]


def test_sweep_regions_on_the_programs_answer(program):
    """ascending, disjoint, on whole doubles (every offset is an integer count of doubles from a base of doubles: 8-byte starts for
    the double regions, and for the int regions pa and `last`, which need 4), every view inside its area -- read off the program's
    answers alone"""
    P = dict(zip(DS, _ask(program, "regions_products", [f"products {d}" for d in DS])))
    E = dict(zip(DS, _ask(program, "regions_epilogue", [f"epilogue {d}" for d in DS])))
    I = dict(zip(DS, _ask(program, "regions_item", [f"item {d}" for d in DS])))
    for d in DS:
        p, e, item = P[d], E[d], I[d]["item"]
        dd, dp = d * d, d + (d & 1)
        # the Jacobi view: four d x d blocks, two dp vectors, three d vectors, dp ints; inside the area
        assert _ordered([p["A0"], p["A0"] + dd, p["A1"], p["A1"] + dd, p["V0"], p["V0"] + dd, p["V1"], p["V1"] + dd, p["al"], p["al"] + dp,
                         p["be"], p["be"] + dp, p["lam"], p["lam"] + 3 * d, p["pa"]]), d
        assert 8 * p["pa"] + 4 * dp <= 8 * p["jacobi_end"] <= 8 * p["doubles"], d
        # the Cholesky view with m = d rows of A; the area is the larger of the two views
        assert _ordered([p["Ll"], p["Ll"] + dd, p["Xl"], p["Xl"] + dd, p["Al"], p["Al"] + d * d]) and p["Al"] + d * d == p["chol_end"], d
        assert p["doubles"] == max(p["jacobi_end"], p["chol_end"]), d
        # staging behind the area, the launches hold what their kernels carve
        assert _ordered([p["doubles"], p["Sl"], p["Sl"] + dd, p["ml"], p["ml"] + d, p["staged_end"]]), d
        assert 8 * p["doubles"] <= p["prep_bytes"] and 8 * p["staged_end"] <= p["prep_all_bytes"], d
        # a launch sized for dmax holds the layout of every d <= dmax (prep_all_kernel, epilogue_all_kernel: mixed d in one launch)
        for dmax in range(d, 33):
            assert 8 * p["staged_end"] <= P[dmax]["prep_all_bytes"] and e["end"] <= E[dmax]["tree"] <= E[dmax]["all_doubles"] - 256, (d, dmax)
        # the epilogue view, its `last` word behind it
        npo = (d + 1) * (d + 2) // 2
        assert _ordered([e["Ms"], e["Ms"] + npo, e["M2"], e["M2"] + dd, e["Tm"], e["Tm"] + dd, e["Sv"], e["Sv"] + dd, e["Lv"], e["Lv"] + dd,
                         e["end"], e["doubles"], e["last"]]), d
        # the item area holds both phases, the tail's word included, and keeps the next wave's area on 16 bytes
        assert item % 2 == 0 and p["staged_end"] <= item and 8 * e["last"] + 4 <= 8 * item, d
    GD = [(d, m) for d in DS for m in range(0, d + 1)]
    for (d, m), g, c, h in zip(GD, _ask(program, "regions_generic", [f"generic {d} {m}" for d, m in GD]),
                               _ask(program, "regions_chol", [f"chol {d} {m}" for d, m in GD]), _ask(program, "regions_helper", [f"helper {d} {m}" for d, m in GD])):
        z = 256 * (d + 1)
        assert _ordered([g["zs"], g["zs"] + z, g["xs"], g["xs"] + z, g["cs"], g["cs"] + 256, g["Ssh"], g["Ssh"] + d * d, g["mush"], g["mush"] + d,
                         g["Ash"], g["Ash"] + m * d, g["bsh"], g["bsh"] + m, g["gsh"], g["gsh"] + m, g["end"]]) and 8 * g["end"] <= g["bytes"], (d, m)
        assert g["refused"] == 0, (d, m)                                   # no shape the prep kernels take is refused
        assert c["chol_end"] <= P[d]["doubles"], (d, m)                    # the Cholesky view for every m <= d
        assert _ordered([h["Al"], h["Al"] + m * d, h["mh"], h["mh"] + d, h["end"]]), (d, m)
    # the helper wave's view inside a region of both fused instances at copies = 1
    for Mw, dmax in ((6, 12), (2, 4)):
        h = _ask(program, "helper_fused", [f"helper {dmax} {Mw}"])[0]
        r = _ask(program, "region_fused", [f"fused {dmax} {M.walk(dmax, Mw, 1)} {M.keep(dmax, Mw)} 1"])[0]
        assert h["end"] == Mw * dmax + dmax <= r["region"], (Mw, dmax)


def test_the_layout_is_written_once():
    """what the issue asks of the text: the header is plain C++ without a heap, and the arithmetic of the products area stands in
    it and nowhere else under csrc"""
    header = open(os.path.join(CSRC, "factor_lds.hpp")).read()
    assert "#include <hip" not in header and "__global__" not in header
    for word in ("std::vector", "<vector>", "malloc", "new "):
        assert word not in header
    for name in sorted(os.listdir(CSRC)):
        if name != "factor_lds.hpp":
            text = open(os.path.join(CSRC, name)).read()
            assert "(dp + 1) / 2" not in text and "4 * dd + 2 * dp" not in text, name
            assert "behind prep_body's own LDS" not in text, name
            for word in ("size_t epilogue_lds_doubles", "size_t box_closed_lds_doubles", "size_t halfspace_closed_lds_doubles", "int SPLIT_LDS_DOUBLES",
                         "size_t fused_item_doubles", "size_t block3_lds_doubles"):
                assert word not in text, (name, word)
