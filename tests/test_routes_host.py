"""Route selection of the factor stage (gaussianvi_amd/csrc/routes.hpp) through a stand-alone program
(tests/stubs/routes_check.cpp), as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer: the instance lists, the
route and chunking of one set's pass (decide_route) against the model of tests/route_model.py, the refusals with their exact
texts, which launches of the resident iteration go out as one (decide_fuse, decide_full) on the legs of
tests/test_factor_routes_gpu.py::test_resident_fusing restated as facts, and the integers gvi_profile_geometry reports.  Every
expected value is written out here or comes from route_model.py; none is read back from the header.

A table is described by the facts the decision reads of it: the stand-in below carries (N, largest support, tiles) where the
model reads them off the nodes.  Of the four refusals tests/test_factor_routes_gpu.py::test_refusals pins, "factor dimension
> 32" is the prep launch's own (it runs before any plan) and is no decision of the header: here its place is taken by the
generic kernel's and the half-space kernel's d <= 32, and by the miss of with_prep_instance at d = 33 that the launch answers
with that text."""
import itertools
import os
import subprocess

import pytest

import route_model as rm
from route_model import ARM, BODY, FIXED, H2D, H3D, OPSI_ROWS, PREP, QUAD, RANGE, REG, SCOST, SEG2, SEG3, SPLIT_D, SREG, _ceil, _chunks, _route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "routes_check.cpp")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
BOX, HALFSPACE = 10, 11
ERR_UNSUPPORTED, ERR_STATE = 3, 5
VARIANTS = (0, 1, 2, 5, 6, 7)
NAME = dict(orbit="Orbit", opsi="OrbitPsi", sreg="Sreg", scost="Scost", reg="Reg", split="Split", generic="Generic")
ROUTES = ("Empty", "Closed", "Orbit", "OrbitPsi", "Split", "Sreg", "Scost", "Reg", "Generic")     # enum class Route, in order
MSG_REG = "register kernel not instantiated for this (kind, d)"
MSG_SDF = "HINGE_SDF set without a grid: call gvi_factors_set_sdf2d / gvi_factors_set_sdf3d"
MSG_ARM = "HINGE_SDF_3D_ARM set without an arm model: call gvi_factors_set_arm"


class Table:
    """what the model reads off the nodes of a table, stated: N points, largest support of a sign orbit, 64-lane tiles"""

    def __init__(self, N, smax, tiles):
        self.N, self.shape = N, (smax, tiles)

    def __len__(self):
        return self.N


@pytest.fixture(autouse=True)
def _stated_tables(monkeypatch):
    monkeypatch.setattr(rm, "_orbit_shape", lambda Z: Z.shape)


# ---- the written-out instance lists ----
REG_BOX = (2, 4, 6, 8)                                  # HINGE_BOX: beside the 24 of route_model.REG (its sets default to the closed form)
REG_PSI = {RANGE: lambda d: "range", H2D: lambda d: f"sdf {d} 4", BODY: lambda d: f"sdf {d} 5", H3D: lambda d: f"sdf {d} 6",
           SEG2: lambda d: f"seg {d} 2", SEG3: lambda d: f"seg {d} 3", QUAD: lambda d: f"quad {d} {d // 2}", FIXED: lambda d: f"quad {d} {d}",
           BOX: lambda d: f"box {d}"}
ORBIT = {(2, False): "2 4 4 1", (14, False): "14 4 2 0", (6, False): "6 4 4 1", (6, True): "6 6 2 1", (12, False): "12 4 3 1",
         (12, True): "12 6 2 1"}                          # (m, support > 4) -> M SMAX WAVES PAIR
FUSED = {(6, False, 12, 6): "6 4 4 12 6", (6, True, 12, 6): "6 6 2 12 6", (2, False, 4, 2): "2 4 4 4 2"}
CLOSED = {QUAD: "sumsq", FIXED: "sumsq", BOX: "box", HALFSPACE: "halfspace"}
FORCE = {0: "1 0 1 1 0", 1: "0 0 0 0 0", 2: "1 1 0 0 0", 5: "1 0 1 0 0", 6: "1 0 0 1 0", 7: "1 0 1 1 1"}   # reg must_reg sgpr orbit opsi


def _m_fits(kind, d, m):
    return (kind != QUAD or d == 2 * m) and (kind != FIXED or d == m)


def _list_cases():
    """(command, expected answer) of every list"""
    out = []
    reg_all = {**REG, BOX: REG_BOX}
    for kind, d in itertools.product(range(-1, 13), range(1, 33)):
        for m in sorted({d, d // 2, 0}):
            hit = d in reg_all.get(kind, ()) and _m_fits(kind, d, m)
            out.append((f"reg {kind} {d} {m}", f"reg 1 {d} {REG_PSI[kind](d)}" if hit else "reg 0"))
            hit = d in SREG.get(kind, ()) and _m_fits(kind, d, m)
            out.append((f"sreg {kind} {d} {m}", f"sreg 1 {d} {m} {int((kind, d) != (FIXED, 12))}" if hit else "sreg 0"))
            hit = d in SCOST.get(kind, ()) and _m_fits(kind, d, m)
            out.append((f"scost {kind} {d} {m}", f"scost 1 {d} {m}" if hit else "scost 0"))
            if kind == 0:
                hit = d in SPLIT_D and m in (d, d // 2)
                out.append((f"split {d} {m}", f"split 1 {d} {_ceil(m, 4)}" if hit else "split 0"))
    for m, smax in itertools.product(range(1, 17), range(0, 9)):
        key = (m, smax > 4)
        hit = 1 <= smax <= 6 and key in ORBIT
        out.append((f"orbit {m} {smax}", f"orbit 1 {ORBIT[key]}" if hit else "orbit 0"))
        for d0, d1 in [(12, 6), (4, 2), (24, 12), (28, 14), (6, 12), (12, 12)]:
            key = (m, smax > 4, d0, d1)
            hit = 1 <= smax <= 6 and key in FUSED
            out.append((f"fused {m} {smax} {d0} {d1}", f"fused 1 {FUSED[key]}" if hit else "fused 0"))
    for kind in range(-1, 13):
        out.append((f"opsi {kind}", f"opsi 1 {kind}" if kind in OPSI_ROWS else "opsi 0"))
        out.append((f"closed {kind}", f"closed 1 {CLOSED[kind]}" if kind in CLOSED else "closed 0"))
    for v in range(-1, 9):
        out.append((f"variant {v}", f"variant 1 {FORCE[v]}" if v in FORCE else "variant 0"))
    for d in range(1, 41):                                                   # the prep kernels: the first tier that holds d
        tier = next((eplp for dmax, eplp in PREP if d <= dmax), None)
        out.append((f"prep {d}", f"prep 0" if tier is None else f"prep 1 {tier}"))
    return out


# ---- decide_route ----
def _facts(kind, d, N, smax, tiles, K=4, Nmp=None, **over):
    """the facts of a set of `kind` on a generated table, as gvi_factors_add and upload_table leave them"""
    sumsq = kind in (QUAD, FIXED)
    f = dict(kind=kind, d=d, m=(d // 2 if kind == QUAD else d if kind == FIXED else 0), K=K, all_pos=1, arm=1, sdf=1,
             ndof=7 if kind == ARM else 0, rows=OPSI_ROWS.get(kind, 3), Np=_ceil(N, 256) * 256,
             Nmp=(_ceil(N - N // 2, 64) * 64 if d <= 12 else 0) if Nmp is None else Nmp, p=3,
             coded=int(d >= 16 and d % 4 == 0), Zq=int(d <= 12), orb=1, smax=smax, tiles=tiles)
    assert sumsq or f["m"] == 0
    f.update(over)
    return f


def _line(cmd, **kv):
    return cmd + " " + " ".join(f"{k}={int(v)}" for k, v in kv.items())


def _want_route(route, K, nchunk, chunk, Nmp, pipe=0):
    gx = {"Split": K, "Generic": K, "Scost": _ceil(K, 8)}.get(route, _ceil(K, 4))
    mchunk = _ceil(Nmp // 64, nchunk) * 64 if Nmp else 0
    return f"route 0 {route} {nchunk} {chunk} {mchunk} {gx} {nchunk} {pipe} | "


# one row per compiled instance, as tests/test_factor_routes_gpu.py has them: (kind, d, points of the table, largest support, tiles)
ROWS = ([(k, d, 64 * d + 1, 2, 3) for k in (RANGE, H2D, BODY, H3D, SEG2, SEG3, QUAD, FIXED) for d in REG[k] if d > 1] +
        [(RANGE, 1, 5, 1, 1), (FIXED, 1, 5, 1, 1)] +
        [(k, d, 2 * d * d + 2 * d + 1, 2, 1 + d // 8) for k in (QUAD, FIXED) for d in SPLIT_D] +
        [(QUAD, 4, 201, 4, 2), (FIXED, 6, 1073, 4, 4), (FIXED, 6, 2561, 5, 6), (FIXED, 12, 17217, 4, 40), (FIXED, 12, 80000, 5, 120),
         (QUAD, 28, 1625, 2, 8)] +
        [(RANGE, 1, 9, 1, 1), (H2D, 4, 137, 3, 2), (BODY, 3, 69, 3, 1), (H3D, 3, 69, 3, 1), (ARM, 7, 113, 2, 1)])


def _route_cases():
    out = []
    for (kind, d, N, smax, tiles), variant, orbit_on in itertools.product(ROWS, VARIANTS, (1, 0)):
        f = _facts(kind, d, N, smax, tiles)
        Z = Table(N, smax, tiles)
        nchunk_full = None
        for full in (1, 0):
            route = _route(kind, d, f["m"] or d, Z, variant, bool(orbit_on), bool(full))
            cmd = _line("route", variant=variant, full=full, orbit=orbit_on, **f)
            if route is None:
                out.append((cmd, f"route {ERR_UNSUPPORTED} Empty 1 {f['Np']} 0 0 1 0 | {MSG_REG}"))
                continue
            nchunk, chunk = _chunks(route, f["K"], Z, nchunk_full)
            if full:
                nchunk_full = nchunk
            pipe = int(route == "sreg" and (kind, d) != (FIXED, 12))
            out.append((cmd, _want_route(NAME[route], f["K"], nchunk, chunk, f["Nmp"], pipe)))
    return out


def _chunk_cases():
    """K, Np and tiles crossed, per chunking rule; default options against _chunks, other values against the rule written out"""
    out = []
    legs = [("orbit", FIXED, 6, 0), ("sreg", QUAD, 12, 5), ("reg", FIXED, 4, 0), ("split", FIXED, 16, 0), ("generic", FIXED, 6, 1)]
    for (route, kind, d, variant), K, Np, tiles, Nmp in itertools.product(legs, (1, 3, 257, 5000), (256, 1792, 65536), (1, 5, 40), (0, 128, 1024)):
        if route != "orbit" and tiles != 1:
            continue                                                     # only the orbit rule reads the tile count
        f = _facts(kind, d, Np, 3, tiles, K=K, Nmp=Nmp)
        Z = Table(Np, 3, tiles)
        full = _chunks(route, K, Z)
        out.append((_line("route", variant=variant, full=1, **f), _want_route(NAME[route], K, *full, Nmp, int(route == "sreg"))))
        if route == "sreg":                                              # its cost pass: the two-factor kernel, eight times finer
            out.append((_line("route", variant=variant, full=0, **f), _want_route("Scost", K, *_chunks("scost", K, Z, full[0]), Nmp)))
            out.append((_line("route", variant=variant, full=0, no_scost=1, **f), _want_route("Sreg", K, *full, Nmp, 1)))
        tw, ow, omt = 512, 1000, 2
        iters = Np // 256
        if route == "orbit":
            want = (min(tiles, max(1, _ceil(ow, K)), max(1, tiles // omt)), Np)
        elif route in ("sreg", "reg"):
            nch = min(max(1, _ceil(tw, K)), iters)
            want = (_ceil(Np, _ceil(iters, nch) * 256), _ceil(iters, nch) * 256)
        else:
            want = full                                                  # split and generic kernels read none of the three
        out.append((_line("route", variant=variant, full=1, tw=tw, ow=ow, omt=omt, **f),
                    _want_route(NAME[route], K, *want, Nmp, int(route == "sreg"))))
    return out


def _pipe_cases():
    out = []
    for (kind, d, pipelined), Zq, sreg_pipe in itertools.product([(QUAD, 4, 1), (QUAD, 8, 1), (QUAD, 12, 1), (FIXED, 6, 1), (FIXED, 12, 0)], (0, 1), (0, 1)):
        f = _facts(kind, d, 1000, 2, 3, Zq=Zq)
        nchunk, chunk = _chunks("sreg", 4, Table(1000, 2, 3))
        out.append((_line("route", variant=5, full=1, sreg_pipe=sreg_pipe, **f),
                    _want_route("Sreg", 4, nchunk, chunk, f["Nmp"], int(pipelined and Zq and sreg_pipe))))
    return out


def _refusal_cases():
    hinge = _facts(H2D, 8, 500, 2, 3)
    arm = _facts(ARM, 7, 113, 2, 1)
    empty = _facts(FIXED, 6, 1073, 4, 4, K=0)
    return [
        (_line("route", variant=0, **dict(hinge, sdf=0)), f"route {ERR_STATE} Empty 1 512 0 0 1 0 | {MSG_SDF}"),
        (_line("route", variant=2, full=1, **hinge), f"route {ERR_UNSUPPORTED} Empty 1 512 0 0 1 0 | {MSG_REG}"),
        (_line("route", variant=2, full=0, **hinge), f"route {ERR_UNSUPPORTED} Empty 1 512 0 0 1 0 | {MSG_REG}"),
        (_line("route", variant=0, **dict(arm, arm=0)), f"route {ERR_STATE} Empty 1 256 0 0 1 0 | {MSG_ARM}"),
        (_line("route", variant=0, **dict(arm, arm=0, sdf=0)), f"route {ERR_STATE} Empty 1 256 0 0 1 0 | {MSG_ARM}"),   # the arm model is asked for first
        (_line("route", variant=0, **dict(hinge, sdf=0, psi_ext=1)), _want_route("Generic", 4, *_chunks("generic", 4, Table(500, 2, 3)), hinge["Nmp"])),
    ] + [(_line("route", variant=v, full=full, **empty), "route 0 Empty 1 1280 0 0 1 0 | ") for v in VARIANTS for full in (0, 1)]


def _d_gt_32_cases():
    out = []
    for d in (32, 33):
        f = _facts(FIXED, d, 2 * d * d + 2 * d + 1, 2, 40)
        nchunk, chunk = _chunks("generic", 4, Table(2 * d * d + 2 * d + 1, 2, 40))
        ok = _want_route("Generic", 4, nchunk, chunk, 0)
        out.append((_line("route", variant=1, **f), ok if d == 32 else
                    ok.replace("route 0", f"route {ERR_UNSUPPORTED}").replace(" | ", " | generic kernel supports d <= 32")))
        hs = _facts(HALFSPACE, d, 2 * d * d + 2 * d + 1, 2, 40, closed=1, J=3)
        want = f"route 0 Closed 1 {hs['Np']} 0 4 1 0 | "
        out.append((_line("route", variant=0, **hs), want if d == 32 else
                    want.replace("route 0", f"route {ERR_UNSUPPORTED}").replace(" | ", " | closed-form HINGE_HALFSPACE kernel supports d <= 32")))
    return out


# ---- decide_fuse / decide_full: the legs of test_resident_fusing as facts ----
def _sets(*facts):
    return " ; " + " ; ".join(" ".join(f"{k}={int(v)}" for k, v in f.items()) for f in facts)


def _chain(n, **over1):
    """binary priors d = 2n on T - 1 = 4 factors + unary factors d = n on 5, tables of degree 3 (supports <= 2)"""
    return (_facts(QUAD, 2 * n, 8 * n * n + 4 * n + 1, 2, 2 + n // 2, K=4), dict(_facts(FIXED, n, 2 * n * n + 2 * n + 1, 2, 1 + n // 4, K=5), **over1))


def _planar(N_obstacle):
    """d = 8 priors + d = 4 hinge-on-SDF obstacle factors + d = 4 anchors; N_obstacle points in the obstacle set's table"""
    return (_facts(QUAD, 8, 145, 2, 2, K=4), _facts(H2D, 4, N_obstacle, 3, 2, K=5), _facts(FIXED, 4, 41, 2, 1, K=2))


def _fuse_cases():
    n6, n14, planar4, planar8 = _chain(6), _chain(14), _planar(1000), _planar(2000)
    cases = [
        # (rules and pass, sets, cost launch, full launch, full pass)
        ({}, n6, "OrbitPair", "OrbitPair", "Fused"),
        ({}, _chain(2), "OrbitPair", "OrbitPair", "Fused"),
        ({}, n14, "None", "None", "Separate"),                                       # no pair instance at m = 14
        ({}, _chain(6, all_pos=0), "None", "None", "Separate"),                      # an indefinite unary weight
        (dict(orbit=0), n6, "ScostPair", "SregPair", "Separate"),
        (dict(orbit=0, no_scost=1), n6, "None", "SregPair", "Separate"),
        (dict(orbit=0, pair_fuse=0), n6, "None", "None", "Separate"),
        (dict(orbit=0, sreg_pipe=0), n6, "ScostPair", "SregPair", "Separate"),
        (dict(fused=0), n6, "OrbitPair", "OrbitPair", "Separate"),
        (dict(pair_fuse=0), n6, "None", "None", "Separate"),
        (dict(profile_all=1), n6, "None", "None", "Separate"),
        (dict(ngd=0), n6, "OrbitPair", "OrbitPair", "Separate"),                     # the JKO rule
        (dict(chol_sqrt=0), n6, "OrbitPair", "OrbitPair", "Separate"),               # symmetric-root products
        ({}, tuple(dict(f, p=2) for f in n6), "OrbitPair", "OrbitPair", "Separate"),     # degree 2: no Cholesky route
        ({}, (n6[0], dict(n6[1], resident=1)), "OrbitPair", "OrbitPair", "Separate"),    # products of the slot resident
        ({}, (dict(n6[0], K=2), dict(n6[1], K=7)), "OrbitPair", "OrbitPair", "Separate"),   # 1 + ceil(7 / 2) = 5 items per block > 4
        ({}, (dict(n6[0], K=2), dict(n6[1], K=6)), "OrbitPair", "OrbitPair", "Fused"),
        ({}, (n6[1],), "None", "None", "Separate"),                                  # one unary set: key (6, ., 6, 3) has no instance
        ({}, (n6[0],), "None", "None", "Fused"),                                     # one prior set: the chain pattern's key
        ({}, planar4, "Planar3", "Planar3", "Block3"),                               # 1000 points: 4 chunks per factor
        ({}, planar8, "Planar3", "Planar3", "Separate"),                             # 2000 points: 8 chunks
        (dict(pair_fuse=0), planar4, "None", "None", "Separate"),
        (dict(fused=0), planar4, "Planar3", "Planar3", "Separate"),
        (dict(profile_all=1), planar4, "None", "None", "Separate"),
        (dict(ngd=0), planar4, "Planar3", "Planar3", "Separate"),
        (dict(variant=7), planar4, "None", "None", "Separate"),                      # the obstacle set on the sign-orbit kernel
        (dict(variant=5), planar4, "None", "None", "Separate"),
        ({}, (planar4[0], planar4[1], dict(planar4[2], resident=1)), "Planar3", "Planar3", "Separate"),
        ({}, (planar4[0], planar4[1], dict(planar4[2], K=0)), "None", "None", "Separate"),    # an empty shard
        ({}, (planar4[0], planar4[1], dict(planar4[2], closed=1)), "None", "None", "Separate"),
        ({}, (planar4[1], planar4[0], planar4[2]), "None", "None", "Separate"),      # another order of the sets
    ]
    out = []
    for rules, sets, cost, full, fullpass in cases:
        out.append((_line("fuse", full=0, **rules) + _sets(*sets), f"fuse {cost}"))
        out.append((_line("fuse", full=1, **rules) + _sets(*sets), f"fuse {full}"))
        out.append((_line("full", **rules) + _sets(*sets), f"full {fullpass}"))
    return out


def _geometry_cases():
    out = []
    for (i, route), fused, closed in itertools.product(enumerate(ROUTES), (0, 1), (0, 1)):
        code = (0 if closed else 7 if route == "OrbitPsi" else 6 if route == "Orbit" else 5 if fused else
                2 if route in ("Sreg", "Scost", "Reg") else 3 if route == "Split" else 1)
        out.append((f"geo {i} {fused} {closed}", f"geo {code}"))
    return out


GROUPS = {"lists": _list_cases, "routes": _route_cases, "chunks": _chunk_cases, "pipe": _pipe_cases, "refusals": _refusal_cases,
          "d_gt_32": _d_gt_32_cases, "fuse": _fuse_cases, "geometry": _geometry_cases}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("routes_" + request.param)
    exe = str(tmp / "routes_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return tmp, exe


@pytest.mark.parametrize("group", list(GROUPS))
def test_decisions(program, group):
    tmp, exe = program
    cases = GROUPS[group]()
    script = tmp / (group + ".txt")
    script.write_text("\n".join(c for c, _ in cases) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases), r.stdout[-2000:]
    wrong = [(c, want, got) for (c, want), got in zip(cases, lines) if got != want]
    print(f"    {group}: {len(cases)} decisions")
    assert not wrong, wrong[:5]


def test_the_cases_cover_what_they_claim():
    lists = dict(_list_cases())
    # instances of a list: distinct first two arguments that hit ((kind, d) whatever m, (d, m), (m, support), the kind)
    hits = lambda name: len({tuple(k.split()[1:3]) for k, v in lists.items() if k.startswith(name + " ") and v.startswith(name + " 1")})
    assert hits("reg") == 24 + len(REG_BOX) and sum(len(v) for v in REG.values()) == 24
    assert (hits("sreg"), hits("scost"), hits("split"), hits("opsi"), hits("closed")) == (5, 2, 6, 5, 4)
    assert sum(v == "sreg 1 12 12 0" for v in lists.values()) == 1 and sum(v.startswith("sreg 1") and v.endswith(" 1") for v in lists.values()) == 4
    assert {v for k, v in lists.items() if k.startswith("orbit ") and v != "orbit 0"} == {"orbit 1 " + v for v in ORBIT.values()}
    assert {v for k, v in lists.items() if k.startswith("fused ") and v != "fused 0"} == {"fused 1 " + v for v in FUSED.values()}
    assert hits("fused") == 4 + 2 + 4                                        # (6, 1..4), (6, 5..6), (2, 1..4)
    # the prep tiers at their edges, written out: d = 1, 8 | 9, 16 | 17, 32 hit 1 | 4 | 16 elements per lane, d = 33 misses
    assert [lists[f"prep {d}"] for d in (1, 8, 9, 16, 17, 32, 33)] == ["prep 1 1", "prep 1 1", "prep 1 4", "prep 1 4", "prep 1 16", "prep 1 16", "prep 0"]
    routes = [want.split()[2] for _, want in _route_cases() if want.startswith("route 0")]
    assert set(routes) == set(NAME.values())                                 # every route but Empty and Closed, which have cases of their own
    assert len(_route_cases()) == len(ROWS) * len(VARIANTS) * 2 * 2
    assert len(_geometry_cases()) == 9 * 2 * 2
