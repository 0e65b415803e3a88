"""The moving-ball obstacle kinds (GVI_PSI_HINGE_BALLS_2D = 13 / _3D = 14) on the CPU, through a
stand-alone program (tests/stubs/balls_check.cpp) built plain and under AddressSanitizer / UndefinedBehaviorSanitizer: the
rows of the kind table (layouts, every refusal with its exact text, flags, the hole at 12) and psi / clearance of
gaussianvi_amd/csrc/balls_psi.hpp against the numpy reference of tests/balls_ref.py.

Bound of the arithmetic: 1e-13, max-norm relative over the states of a case (rel of tests/test_gpu_parity.py).  Both sides are
float64 sums of at most d + P + 1 rounded terms per check point and at most 8 check points; the hinge's difference
eps + r - sd loses digits only next to the boundary, where psi itself is small against the largest psi of the case."""
import os
import subprocess

import numpy as np
import pytest

import balls_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "balls_check.cpp")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
OK, ERR_ARG = 0, 1
B2, B3 = 13, 14
INF = float("inf")

MSG_LAYOUT = ("HINGE_BALLS_* needs params_per_factor = 3 + J (P (d + 1) + 1) + 8 (2 P + 1) with 1 <= J <= 8 check points "
              "(P = 2 for _2D, 3 for _3D)")
MSG_NAN = "HINGE_BALLS: NaN in the parameter block"
MSG_SIGMA = "HINGE_BALLS: sigma must be finite and >= 0"
MSG_EPS = "HINGE_BALLS: eps and r must be finite"
MSG_W = "HINGE_BALLS: W, c and tau must be finite"
MSG_R = "HINGE_BALLS: a radius is finite and >= 0, or -inf for an empty slot"
MSG_BALL = "HINGE_BALLS: a ball needs a finite centre and velocity"


def size(P, d, J):
    return 3 + J * (P * (d + 1) + 1) + 8 * (2 * P + 1)


# (kind, d, params_per_factor) -> (status, m, J, need, message)
LAYOUTS = [
    ((B2, 2, size(2, 2, 1)), (OK, 0, 1, 3 + 7 + 40, "")),
    ((B2, 4, size(2, 4, 3)), (OK, 0, 3, 3 + 33 + 40, "")),
    ((B2, 8, size(2, 8, 8)), (OK, 0, 8, 3 + 8 * 19 + 40, "")),
    ((B2, 8, size(2, 8, 9)), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),           # J = 9
    ((B2, 8, size(2, 8, 0)), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),           # J = 0
    ((B2, 4, size(2, 4, 3) + 1), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),       # one double long
    ((B2, 4, size(2, 4, 3) - 1), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),       # one double short
    ((B2, 4, 3), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),
    ((B2, 4, 0), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),
    ((B3, 3, size(3, 3, 1)), (OK, 0, 1, 3 + 13 + 56, "")),
    ((B3, 12, size(3, 12, 8)), (OK, 0, 8, 3 + 8 * 40 + 56, "")),
    ((B3, 6, size(2, 6, 2)), (ERR_ARG, 0, 0, 0, MSG_LAYOUT)),           # a 2-D block handed to the 3-D kind: 3 + 2 * 15 + 40 = 73, and 73 - 59 = 14 is no multiple of 22
    ((12, 2, 3), (ERR_ARG, 0, 0, 0, "unknown psi kind")),               # the hole stays a hole
    ((15, 2, 3), (ERR_ARG, 0, 0, 0, "unknown psi kind")),
]


def block(P, d, J, sigma=2.0, eps=0.1, r=0.05, balls=((0.0, 1.0),), edit=None):
    """One valid block as a list: W = [I 0] + 0.01, c = 0.02, tau_j = 0.1 j; balls = (first centre coordinate, radius) of the
    leading slots, velocity 0.5, the other slots empty.  edit(b) changes entries in place."""
    W = np.zeros((J, P, d)) + 0.01
    W[:, :, :P] += np.eye(P)
    pts = np.concatenate([W.reshape(J, -1), np.full((J, P), 0.02), 0.1 * np.arange(J)[:, None]], axis=1)
    slots = np.zeros((8, 2 * P + 1))
    slots[:, 2 * P] = -INF
    for m, (x0, R) in enumerate(balls):
        slots[m] = [x0] * P + [0.5] * P + [R]
    b = np.concatenate([[sigma, eps, r], pts.reshape(-1), slots.reshape(-1)])
    assert b.size == size(P, d, J)
    if edit:
        edit(b)
    return b


def at(b, i, v):
    b[i] = v


def slot0(P, d, J):
    return 3 + J * (P * (d + 1) + 1)


S2 = slot0(2, 4, 2)                      # first slot of the 2-D blocks below: o (2) | v (2) | R
# (kind, P, d, J, K blocks) -> (status, message).  Two-factor cases carry the offending value in the SECOND block.
PARAMS = [
    ((B2, 2, 4, 2, [block(2, 4, 2)]), (OK, "")),
    ((B3, 3, 6, 1, [block(3, 6, 1, balls=[(0.0, 1.0)] * 8)]), (OK, "")),
    ((B2, 2, 4, 2, [block(2, 4, 2, balls=())]), (OK, "")),                                                     # every slot empty
    ((B2, 2, 4, 2, [block(2, 4, 2, balls=[(0.0, 0.0)])]), (OK, "")),                                           # R = 0: a point obstacle
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, 7, float("nan")))]), (ERR_ARG, MSG_NAN)),
    ((B2, 2, 4, 2, [block(2, 4, 2), block(2, 4, 2, edit=lambda b: at(b, b.size - 2, float("nan")))]), (ERR_ARG, MSG_NAN)),   # in an EMPTY slot
    ((B2, 2, 4, 2, [block(2, 4, 2, sigma=-1.0)]), (ERR_ARG, MSG_SIGMA)),
    ((B2, 2, 4, 2, [block(2, 4, 2, sigma=INF)]), (ERR_ARG, MSG_SIGMA)),
    ((B2, 2, 4, 2, [block(2, 4, 2, sigma=0.0)]), (OK, "")),
    ((B2, 2, 4, 2, [block(2, 4, 2, eps=INF)]), (ERR_ARG, MSG_EPS)),
    ((B2, 2, 4, 2, [block(2, 4, 2, r=-INF)]), (ERR_ARG, MSG_EPS)),
    ((B2, 2, 4, 2, [block(2, 4, 2, eps=-0.5, r=-0.1)]), (OK, "")),                                             # finite is all that is asked
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, 3, INF))]), (ERR_ARG, MSG_W)),                         # W
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, 3 + 8, -INF))]), (ERR_ARG, MSG_W)),                    # c
    ((B2, 2, 4, 2, [block(2, 4, 2), block(2, 4, 2, edit=lambda b: at(b, 3 + 2 * 11 - 1, INF))]), (ERR_ARG, MSG_W)),   # tau of the last check point
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, S2 + 4, -1.0))]), (ERR_ARG, MSG_R)),
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, S2 + 4, INF))]), (ERR_ARG, MSG_R)),
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, S2 + 0, INF))]), (ERR_ARG, MSG_BALL)),                 # centre of a live slot
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: at(b, S2 + 3, -INF))]), (ERR_ARG, MSG_BALL)),                # velocity of a live slot
    ((B2, 2, 4, 2, [block(2, 4, 2, edit=lambda b: (at(b, S2 + 5, INF), at(b, S2 + 8, -INF)))]), (OK, "")),     # an empty slot may hold +-inf
    ((B3, 3, 3, 1, [block(3, 3, 1, edit=lambda b: at(b, b.size - 1, -0.5))]), (ERR_ARG, MSG_R)),               # the last slot of a 3-D block
]

FLAGS = {B2: {"raw", "clearance"}, B3: {"raw", "clearance"}, 12: set(), 15: set(), -1: set(), 8: {"raw", "sdf2d", "sdf", "clearance"}}


def eval_cases():
    """name -> (P, d, J, block [size], X [N][d]) of the arithmetic check: P = 2 and 3, J = 1 and 8, 0 / 1 / 8 active balls,
    a check point exactly on a centre, R = 0, every slot empty, an empty slot that holds +-inf."""
    rng = np.random.default_rng(1317)
    out = {}
    for P, d in ((2, 4), (3, 6)):
        for J in (1, 8):
            for M in (0, 1, 8):
                W = 0.05 * rng.normal(size=(J, P, d))
                W[:, :, :P] += np.eye(P)
                pts = np.concatenate([W.reshape(J, -1), 0.1 * rng.normal(size=(J, P)), rng.uniform(-0.3, 0.3, (J, 1))], axis=1)
                slots = np.zeros((8, 2 * P + 1))
                slots[:, 2 * P] = -INF
                live = rng.permutation(8)[:M]                          # live slots in any position
                slots[live, :P] = rng.uniform(-1.5, 1.5, (M, P))
                slots[live, P:2 * P] = rng.uniform(-1.0, 1.0, (M, P))
                slots[live, 2 * P] = rng.uniform(0.2, 0.9, M)
                if M == 8:
                    slots[live[0], 2 * P] = 0.0                        # a point obstacle among the eight
                dead = np.setdiff1d(np.arange(8), live)
                if dead.size:
                    slots[dead[0], 0], slots[dead[0], P] = INF, -INF   # what an empty slot may hold
                b = np.concatenate([[rng.uniform(2, 20), rng.uniform(0.1, 0.3), rng.uniform(0.05, 0.2)], pts.reshape(-1), slots.reshape(-1)])
                X = rng.uniform(-2.0, 2.0, (64, d))
                if M:
                    X[:32, :P] = slots[live[0], :P] + rng.normal(0.0, 0.6, (32, P))     # half of the states around a ball
                out[f"P{P}-J{J}-M{M}"] = (P, d, J, b, X)
        # a check point exactly on a centre: W = [I 0], c = 0, x[:P] = o_0 + tau v_0, every product exact in binary
        J = 1
        W = np.zeros((J, P, d))
        W[0, :, :P] = np.eye(P)
        slots = np.zeros((8, 2 * P + 1))
        slots[:, 2 * P] = -INF
        slots[3] = [0.5] * P + [0.25] * P + [0.75]
        b = np.concatenate([[4.0, 0.25, 0.125], W.reshape(-1), np.zeros(P), [2.0], slots.reshape(-1)])
        X = rng.uniform(-2.0, 2.0, (4, d))
        X[0, :P] = 1.0                                                 # 0.5 + 2 * 0.25
        out[f"P{P}-on-centre"] = (P, d, J, b, X)
    return out


EVAL = eval_cases()


def fmt(values):
    return " ".join(repr(float(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module", params=sorted(BUILDS))
def answers(request, tmp_path_factory):
    """every command of this module through one run of the program -> the answer lines, by command line"""
    tmp = tmp_path_factory.mktemp("balls_" + request.param)
    exe = str(tmp / "balls_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmds = ["layout %d %d %d" % c for c, _ in LAYOUTS]
    cmds += ["params %d %d %d %d %s" % (kind, d, size(P, d, J), len(blocks), fmt(np.concatenate(blocks))) for (kind, P, d, J, blocks), _ in PARAMS]
    cmds += ["flags %d" % k for k in FLAGS]
    cmds += ["numbers"]
    cmds += ["eval %d %d %d %d %s %s" % (P, d, J, len(X), fmt(b), fmt(X)) for P, d, J, b, X in EVAL.values()]
    script = tmp / "commands.txt"
    script.write_text("\n".join(cmds) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cmds), r.stdout[-2000:]
    return dict(zip(cmds, lines)), cmds


def test_the_kinds_have_the_numbers_of_the_header(answers):
    text = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    for name, value in [("GVI_PSI_HINGE_BALLS_2D", 13), ("GVI_PSI_HINGE_BALLS_3D", 14), ("GVI_BALLS_MAX_M", 8)]:
        assert f"{name} = {value}" in text, name
    assert "= 12" not in text.split("GVI_PSI_HINGE_HALFSPACE = 11")[1].split("};")[0]           # no kind took the hole
    assert answers[0]["numbers"] == "numbers 13 14 8 8 15"
    from gaussianvi_amd import api, synthetic
    assert (api.PSI_HINGE_BALLS_2D, api.PSI_HINGE_BALLS_3D) == (13, 14) == (synthetic.PSI_HINGE_BALLS_2D, synthetic.PSI_HINGE_BALLS_3D)


@pytest.mark.parametrize("case", range(len(LAYOUTS)), ids=["%d-d%d-ppf%d" % c for c, _ in LAYOUTS])
def test_layout(answers, case):
    (kind, d, ppf), (status, m, J, need, msg) = LAYOUTS[case]
    got = answers[0]["layout %d %d %d" % (kind, d, ppf)]
    head, _, text = got.partition(" | ")
    assert head.split()[0] == "layout" and int(head.split()[1]) == status, got
    assert text == msg, got
    if status == OK:
        assert [int(v) for v in head.split()[2:]] == [m, J, need], got


@pytest.mark.parametrize("case", range(len(PARAMS)))
def test_parameter_values(answers, case):
    by_cmd, cmds = answers
    status, msg = PARAMS[case][1]
    got = by_cmd[cmds[len(LAYOUTS) + case]]
    assert got == "params %d | %s" % (status, msg)


def test_flags(answers):
    for kind, want in FLAGS.items():
        got = answers[0]["flags %d" % kind].split()
        assert got[:2] == ["flags", str(kind)] and set(got[2:]) == want, (kind, got)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", sorted(EVAL))
def test_psi_and_clearance_against_the_reference(answers, name):
    by_cmd, cmds = answers
    P, d, J, b, X = EVAL[name]
    line = by_cmd[cmds[len(LAYOUTS) + len(PARAMS) + len(FLAGS) + 1 + list(EVAL).index(name)]]
    assert line.startswith("eval ") and "bad-command" not in line, line[:200]
    got = np.array([float(t) for t in line.split()[1:]]).reshape(len(X), 2)
    psi = br.psi(b[None, :], P, d, X[None, :, :])[0]
    clr = br.clearance(b[None, :], P, d, X[None, :, :])[0]
    empty = name.endswith("M0")
    if empty:
        assert (got[:, 0] == 0.0).all() and (psi == 0.0).all() and (got[:, 1] == INF).all() and (clr == INF).all()
        return
    share = float((psi > 0).mean())
    print(f"{name}: share of states with psi > 0 {share:.2f}, psi max {psi.max():.3g}; psi {rel(got[:, 0], psi):.2e}, clearance {rel(got[:, 1], clr):.2e}")
    assert np.isfinite(got).all() and psi.max() > 0
    assert rel(got[:, 0], psi) <= 1e-13 and rel(got[:, 1], clr) <= 1e-13
    if name.endswith("on-centre"):
        # distance 0: sd = -R exactly, psi = sigma (eps + r + R)^2, clearance = -R - r
        assert got[0, 0] == 4.0 * (0.25 + 0.125 + 0.75) ** 2 and got[0, 1] == -0.75 - 0.125
    elif not name.endswith("M1"):
        assert 0.0 < share < 1.0, "both hinge branches"


def test_builders():
    """synthetic.balls_params pads to eight slots; add_moving_obstacle_set gives factor i the balls where they are at t_i."""
    from gaussianvi_amd import synthetic as syn
    W = np.zeros((2, 2, 4))
    W[:, :, :2] = np.eye(2)
    p = syn.balls_params([1.0, 2.0, 3.0], 0.2, 0.1, W, np.zeros((2, 2)), [0.0, 0.5], [[1.0, 2.0], [3.0, 4.0]], [[0.5, 0.0], [0.0, -0.5]], [0.3, 0.0])
    assert p.shape == (3, size(2, 4, 2))
    u = br.unpack(p, 2, 4)
    assert np.array_equal(u["sigma"], [1.0, 2.0, 3.0]) and np.array_equal(u["tau"], [[0.0, 0.5]] * 3) and np.array_equal(u["W"][1], W)
    assert np.array_equal(u["R"], [[0.3, 0.0] + [-INF] * 6] * 3) and np.array_equal(u["o"][2, :2], [[1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(u["v"][0, 1], [0.0, -0.5]) and (u["o"][:, 2:] == 0).all() and (u["v"][:, 2:] == 0).all()
    assert syn.balls_params(1.0, 0.2, 0.1, W, np.zeros((2, 2)), [0.0, 0.5], np.zeros((0, 2)), np.zeros((0, 2)), []).shape == (1, size(2, 4, 2))
    base = syn.make_planar_chain(T=9, p=3)
    o0, v = np.array([[0.3, 1.6], [2.0, 2.0]]), np.array([[0.0, -1.6], [0.1, 0.0]])
    one = syn.add_moving_obstacle_set(base, o0, v, [0.5, 0.2], sigma=15.0, eps=0.2, r=0.1, p=3)["specs"][-1]
    assert (one["kind"], one["d"], len(one["start"])) == (syn.PSI_HINGE_BALLS_2D, 4, 9) and len(base["specs"]) == 3
    u = br.unpack(one["params"], 2, 4)
    assert np.array_equal(u["o"][4, :2], o0 + 1.0 * v) and np.array_equal(u["v"][4, :2], v) and (u["tau"] == 0).all()
    taus = [0.0625, 0.125]
    two = syn.add_moving_obstacle_set(base, o0, v, [0.5, 0.2], taus=taus, dt=0.25)["specs"][-1]
    assert (two["d"], len(two["start"])) == (8, 8)
    u = br.unpack(two["params"], 2, 8)
    Wr, _ = syn.minacc_segment_readout(2, syn.QC, 0.25, taus, 2)
    assert np.array_equal(u["W"][3], Wr) and np.array_equal(u["tau"][3], taus) and np.array_equal(u["o"][3, :2], o0 + 0.75 * v)
    three = syn.add_moving_obstacle_set(syn.make_obstacle_chain("pr3d", T=5), [[0.0, 0.0, 1.0]], [[0.0, 0.0, -1.0]], [0.4])["specs"][-1]
    assert three["kind"] == syn.PSI_HINGE_BALLS_3D and three["params"].shape == (5, size(3, 6, 1))


def test_callsite_compiles_against_the_shim(tmp_path):
    from gaussianvi_amd import build
    build.build_lib()
    exe = str(tmp_path / "balls_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "balls_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
