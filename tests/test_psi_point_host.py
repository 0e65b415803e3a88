"""psi_point and hinge_psi_clearance (gaussianvi_amd/csrc/psi_point.hpp) on the CPU: the chain from a psi kind to its psi and
clearance at one state, which the generic moments kernel and the sample-cost kernel run, compiled as a stand-alone program
(tests/stubs/psi_point_on_cpu.cpp) plain and under AddressSanitizer / UndefinedBehaviorSanitizer and run on every PSI_RAW kind
against the oracle's psi_batch_* and the numpy references of the segment, ball and limit kinds.

Grids are 5 rows x 4 columns and 4 x 5 x 3 with a cell of 0.5 (1 / cell is exact, so the device's multiplication and the oracle's
division agree); the queries of every grid case lie inside the grid, on the last node of each axis, on cell boundaries and
beyond every side.  Every buffer of the program is a std::vector of exactly its size.

Bound: 1e-13, max-norm relative over the ~64 states of a case, the bound and the argument of tests/test_balls_host.py: both
sides are float64 sums of a few rounded terms per check point (at most d + P + 1 for a read-out, 4 / 8 weighted corners for a
look-up) and at most 8 check points.  The arm rounds double trigonometry to float, where one libm's last bit moves a sphere by
1e-8 of the arm's length: it gets the 1e-8 that tests/test_sample_cost_gpu.py holds the device to for the grid kinds.

Measured maxima (plain and sanitized builds alike), psi / clearance:
  range_1d, sdf2d, body (4 cases), sdf3d, box: 0 / 0 (the same bits as the reference)
  arm 4.8e-16 / 6.3e-16    seg (3 cases) 2.9e-16 / 4.3e-16    halfspace 1.5e-16 / 2.1e-16    balls (2 cases) 2.4e-16 / 3.0e-16
"""
import os
import subprocess

import numpy as np
import pytest

import balls_ref
import box_ref
import gvi_oracle as o
import halfspace_ref
import segment_ref
from gaussianvi_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "stubs", "psi_point_on_cpu.cpp")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
N = 64
CELL = 0.5
# obstacle: one disc / ball (centre, radius)
GRID2 = dict(origin=(-0.5, -1.0), shape=(5, 4), obstacle=((0.3, 0.1), 0.45))                     # rows x cols: x in [-0.5, 1], y in [-1, 1]
GRID3 = dict(origin=(-1.0, -0.75, -0.25), shape=(4, 5, 3), obstacle=((0.2, 0.1, 0.3), 0.4))      # rows x cols x slices: x in [-1, 1], y in [-0.75, 0.75], z in [-0.25, 0.75]
GRID3_ARM = dict(GRID3, obstacle=((0.4, 0.3, 0.2), 0.3))                                         # off the arm's base, which sits at the origin
BOUND, BOUND_ARM = 1e-13, 1e-8


def field_of(grid):
    rows, cols = grid["shape"][:2]
    centre, radius = grid["obstacle"]
    if len(grid["shape"]) == 2:
        return syn.circle_sdf(grid["origin"], CELL, rows, cols, [centre], [radius])
    return syn.sphere_sdf3d(grid["origin"], CELL, rows, cols, grid["shape"][2], [centre], [radius])


def extent(grid):
    P = len(grid["shape"])
    lo = np.array(grid["origin"], dtype=np.float64)
    nodes = np.array([grid["shape"][1], grid["shape"][0]] + list(grid["shape"][2:]), dtype=np.float64)   # x -> columns, y -> rows
    return P, lo, lo + (nodes - 1.0) * CELL


def queries(rng, grid):
    """[N][P]: inside the grid, on the last node of each axis, on a cell boundary of each axis and of all at once, beyond each
    side of each axis and beyond a corner, the rest around the grid."""
    P, lo, hi = extent(grid)
    q = [rng.uniform(lo, hi, P) for _ in range(32)]
    for a in range(P):
        for v in (hi[a], lo[a], lo[a] + CELL, lo[a] - 0.7, hi[a] + 0.7):
            t = rng.uniform(lo, hi, P)
            t[a] = v
            q.append(t)
    q += [hi.copy(), lo + CELL, lo - 0.3, hi + 0.3]
    while len(q) < N:
        q.append(rng.uniform(lo - 0.3, hi + 0.3, P))
    return np.array(q[:N])


def clearance_from(sd, radii):
    """min over the check points (axis 0) of sd - r"""
    return (sd - np.reshape(radii, (-1, 1))).min(axis=0)


def make_cases():
    """name -> dict(kind, d, J, raw, X [N][d], grid, arm, psi [N], clr [N] or None, hinge, bound)"""
    rng = np.random.default_rng(1063)
    nan = np.full(N, np.nan)
    cases = {}

    def add(name, kind, d, raw, X, psi, clr, J=0, grid=None, arm=None, hinge=True, bound=BOUND):
        cases[name] = dict(kind=kind, d=d, J=J, raw=np.asarray(raw, dtype=np.float64), X=X, grid=grid, arm=arm, psi=psi, clr=clr, hinge=hinge, bound=bound)

    # the kinds without a point psi / without a clearance
    add("quad_prior", syn.PSI_QUAD_PRIOR, 4, [], rng.normal(size=(N, 4)), nan, nan, hinge=False)
    raw = [1.2, 20.0, 40.0, 0.09, 9.0]
    X = rng.uniform(15.0, 45.0, (N, 1))
    add("range_1d", syn.PSI_RANGE_1D, 1, raw, X, o.psi_batch_range_1d(*raw)(X[None])[0], nan, hinge=False)

    f2, f3 = field_of(GRID2), field_of(GRID3)
    g2, g3 = (GRID2["origin"], CELL, f2), (GRID3["origin"], CELL, f3)
    # planar point robot, d = 4: the pose is x[0:2]
    X = rng.normal(size=(N, 4))
    X[:, :2] = queries(rng, GRID2)
    raw = np.array([[7.5, 0.3, 0.15]])
    add("sdf2d", syn.PSI_HINGE_SDF_2D, 4, raw[0], X, o.psi_batch_hinge_sdf2d(raw, *g2)(X[None])[0],
        o.planar_sdf_lookup(X[:, 0], X[:, 1], *g2) - raw[0, 2], grid=GRID2)
    # planar body, 1 and 3 balls, phi zero and not
    for nb in (1, 3):
        for tag in ("phi0", "phi"):
            X = rng.normal(size=(N, 3))
            X[:, :2] = queries(rng, GRID2)
            X[:, 2] = 0.0 if tag == "phi0" else rng.uniform(-3.0, 3.0, N)
            raw = np.array([[6.0, 0.25, 0.2, 1.5, float(nb), 0.8]])
            sig, eps, r, slope, _, L = raw[0]
            lx, lz = X[:, 0] - (L - r * 1.5) * np.cos(X[:, 2]) / 2.0, X[:, 1] - (L - r * 1.5) * np.sin(X[:, 2]) / 2.0
            sd = np.array([o.planar_sdf_lookup(lx + L * np.cos(X[:, 2]) / nb * i, lz + L * np.sin(X[:, 2]) / nb * i, *g2) for i in range(nb)])
            add(f"body-{nb}-{tag}", syn.PSI_HINGE_SDF_2D_BODY, 3, raw[0], X, o.psi_batch_hinge_sdf2d_body(raw, *g2)(X[None])[0],
                clearance_from(sd, [r] * nb), grid=GRID2)
    # 3-D point robot, d = 3
    X = queries(rng, GRID3)
    raw = np.array([[5.0, 0.35, 0.1]])
    add("sdf3d", syn.PSI_HINGE_SDF_3D, 3, raw[0], X, o.psi_batch_hinge_sdf3d(raw, *g3)(X[None])[0],
        o.sdf3d_lookup(X[:, 0], X[:, 1], X[:, 2], *g3) - raw[0, 2], grid=GRID3)
    # the arm of the synthetic graphs at d = 7: spheres 0 .. 6 stay within 0.65 of the base, some below the grid
    arm = syn.wam_like_arm()
    X = rng.uniform(-2.0, 2.0, (N, 7))
    raw = np.array([[4.0, 0.1]])
    ga = (GRID3_ARM["origin"], CELL, field_of(GRID3_ARM))
    pts = o.arm_sphere_centers(X, arm["a"], arm["alpha"], arm["d"], arm["theta_bias"], arm["frames"][:7], arm["centers"][:7])
    sd = np.array([o.sdf3d_lookup(pts[:, i, 0], pts[:, i, 1], pts[:, i, 2], *ga) for i in range(7)])
    add("arm", syn.PSI_HINGE_SDF_3D_ARM, 7, raw[0], X, o.psi_batch_hinge_sdf3d_arm(raw, arm, *ga)(X[None])[0],
        clearance_from(sd, arm["radii"][:7]), grid=GRID3_ARM, arm=arm, bound=BOUND_ARM)
    # segments
    for P, d, J in ((2, 4, 1), (2, 8, 8), (3, 6, 3)):
        grid, g = (GRID2, g2) if P == 2 else (GRID3, g3)
        W = 0.05 * rng.normal(size=(J, P, d))
        W[:, :, :P] += np.eye(P)
        raw = syn.segment_params(6.5, 0.3, 0.12, W, 0.1 * rng.normal(size=(J, P)))
        X = 0.3 * rng.normal(size=(N, d))
        X[:, :P] = queries(rng, grid)
        kind = syn.PSI_HINGE_SDF_2D_SEG if P == 2 else syn.PSI_HINGE_SDF_3D_SEG
        add(f"seg-P{P}-d{d}-J{J}", kind, d, raw[0], X, segment_ref.psi_batch_hinge_seg(raw, P, d, *g)(X[None])[0],
            segment_ref.clearance(raw, P, d, *g, X[None])[0], J=J, grid=grid)
    # the kinds of the plain headers, through the dispatch
    d = 4
    raw = syn.box_params([3.0, 0.0, 2.0, 1.0], 0.1, [-1.0, -np.inf, -0.5, -np.inf], [1.0, np.inf, np.inf, 0.8])
    X = rng.normal(size=(N, d))
    add("box", syn.PSI_HINGE_BOX, d, raw[0], X, box_ref.psi_batch(raw, d)(X[None])[0], box_ref.margin(raw, d, X[None])[0])
    A = rng.normal(size=(3, d))
    raw = syn.halfspace_params([2.0, 0.0, 5.0], 0.1, [0.5, 0.2, 0.8], A)
    add("halfspace", syn.PSI_HINGE_HALFSPACE, d, raw[0], X, halfspace_ref.psi_batch(raw, d)(X[None])[0], halfspace_ref.margin(raw, d, X[None])[0], J=3)
    for P, d, J in ((2, 4, 3), (3, 6, 2)):
        W = 0.05 * rng.normal(size=(J, P, d))
        W[:, :, :P] += np.eye(P)
        cen, vel, rad = rng.uniform(-1.0, 1.0, (3, P)), 0.5 * rng.normal(size=(3, P)), rng.uniform(0.3, 0.7, 3)
        raw = syn.balls_params(9.0, 0.2, 0.1, W, 0.1 * rng.normal(size=(J, P)), np.linspace(0.0, 0.2, J), cen, vel, rad)
        X = rng.uniform(-2.0, 2.0, (N, d))
        kind = syn.PSI_HINGE_BALLS_2D if P == 2 else syn.PSI_HINGE_BALLS_3D
        add(f"balls-P{P}", kind, d, raw[0], X, balls_ref.psi(raw, P, d, X[None])[0], balls_ref.clearance(raw, P, d, X[None])[0], J=J)
    return cases


CASES = make_cases()


def hexes(values):
    return " ".join(float(v).hex() for v in np.ravel(values))


def write_cases(path):
    with open(path, "w") as f:
        f.write(f"{len(CASES)}\n")
        for c in CASES.values():
            f.write(f"{c['kind']} {c['d']} {c['J']} {c['raw'].size} {N}\n")
            if c["grid"] is None:
                f.write("0 0 0 0 0 0 1\n\n")
            else:
                shape, origin = c["grid"]["shape"], c["grid"]["origin"]
                f.write("%d %d %d %s %s\n" % (shape[0], shape[1], shape[2] if len(shape) == 3 else 0,
                                              hexes(list(origin) + [0.0] * (3 - len(origin))), float(CELL).hex()))
                f.write(hexes(np.ravel(field_of(c["grid"]), order="F")) + "\n")            # r + c rows + z rows cols
            arm = c["arm"]
            pk = [] if arm is None else np.concatenate([[len(arm["a"]), len(arm["frames"])], arm["a"], arm["alpha"], arm["d"], arm["theta_bias"],
                                                        arm["frames"], np.ravel(arm["centers"]), arm["radii"]])
            f.write(f"{len(pk)}\n{hexes(pk)}\n{hexes(c['raw'])}\n{hexes(c['X'])}\n")


@pytest.fixture(scope="module", params=sorted(BUILDS))
def answers(request, tmp_path_factory):
    """one run of the program over every case -> {case index: (psi [N], clr [N])}"""
    tmp = tmp_path_factory.mktemp("psi_point_" + request.param)
    exe = str(tmp / "psi_point_on_cpu")
    r = subprocess.run(BUILDS[request.param] + ["-I", CSRC, STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    path = str(tmp / "cases.txt")
    write_cases(path)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines()[:-1]:
        t = ln.split()
        out.setdefault(int(t[1]), {})[t[0]] = np.array([float.fromhex(v) for v in t[2:]])
    assert sorted(out) == list(range(len(CASES)))
    return out


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_cases_cover_every_raw_kind_and_the_grid_edges():
    raw_kinds = {syn.PSI_RANGE_1D, syn.PSI_HINGE_SDF_2D, syn.PSI_HINGE_SDF_2D_BODY, syn.PSI_HINGE_SDF_3D, syn.PSI_HINGE_SDF_3D_ARM,
                 syn.PSI_HINGE_SDF_2D_SEG, syn.PSI_HINGE_SDF_3D_SEG, syn.PSI_HINGE_BOX, syn.PSI_HINGE_HALFSPACE, syn.PSI_HINGE_BALLS_2D,
                 syn.PSI_HINGE_BALLS_3D}
    assert {c["kind"] for c in CASES.values()} == raw_kinds | {syn.PSI_QUAD_PRIOR}
    assert GRID2["shape"] == (5, 4) and GRID3["shape"] == (4, 5, 3) and (1.0 / CELL) * CELL == 1.0 and np.log2(CELL) % 1 == 0
    for grid in (GRID2, GRID3):
        P, lo, hi = extent(grid)
        q = queries(np.random.default_rng(0), grid)
        inside = ((q > lo) & (q < hi)).all(axis=1)
        assert inside.sum() >= 16
        for a in range(P):
            assert (q[:, a] == hi[a]).any() and (q[:, a] < lo[a]).any() and (q[:, a] > hi[a]).any()
            assert (((q[:, a] - lo[a]) / CELL) % 1 == 0)[inside | (q[:, a] == lo[a] + CELL)].any()


@pytest.mark.parametrize("name", list(CASES))
def test_psi_and_clearance_against_the_reference(answers, name):
    c = CASES[name]
    got = answers[list(CASES).index(name)]
    psi, clr = c["psi"], c["clr"]
    if c["hinge"]:
        share = float((psi > 0).mean())                                   # the condition is on the reference alone
        assert 0.05 < share < 0.95, (name, share)
    if np.isnan(psi).all():
        assert np.isnan(got["psi"]).all(), name                           # no point psi for this kind
    else:
        assert np.isfinite(got["psi"]).all() and psi.max() > 0
        e = rel(got["psi"], psi)
        print(f"{name}: psi {e:.2e}")
        assert e <= c["bound"], (name, e)
    if np.isnan(clr).all():
        assert np.isnan(got["clr"]).all(), name                           # no clearance for this kind
    else:
        assert np.isfinite(got["clr"]).all()
        e = rel(got["clr"], clr)
        print(f"{name}: clearance {e:.2e}")
        assert e <= c["bound"], (name, e)
