"""CPU checks of the read-out-space quadrature (gvi_factors_set_readout_rule): the functions the kernel
calls (gaussianvi_amd/csrc/readout_moments.hpp) compiled for the host, plain and under AddressSanitizer / UBSan, against
tests/readout_ref.py with both roots of Sigma; the accuracy claim against the exact moments of a half-plane hinge; the route
decisions with the rule on; the bindings, the builders and the shim call site."""
import math
import os
import subprocess

import numpy as np
import pytest

import balls_ref as br
import gvi_oracle as o
import readout_ref as rr
from gaussianvi_amd import _lib, api, build, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def compile_stub(tmp_path, name, flags):
    exe = str(tmp_path / (name + ("_san" if flags else "")))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "stubs", name + ".cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def sym_root(Sigma):
    lam, V = np.linalg.eigh(Sigma)
    return (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T


# ---- 1. the header on the CPU ----
LEAD, SEG, BALLS = 0, 1, 2                   # READOUT_* of psi_kinds.hpp
KIND_OF = {(LEAD, 2): syn.PSI_HINGE_SDF_2D, (LEAD, 3): syn.PSI_HINGE_SDF_3D, (SEG, 2): syn.PSI_HINGE_SDF_2D_SEG, (SEG, 3): syn.PSI_HINGE_SDF_3D_SEG,
           (BALLS, 2): syn.PSI_HINGE_BALLS_2D, (BALLS, 3): syn.PSI_HINGE_BALLS_3D}


def grid_of(P):
    """a disc / ball of radius 0.7 at the origin on a grid whose cell is a power of two (1 / cell exact)"""
    if P == 2:
        return dict(sdf_origin=(-2.0, -2.0), sdf_cell=0.25, sdf_field=syn.circle_sdf((-2.0, -2.0), 0.25, 17, 17, [(0.0, 0.0)], [0.7]))
    return dict(sdf_origin=(-2.0, -2.0, -2.0), sdf_cell=0.5, sdf_field=syn.sphere_sdf3d((-2.0, -2.0, -2.0), 0.5, 9, 9, 9, [(0.0, 0.0, 0.0)], [0.7]))


def stub_cases():
    """(P, d, J, order, block [1][...], mu [d], Sigma [d][d], tag, cls): BALLS blocks with random read-outs whose means are 0.3
    off a ball's rim, then a zero row of W, two parallel rows, and both together; one LEAD and one SEG case per P on a grid, the
    means 0.3 off the obstacle's rim."""
    rng = np.random.default_rng(18)
    cases = []
    for P, d, J, order in [(2, 2, 1, 7), (2, 4, 3, 8), (2, 8, 8, 16), (2, 12, 3, 2), (3, 3, 1, 4), (3, 6, 3, 5), (3, 12, 8, 10), (2, 32, 3, 9)]:
        for tag in ("random", "zero_row", "parallel", "zero_and_parallel"):
            if tag == "zero_and_parallel" and P == 2:
                continue
            mu, Sigma = syn.random_marginals(rng, 1, d, 0.05)
            W = rng.normal(size=(J, P, d)) / np.sqrt(d) * 2.0
            if tag in ("zero_row", "zero_and_parallel"):
                W[:, P - 1, :] = 0.0                                  # the time stamp as last coordinate
            if tag in ("parallel", "zero_and_parallel"):
                W[:, 1, :] = -0.5 * W[:, 0, :]
            M = 3
            cen, vel, rad = rng.normal(size=(M, P)), 0.5 * rng.normal(size=(M, P)), rng.uniform(0.3, 0.8, M)
            tau = np.linspace(0.05, 0.2, J)
            u = rng.normal(size=(J, P))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            target = (cen[0] + tau[:, None] * vel[0]) + (rad[0] + 0.3) * u
            c = target - W @ mu[0]
            blk = syn.balls_params(rng.uniform(5, 20), 0.2, 0.1, W, c, tau, cen, vel, rad)
            cases.append((P, d, J, order, blk, mu[0], Sigma[0], tag, BALLS))
    rng = np.random.default_rng(1806)                                # the grid classes, after the BALLS cases and on their own stream
    for P, d, J, order in [(2, 4, 1, 8), (3, 6, 1, 5), (2, 8, 3, 8), (3, 6, 3, 5)]:
        cls = LEAD if J == 1 else SEG
        mu, Sigma = syn.random_marginals(rng, 1, d, 0.05)
        u = rng.normal(size=(J, P))
        target = (0.7 + 0.3) * u / np.linalg.norm(u, axis=1, keepdims=True)
        if cls == LEAD:
            mu[0, :P] = target[0]
            blk = np.array([[12.0, 0.3, 0.1]])
        else:
            W = rng.normal(size=(J, P, d)) / np.sqrt(d) * 2.0
            blk = syn.segment_params(12.0, 0.3, 0.1, W, target - W @ mu[0])
        cases.append((P, d, J, order, blk, mu[0], Sigma[0], "random", cls))
    return cases


def write_cases(path, cases, which):
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for P, d, J, order, blk, mu, Sigma, _, cls in cases:
            S = sym_root(Sigma) if which == 0 else np.linalg.cholesky(Sigma)
            if which == 1 and d > 1:
                assert np.abs(S - S.T).max() > 1e-3                      # a root whose rows and columns differ
            x, w = rr.rule(order)
            f.write(f"mom {P} {cls} {d} {J} {order}\n")
            if cls != BALLS:
                g = grid_of(P)
                shape = g["sdf_field"].shape
                f.write("%d %d %d " % (shape[0], shape[1], shape[2] if P == 3 else 0))
                f.write(" ".join(float(v).hex() for v in list(g["sdf_origin"]) + [0.0] * (3 - P) + [g["sdf_cell"]]) + "\n")
                f.write(" ".join(float(v).hex() for v in np.ravel(g["sdf_field"], order="F")) + "\n")     # r + c rows + z rows cols
            f.write("\n".join(" ".join(float(v).hex() for v in np.ravel(a)) for a in (blk, mu, S, x, w)) + "\n")


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "sanitized"])
def test_header_on_cpu(tmp_path, flags):
    """readout_moments.hpp as a stand-alone host program, run on stub_cases() -- the three read-out classes, the grid classes through
    the look-ups of psi_point.hpp -- with the symmetric root of Sigma and with its lower
    Cholesky factor (row-major, x = mu + S z): S m1 and S M2 S^T of the two roots agree with each other and with readout_ref to
    1e-12 (max-norm relative), the bound of the half-space program's test; the result depends on Sigma only."""
    exe = compile_stub(tmp_path, "readout_on_cpu", flags)
    cases = stub_cases()
    assert {c[0] for c in cases} == {2, 3} and {c[7] for c in cases} == {"random", "zero_row", "parallel", "zero_and_parallel"}
    assert {(c[8], c[0]) for c in cases} == set(KIND_OF)                 # every class at every P
    back = {}
    worst = 0.0
    for which in (0, 1):
        path = str(tmp_path / f"cases{which}.txt")
        write_cases(path, cases, which)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("mom")]
        assert len(lines) == len(cases)
        for ci, (P, d, J, order, blk, mu, Sigma, tag, cls) in enumerate(cases):
            t = lines[ci]
            assert int(t[1]) == ci and int(t[2]) == 1
            v = np.array([float.fromhex(s) for s in t[3:]])
            S = sym_root(Sigma) if which == 0 else np.linalg.cholesky(Sigma)
            m0, m1, M2 = v[0], v[1:1 + d], v[1 + d:].reshape(d, d)
            got = dict(E_phi=m0, E_xmuphi=S @ m1, E_xxphi=S @ M2 @ S.T)
            spec = dict(kind=KIND_OF[(cls, P)], d=d, params=blk, temperature=np.ones(1), **({} if cls == BALLS else grid_of(P)))
            diag = []
            ref = rr.spec_moments(spec, mu[None], Sigma[None], order, diag=diag)
            keeps = {tuple(e["keep"]) for e in diag[0]}
            want = {"random": (True,) * P, "zero_row": (True,) * (P - 1) + (False,), "parallel": (True, False) + (True,) * (P - 2),
                    "zero_and_parallel": (True, False, False)}[tag]
            assert keeps == {want}, (tag, keeps)
            assert ref["E_phi"][0] > 0
            for k in got:
                err = relmax(got[k], ref[k][0])
                worst = max(worst, err)
                assert err <= 1e-12, (tag, which, P, d, J, order, k, err)
            back[(which, ci)] = got
    for ci in range(len(cases)):
        for k in ("E_phi", "E_xmuphi", "E_xxphi"):
            assert relmax(back[(1, ci)][k], back[(0, ci)][k]) <= 1e-12, (cases[ci][7], k)
    print(f"host build of readout_moments.hpp against readout_ref: {worst:.2e}")


def test_cholesky_drop_rule_on_cpu(tmp_path):
    """readout_chol on given matrices: a negative pivot, a negative diagonal and a NaN are refused (the factor is NaN); a pivot
    within 64 ulp of C_kk is dropped; L equals the reference's."""
    exe = compile_stub(tmp_path, "readout_on_cpu", SAN)
    rng = np.random.default_rng(3)
    mats = []
    for P in (2, 3):
        B = rng.normal(size=(P, P))
        good = B @ B.T + 0.1 * np.eye(P)
        neg = good.copy()
        neg[P - 1, P - 1] = (np.linalg.cholesky(good)[P - 1, :P - 1] ** 2).sum() - 0.01          # last pivot -0.01
        diag = good.copy(); diag[0, 0] = -1.0
        nan = good.copy(); nan[1, 0] = nan[0, 1] = np.nan
        v = rng.normal(size=P)
        rank1 = np.outer(v, v)
        zero = good.copy(); zero[P - 1, :] = 0.0; zero[:, P - 1] = 0.0
        mats += [("good", good), ("negative_pivot", neg), ("negative_diagonal", diag), ("nan", nan), ("rank1", rank1), ("zero_row", zero), ("zeros", np.zeros((P, P)))]
    path = str(tmp_path / "chol.txt")
    with open(path, "w") as f:
        f.write(f"{len(mats)}\n")
        for _, C in mats:
            f.write(f"chol {len(C)}\n" + " ".join(float(v).hex() for v in C.ravel()) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("chol")]
    for (tag, C), t in zip(mats, lines):
        P = len(C)
        ok, keep = int(t[2]) == 1, np.array([int(v) for v in t[3:3 + P]], dtype=bool)
        L = np.array([float.fromhex(v) for v in t[3 + P:]]).reshape(P, P)
        Lr, kr, okr = rr.chol_drop(C)
        assert ok == okr == (tag not in ("negative_pivot", "negative_diagonal", "nan")), tag
        if ok:
            assert (keep == kr).all() and np.allclose(L, Lr, rtol=1e-13, atol=0), tag
            assert {"good": P, "rank1": 1, "zero_row": P - 1, "zeros": 0}[tag] == keep.sum(), tag
            assert np.allclose(L @ L.T, C, rtol=0, atol=1e-13 * max(np.abs(C).max(), 1e-300))


def test_reference_refuses_an_ill_conditioned_readout():
    """The reference alone asserts cond(C_j) <= 1e4 for every input it hands out."""
    W = np.array([[1.0, 0.0, 0.0], [1.0, 1e-3, 0.0]])
    with pytest.raises(AssertionError):
        rr.check_point(W, np.zeros(2), np.zeros(3), np.eye(3), 4, lambda q: q[:, 0])


# ---- 2. the accuracy claim ----
def Phi(t):
    return 0.5 * math.erfc(-t / math.sqrt(2.0))


def phi(t):
    return math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def exact_hinge_moments(c, s):
    """E[h], E[t h], E[(t^2 - 1) h] of h = max(0, c + s t)^2, t ~ N(0, 1): by Stein's lemma E[t h] = E[h'] and
    E[(t^2 - 1) h] = E[h''], with a = c / s:  E[h] = s^2 ((a^2 + 1) Phi(a) + a phi(a)), E[h'] = 2 s^2 (a Phi(a) + phi(a)),
    E[h''] = 2 s^2 Phi(a)."""
    a = c / s
    return s * s * ((a * a + 1) * Phi(a) + a * phi(a)), 2 * s * s * (a * Phi(a) + phi(a)), 2 * s * s * Phi(a)


@pytest.mark.parametrize("c", [-1.0, 0.0, 0.7, 2.0])
def test_accuracy_against_the_sparse_rule(c):
    """d = 4, psi = max(0, c + v^T z)^2, v = (0.8, -0.5, 0, 0): in each of (E[psi], E[t psi], E[(t^2 - 1) psi]) along v that is not
    exact for both rules, the reference at order 12 is at least 10 times closer to the exact value than the sparse rule
    o.nwspgr(4, 5).  (At c = 0, E[psi] and E[(t^2 - 1) psi] are exact for both by symmetry.)"""
    v = np.array([0.8, -0.5, 0.0, 0.0])
    s = np.linalg.norm(v)
    u = v / s
    exact = np.array(exact_hinge_moments(c, s))
    Z, w = o.nwspgr(4, 5)
    psi = np.maximum(0.0, c + Z @ v) ** 2
    t = Z @ u
    sparse = np.array([(w * psi).sum(), (w * t * psi).sum(), (w * (t * t - 1) * psi).sum()])
    # the read-out q = (z_0, z_1) of dimension 2 with f(q) = max(0, c + 0.8 q_0 - 0.5 q_1)^2
    W = np.eye(2, 4)
    r = rr.moments([[(W, np.zeros(2), lambda q: np.maximum(0.0, c + q @ v[:2]) ** 2)]], np.zeros((1, 4)), np.eye(4)[None], 12)
    dense = np.array([r["E_phi"][0], u @ r["E_xmuphi"][0], u @ (r["E_xxphi"][0] - r["E_phi"][0] * np.eye(4)) @ u])
    es, ed = np.abs(sparse - exact) / np.abs(exact), np.abs(dense - exact) / np.abs(exact)
    print(f"c {c}: sparse (4, 5) {es}, tensor order 12 {ed}")
    checked = 0
    for i in range(3):
        if es[i] < 1e-13 and ed[i] < 1e-13:
            continue                                                  # exact for both
        checked += 1
        assert ed[i] * 10 <= es[i], (c, i, ed[i], es[i])
    assert checked == (1 if c == 0.0 else 3)


# ---- 3. route decisions ----
@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "sanitized"])
def test_route_decisions(tmp_path, flags):
    exe = compile_stub(tmp_path, "readout_routes_check", flags)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ALL OK", r.stdout[-4000:] + r.stderr[-4000:]


# ---- 4. the interface without a device ----
def test_interface_is_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    assert "gvi_status gvi_factors_set_readout_rule(gvi_ctx* ctx, int set_id, int order);" in header
    assert "gvi_status gvi_factors_readout_info(const gvi_ctx* ctx, int set_id, int* order, int* P, int* J, int64_t* points_per_check_point);" in header
    assert "8 read-out-space rule" in header
    assert {"gvi_factors_set_readout_rule", "gvi_factors_readout_info"} <= set(_lib.SIGNATURES)
    assert hasattr(api.Context, "factors_set_readout_rule") and hasattr(api.Context, "factors_readout_info")
    hip = open(os.path.join(CSRC, "api_setup.inc")).read()        # the file that defines gvi_factors_set_readout_rule
    for text in ("only the kinds on linear read-outs", "order is 0 (off) or 2 <= order <= 16 with order^P <= 1024"):
        assert text in hip
    assert "read-out rule kernel supports d <= 32" in open(os.path.join(CSRC, "routes.hpp")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 18." in design and "gvi_factors_set_readout_rule" in open(os.path.join(ROOT, "README.md")).read()


def test_builders_carry_the_order():
    plain = syn.make_planar_chain(T=9, segment_taus=[0.1])
    assert all("readout_order" not in s for s in plain["specs"])
    ch = syn.make_planar_chain(T=9, segment_taus=[0.1], readout_order=8)
    assert [s.get("readout_order", 0) for s in ch["specs"]] == [0, 0, 8, 0]
    assert np.array_equal(ch["specs"][2]["params"], plain["specs"][2]["params"])
    pr = syn.make_obstacle_chain("pr3d", segment_taus=[0.1], readout_order=5)
    assert [s.get("readout_order", 0) for s in pr["specs"]] == [0, 0, 5, 0] and pr["specs"][2]["kind"] == syn.PSI_HINGE_SDF_3D_SEG
    mv = syn.add_moving_obstacle_set(plain, [[0.0, 1.0]], [[0.0, -1.0]], [0.5], readout_order=9)
    assert mv["specs"][-1]["readout_order"] == 9 and "readout_order" not in syn.add_moving_obstacle_set(plain, [[0.0, 1.0]], [[0.0, -1.0]], [0.5])["specs"][-1]


def test_reference_on_the_three_layouts():
    """readout_ref reads the leading coordinates, _SEG blocks and BALLS blocks alike: a BALLS set whose ball is the disc of a fine
    planar grid agrees with the grid kinds to the grid's interpolation error, and HINGE_SDF_2D is the _SEG set with W = [I | 0]."""
    rng = np.random.default_rng(9)
    d, K, order = 4, 3, 8
    mu, Sigma = syn.random_marginals(rng, K, d, 0.01)
    mu[:, :2] = [[0.9, 0.2], [1.1, -0.3], [0.2, 1.0]]
    origin, cell = (-2.0, -2.0), 0.01
    fld = syn.circle_sdf(origin, cell, 401, 401, [(0.0, 0.0)], [0.7])
    head = np.tile([12.0, 0.3, 0.1], (K, 1))
    lead = dict(kind=syn.PSI_HINGE_SDF_2D, d=d, params=head, temperature=np.ones(K), sdf_origin=origin, sdf_cell=cell, sdf_field=fld)
    W = np.eye(2, d)[None]
    seg = dict(lead, kind=syn.PSI_HINGE_SDF_2D_SEG, params=syn.segment_params(12.0, 0.3, 0.1, np.tile(W, (K, 1, 1, 1)), np.zeros((K, 1, 2))))
    balls = dict(kind=syn.PSI_HINGE_BALLS_2D, d=d, temperature=np.ones(K),
                 params=np.tile(syn.balls_params(12.0, 0.3, 0.1, W, np.zeros((1, 2)), [0.0], [[0.0, 0.0]], [[0.0, 0.0]], [0.7]), (K, 1)))
    a, b, c = (rr.spec_moments(s, mu, Sigma, order) for s in (lead, seg, balls))
    assert a["E_phi"].min() > 1e-3
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert relmax(c[k], a[k]) <= 1e-3, (k, relmax(c[k], a[k]))      # bilinear interpolation of a disc's distance at cell 0.01
    assert br.NPOS[balls["kind"]] == rr.NPOS[balls["kind"]] == 2


def test_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "readout_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "readout_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
