"""CPU checks of the limit factors (GVI_PSI_HINGE_BOX): the closed-form 1-D expectations of
tests/box_ref.py against piecewise Gauss-Legendre integration, the functions the kernels call (gaussianvi_amd/csrc/
box_moments.hpp) compiled for the host under AddressSanitizer / UBSan against box_ref, the builders, and the shim call site."""
import math
import os
import subprocess

import numpy as np
import pytest

import box_ref as br
import gvi_oracle as o
from gaussianvi_amd import api, build, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [-6.0, -4.0, -2.5, -1.5, -1.0, -0.3, 0.0, 1e-9, 0.3, 1.0, 1.5, 2.5, 4.0, 6.0]


def test_constants():
    assert api.PSI_HINGE_BOX == 10 == syn.PSI_HINGE_BOX
    assert "GVI_PSI_HINGE_BOX = 10" in open(os.path.join(ROOT, "include", "gvi_hip.h")).read()


def gauss_legendre_side(sigma, sd, gap, sgn, nodes=64, span=12.0):
    """E[h], E[h'], E[h''] of h(x) = sigma max(0, sgn (x - a))^2, x = m + sd z, by Gauss-Legendre on the two pieces of
    z in [-span, span] split at the kink z0 = -gap / (sgn sd): polynomial times Gaussian on each piece."""
    xg, wg = np.polynomial.legendre.leggauss(nodes)
    z0 = min(max(-sgn * gap / sd, -span), span)
    out = np.zeros(3)
    # pieces of at most 4 sd: 64 nodes then resolve the Gaussian to rounding
    edges = sorted(set([-span, span, z0] + list(np.arange(-span, span + 1e-9, 4.0))))
    for a, b in zip(edges[:-1], edges[1:]):
        if b <= a:
            continue
        z = 0.5 * (b - a) * xg + 0.5 * (a + b)
        w = 0.5 * (b - a) * wg * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        e = sgn * (sd * z) + gap                      # sgn (x - a)
        on = e > 0
        out += [(w * sigma * np.where(on, e * e, 0.0)).sum(), (w * sgn * 2.0 * sigma * np.where(on, e, 0.0)).sum(),
                (w * 2.0 * sigma * on).sum()]
    return out


@pytest.mark.parametrize("sgn", [1.0, -1.0])
def test_side_expectations_vs_gauss_legendre(sgn):
    """1e-12 relative for |t| <= 6."""
    worst = 0.0
    for sigma in (0.5, 3.0):
        for sd in (0.05, 0.7):
            for t in TS:
                got = np.array(br.side_expectations(sigma, sd, t * sd, sgn)).reshape(3)
                ref = gauss_legendre_side(sigma, sd, t * sd, sgn)
                err = np.abs(got - ref) / np.abs(ref)
                worst = max(worst, err.max())
                assert err.max() <= 1e-12, (sigma, sd, t, got, ref)
    print(f"sgn {sgn:+.0f}: worst relative error against Gauss-Legendre {worst:.2e}")


def test_tails_and_infinite_sides_are_finite():
    for t in (-40.0, 40.0):
        for sgn in (1.0, -1.0):
            e = np.array(br.side_expectations(2.0, 0.3, t * 0.3, sgn)).reshape(3)
            assert np.isfinite(e).all()
            if t < 0:
                assert (np.abs(e) <= 1e-300).all(), e
            else:                                      # the hinge is on everywhere: a plain quadratic, E = sigma (gap^2 + sd^2)
                assert np.allclose(e, [2.0 * (144.0 + 0.09), sgn * 2.0 * 2.0 * 12.0, 4.0], rtol=1e-15, atol=0)
    inf = np.inf
    params = syn.box_params([1.0, 2.0, 3.0], 0.1, [-inf, -inf, -1.0], [1.0, inf, inf])
    mu, Sigma = np.array([[0.5, 9.0, -3.0]]), np.array([np.diag([0.04, 0.09, 0.01])])
    r = br.closed_moments(params, 3, mu, Sigma, 2.0)
    assert all(np.isfinite(v).all() for v in r.values())
    assert r["Vdmu"][0, 1] == 0 and r["Vddmu"][0, 1, 1] == 0          # the coordinate without limits
    assert np.isnan(br.t_values(params, 3, mu, Sigma)[0, 1]).all()
    none = syn.box_params(1.0, 0.1, [-inf] * 3, [inf] * 3)
    r = br.closed_moments(none, 3, mu, Sigma, 1.0)
    assert all((v == 0).all() for v in r.values())
    assert (br.psi_batch(none, 3)(mu[:, None, :]) == 0).all() and br.margin(none, 3, mu[:, None, :])[0, 0] == inf


def test_closed_form_vs_dense_product_rule():
    """d = 2 with a correlated Sigma: the closed moments against a 200 x 200 product Gauss-Hermite rule.  The rule converges
    algebraically on a kink; 2e-4 is four times its own error (7e-5)."""
    x, w = np.polynomial.hermite_e.hermegauss(200)
    w = w / w.sum()
    Z = np.stack(np.meshgrid(x, x, indexing="ij"), axis=-1).reshape(-1, 2)
    W = np.outer(w, w).reshape(-1)
    rng = np.random.default_rng(11)
    mu, Sigma = syn.random_marginals(rng, 3, 2, 0.1)
    params = syn.box_params(rng.uniform(1, 5, (3, 2)), 0.1, -1.0, 1.0)
    mu[:] = [[0.9, -0.95], [0.5, 1.2], [-1.4, 0.0]]
    ref = o.batched_moments(Z, W, mu, Sigma, br.psi_batch(params, 2), 1.5)
    got = br.closed_moments(params, 2, mu, Sigma, 1.5)
    for k in ("E_phi", "Vdmu", "Vddmu", "E_xmuphi", "E_xxphi"):
        err = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(k, f"{err:.2e}")
        assert err <= 2e-4, (k, err)


def test_device_functions_on_cpu_under_sanitizers(tmp_path):
    """box_moments.hpp as a stand-alone host program built with -fsanitize=address,undefined; its grid of values against
    box_ref.  Bound 1e-13 relative to the VALUE, entry by entry (a value below 1e-300 -- underflow at t = -40 -- must be
    below 1e-300 on both sides).  The brackets of the formulas cancel for t < 0; evaluated literally they are 2e-12 off at
    t = -6 and fail this test, which is what the continued fraction of box_moments.hpp is for."""
    exe = str(tmp_path / "box_side_on_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "gaussianvi_amd", "csrc"), os.path.join(ROOT, "tests", "stubs", "box_side_on_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    side = np.array([[float.fromhex(v) for v in row[1:]] for row in rows if row[0] == "side"])
    assert len(side) == 2 * 3 * 18 * 2
    worst, literal_worst = 0.0, 0.0
    for sigma, sd, gap, sgn, e0, e1, e2 in side:
        assert np.isfinite([e0, e1, e2]).all()
        if sd == 0.0:                                  # deterministic coordinate: the hinge at the mean
            g = max(gap, 0.0)
            assert (e0, e1, e2) == (sigma * g * g, sgn * 2.0 * sigma * g, 2.0 * sigma if gap > 0 else 0.0)
            continue
        t = gap / sd
        ref = np.array(br.side_expectations(sigma, sd, gap, sgn)).reshape(3)
        got = np.array([e0, e1, e2])
        tiny = np.abs(ref) < 1e-300
        assert (np.abs(got[tiny]) < 1e-300).all(), (sigma, sd, t, sgn, got, ref)
        err = np.abs(got[~tiny] - ref[~tiny]) / np.abs(ref[~tiny])
        if err.size:
            worst = max(worst, err.max())
            assert err.max() <= 1e-13, (sigma, sd, t, sgn, got, ref)
        if t <= -3.0:                                  # the literal brackets are NOT good enough here: the test can see the tail branch
            Phi, phi = 0.5 * math.erfc(-t / math.sqrt(2.0)), math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
            naive = sigma * sd * sd * ((1 + t * t) * Phi + t * phi)
            literal_worst = max(literal_worst, abs(naive - ref[0]) / abs(ref[0]) if abs(ref[0]) >= 1e-300 else 0.0)
        if t == -40.0:
            assert max(abs(e0), abs(e1), abs(e2)) <= 1e-300
    print(f"host build of box_moments.hpp against box_ref: worst {worst:.2e}; the literal brackets at t <= -3: {literal_worst:.2e}")
    assert literal_worst > 1e-13                        # the grid reaches where the literal formula loses its digits
    # box_coordinate / psi_hinge_box / box_margin on the d = 4 block of the program
    inf = np.inf
    params = np.array([[1.5, 2.0, 2.5, 3.0, 0.1, 0.1, 0.2, 0.0, -inf, -inf, -1.0, -0.5, 1.0, inf, 1.0, inf]])
    ms = np.array([[0.95, 7.0, -0.9, -0.45], [0.0, -3.0, 0.0, 1.0], [2.0, 0.0, 1.2, -2.0]])
    coord = {(int(row[1]), int(row[2])): [float.fromhex(v) for v in row[3:]] for row in rows if row[0] == "coord"}
    point = {int(row[1]): [float.fromhex(v) for v in row[2:]] for row in rows if row[0] == "point"}
    for c in range(3):
        e = br.coordinate_expectations(params, 4, ms[c:c + 1], np.full((1, 4), 0.3))
        for i in range(4):
            ref, got = np.array([v[0, i] for v in e]), np.array(coord[(c, i)])
            tiny = np.abs(ref) < 1e-300
            assert (np.abs(got[tiny]) < 1e-300).all() and (np.abs(got[~tiny] - ref[~tiny]) <= 1e-13 * np.abs(ref[~tiny])).all(), (c, i, got, ref)
        assert coord[(c, 1)] == [0.0, 0.0, 0.0]
        X = ms[c][None, None, :]
        assert abs(point[c][0] - br.psi_batch(params, 4)(X)[0, 0]) <= 1e-15 * point[c][0]
        assert point[c][1] == br.margin(params, 4, X)[0, 0]


def test_box_params_and_builder():
    inf = np.inf
    prm = syn.box_params(2.0, 0.1, [-inf, -1.0], [1.0, inf])
    assert prm.shape == (1, 8) and prm.flags["C_CONTIGUOUS"]
    assert np.array_equal(prm[0], [2.0, 2.0, 0.1, 0.1, -inf, -1.0, 1.0, inf])
    per = syn.box_params(np.array([[1.0, 2.0], [3.0, 4.0]]), 0.0, -1.0, [[1.0, 2.0], [3.0, 4.0]])
    assert per.shape == (2, 8) and np.array_equal(per[1], [3.0, 4.0, 0.0, 0.0, -1.0, -1.0, 3.0, 4.0])
    sig, eps, lo, hi = br.unpack(per, 2)
    assert np.array_equal(hi, [[1.0, 2.0], [3.0, 4.0]]) and (lo == -1).all() and (eps == 0).all() and sig[1, 0] == 3.0
    base = syn.make_planar_chain(T=9)
    ch = syn.add_box_set(base, [-inf, -inf, -2.0, -0.3], [inf, inf, 2.0, 0.3], sigma=8.0, eps=0.05, p=4)
    assert len(ch["specs"]) == len(base["specs"]) + 1 and all(a is b for a, b in zip(ch["specs"], base["specs"]))
    assert len(base["specs"]) == 3                                       # the chain it was built from is left alone
    box = ch["specs"][-1]
    assert (box["kind"], box["d"], box["p"], box["params"].shape) == (syn.PSI_HINGE_BOX, 4, 4, (9, 16))
    assert np.array_equal(box["start"], np.arange(9)) and (box["temperature"] == 1).all()
    pair = syn.add_box_set(base, -1.0, 1.0, pair=True)["specs"][-1]
    assert (pair["d"], pair["params"].shape) == (8, (8, 32)) and np.array_equal(pair["start"], np.arange(8))


def test_oracle_accepts_the_closed_form():
    """o.ChainNGD on planar(T = 9) plus velocity limits, closed form plugged in as fast_moments: the first step is accepted."""
    import test_box_gpu as g
    ch = g.limited_graph("planar")
    ngd = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](True), ch["mu0"], ch["D0"], ch["U0"])
    ok, cost, ntr = ngd.step()
    print(f"accepted {ok} cost {cost:.4f} trials {ntr}")
    assert ok


def test_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "box_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "box_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
