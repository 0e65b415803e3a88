"""CPU checks of the obstacle factors on a segment (GVI_PSI_HINGE_SDF_2D_SEG / _3D_SEG): the numpy reference psi of
tests/segment_ref.py against the oracle's single-point kinds, the read-out builder, the input condition the GPU tests rely on
(both hinge branches and a mixed factor, asserted on the reference alone), the builders' defaults and the shim call site."""
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o
import segment_ref as sr
from gaussianvi_amd import api, build, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.25
TAUS = [DT / 4, DT / 2, 3 * DT / 4]


def test_constants():
    assert (api.PSI_HINGE_SDF_2D_SEG, api.PSI_HINGE_SDF_3D_SEG) == (8, 9) == (syn.PSI_HINGE_SDF_2D_SEG, syn.PSI_HINGE_SDF_3D_SEG)
    hdr = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    assert "GVI_PSI_HINGE_SDF_2D_SEG = 8" in hdr and "GVI_PSI_HINGE_SDF_3D_SEG = 9" in hdr


@pytest.mark.parametrize("P", [2, 3])
def test_degenerate_case_is_the_single_point_kind_bit_for_bit(P):
    """J = 1, W = [I_P 0], c = 0: the reference equals o.psi_batch_hinge_sdf2d / _3d."""
    ch = syn.make_planar_chain(T=9) if P == 2 else syn.make_obstacle_chain("pr3d", T=9)
    ob = ch["specs"][1]
    rng = np.random.default_rng(7 + P)
    K, d = 5, ob["d"]
    head = np.stack([rng.uniform(5, 20, K), rng.uniform(0.2, 0.6, K), rng.uniform(0.1, 0.4, K)], axis=1)
    X = ch["mu0"][:K, None, :] + 0.6 * rng.normal(size=(K, 200, d))
    X[0, :5] = 50.0                                                     # outside the grid: clamped
    W = np.zeros((1, P, d))
    W[0, :, :P] = np.eye(P)
    params = syn.segment_params(head[:, 0], head[:, 1], head[:, 2], W, np.zeros((1, P)))
    assert params.shape == (K, 3 + P * (d + 1))
    single = (o.psi_batch_hinge_sdf2d if P == 2 else o.psi_batch_hinge_sdf3d)(head, ob["sdf_origin"], ob["sdf_cell"], ob["sdf_field"])
    ref, got = single(X), sr.psi_batch_hinge_seg(params, P, d, ob["sdf_origin"], ob["sdf_cell"], ob["sdf_field"])(X)
    assert ref.max() > 0 and (ref == 0).any()
    assert np.array_equal(got, ref)
    assert np.array_equal(sr.psi_batch_hinge_seg(params, P, d, ob["sdf_origin"], ob["sdf_cell"], ob["sdf_field"])(X[1:3], sel=slice(1, 3)), ref[1:3])


def test_readout_end_points_and_interior():
    for nd, npos in ((2, 2), (3, 3), (3, 2)):
        n = 2 * nd
        W, c = syn.minacc_segment_readout(nd, syn.QC, DT, [0.0, DT], npos)
        assert W.shape == (2, npos, 2 * n) and c.shape == (2, npos) and not c.any()
        first, last = np.zeros((npos, 2 * n)), np.zeros((npos, 2 * n))
        first[:, :npos], last[:, n:n + npos] = np.eye(npos), np.eye(npos)
        assert np.array_equal(W[0], first) and np.array_equal(W[1], last)
        Wm, _ = syn.minacc_segment_readout(nd, syn.QC, DT, [DT / 2], npos)
        A, B, _ = syn.minacc_interpolation(nd, syn.QC, DT, DT / 2)
        assert np.array_equal(Wm[0], np.hstack([A[:npos], B[:npos]]))
        # a constant-velocity segment is reproduced: the position at dt / 2 of x_i = (q, v), x_i+1 = (q + dt v, v)
        q, v = np.arange(1.0, nd + 1), np.linspace(-1.0, 2.0, nd)
        x = np.concatenate([q, v, q + DT * v, v])
        assert np.allclose(Wm[0] @ x, (q + DT / 2 * v)[:npos], rtol=0, atol=1e-13)


def test_segment_params_layout():
    rng = np.random.default_rng(3)
    K, J, P, d = 4, 3, 2, 8
    W, c = rng.normal(size=(K, J, P, d)), rng.normal(size=(K, J, P))
    sig, eps, r = rng.uniform(1, 2, K), rng.uniform(0, 1, K), rng.uniform(0, 1, K)
    prm = syn.segment_params(sig, eps, r, W, c)
    assert prm.shape == (K, 3 + J * P * (d + 1)) and prm.flags["C_CONTIGUOUS"]
    s2, e2, r2, W2, c2 = sr.unpack(prm, P, d)
    for a, b in ((s2, sig), (e2, eps), (r2, r), (W2, W), (c2, c)):
        assert np.array_equal(a, b)
    assert np.array_equal(prm[1, 3:3 + d], W[1, 0, 0]) and np.array_equal(prm[1, 3 + P * d:3 + P * d + P], c[1, 0])
    shared = syn.segment_params(1.0, 0.5, 0.25, W[0], c[0])
    assert shared.shape == (1, prm.shape[1]) and np.array_equal(shared[0, 3:], prm[0, 3:])


def _mixed(shares):
    return bool((shares == 0).any() and (shares == 1).any() and ((shares > 0.05) & (shares < 0.95)).any())


@pytest.mark.parametrize("p", [3, 4])
def test_input_condition_planar(p):
    """A factor with no sigma point in the hinge, one with all of them, and one strictly between 0.05 and 0.95: a device
    result cannot pass on all-zero hinges, and both branches of the hinge are taken inside one factor."""
    ch = syn.make_planar_chain(T=9, p=3, segment_taus=TAUS, segment_p=p)
    spec = ch["specs"][2]
    assert (spec["kind"], spec["d"], spec["p"], len(spec["start"])) == (syn.PSI_HINGE_SDF_2D_SEG, 8, p, 8)
    shares = sr.sigma_point_shares(ch, spec)
    print("planar p", p, np.round(shares, 2))
    assert _mixed(shares), shares


def test_input_condition_pr3d():
    ch = syn.make_obstacle_chain("pr3d", T=9, segment_taus=TAUS, segment_p=3)
    spec = ch["specs"][2]
    assert (spec["kind"], spec["d"], spec["p"], len(spec["start"])) == (syn.PSI_HINGE_SDF_3D_SEG, 12, 3, 8)
    shares = sr.sigma_point_shares(ch, spec)
    print("pr3d", np.round(shares, 2))
    assert _mixed(shares), shares


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("make", [lambda **kw: syn.make_planar_chain(**kw), lambda **kw: syn.make_planar_chain(T=9, p=3, p_obstacle=5, **kw),
                                  lambda **kw: syn.make_obstacle_chain("pr3d", **kw), lambda **kw: syn.make_obstacle_chain("quad2d", **kw)])
def test_builder_defaults_are_unchanged(make):
    """segment_taus = None returns what a call without the argument returns, array by array; with it, the other sets and the
    start state are the same and the segment set sits behind the obstacle set."""
    a, b = make(), make(segment_taus=None)
    assert len(a["specs"]) == 3 and len(b["specs"]) == 3
    for sa, sb in zip(a["specs"], b["specs"]):
        _same(sa, sb)
    for k in ("mu0", "D0", "U0"):
        assert np.array_equal(a[k], b[k])
    assert (a["T"], a["n"], a["name"]) == (b["T"], b["n"], b["name"])
    if a["name"] != "quad2d":
        c = make(segment_taus=TAUS)
        assert len(c["specs"]) == 4 and c["specs"][2]["kind"] in sr.NPOS
        for i, j in ((0, 0), (1, 1), (2, 3)):
            _same(a["specs"][i], c["specs"][j])
        for k in ("mu0", "D0", "U0"):
            assert np.array_equal(a[k], c[k])
        seg, ob = c["specs"][2], c["specs"][1]
        assert np.array_equal(seg["start"], np.arange(a["T"] - 1)) and seg["d"] == 2 * a["n"] and seg["p"] == ob["p"]
        assert np.array_equal(seg["params"][:, :3], ob["params"][:-1]) and seg["sdf_field"] is ob["sdf_field"]


def test_oracle_accepts_the_closure():
    """o.FactorSet takes the reference closure, and o.ChainNGD on planar(T = 9) plus a J = 3 segment set accepts its steps."""
    ch = sr.attach_oracle(syn.make_planar_chain(T=9, p=3, segment_taus=TAUS))
    ngd = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    c0 = ngd.cost_value(ngd.mu, ngd.D, ngd.U)
    ok, c1, ntr = ngd.step()
    print(f"cost {c0:.2f} -> {c1:.2f}, trials {ntr}")
    assert ok and ntr == 1 and c1 < c0


def test_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "segment_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "segment_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
