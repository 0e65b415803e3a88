"""The read-out-space quadrature (gvi_factors_set_readout_rule) on the device against tests/readout_ref.py.

Bounds, max-norm relative per case (rel of tests/test_gpu_parity.py), as in tests/test_box_gpu.py: operators 1e-9 (Vddmu, E_xxphi
1e-8); chain iterates 1e-7 and costs 1e-9.  The rule and the sparse rule compute DIFFERENT numbers on purpose, so they are held to
each other only where both are exact (test_exact_on_a_plane).

The inputs of the parity cases are chosen by the reference alone (draw_case): per case both hinge branches occur, eps of every
factor is moved so that the median node of its rule sits 5e-7 inside (even factors) or outside (odd factors) the hinge boundary
-- a case of one factor has a node within 1e-6 on one side only --, and no node is clamped at the grid edge, except in the case
that clamps on purpose.  f_j is continuously differentiable, so a node that rounding puts on the other side of the boundary
changes a sum by less than 1e-12 of a node's share."""
import functools
import os
import subprocess

import numpy as np
import pytest

import balls_ref as br
import gvi_oracle as o
import halfspace_ref as hr
import readout_ref as rr
import segment_ref as sr
import test_box_gpu as box_gpu
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import TIGHT, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN2, CELL2, ROWS2, COLS2 = (-5.0, -4.0), 0.1, 81, 101
DISCS = [((0.0, 0.6), 1.0), ((-0.5, -0.8), 0.8)]
ORIGIN3, CELL3, SHAPE3 = (-4.0, -3.0, -2.0), 0.2, (31, 41, 21)
BALLS3 = [((0.0, 0.5, 0.1), 0.5), ((-0.5, -0.8, 0.0), 0.4)]
LEAD = (api.PSI_HINGE_SDF_2D, api.PSI_HINGE_SDF_3D)
SEG = (api.PSI_HINGE_SDF_2D_SEG, api.PSI_HINGE_SDF_3D_SEG)
BALLS = (api.PSI_HINGE_BALLS_2D, api.PSI_HINGE_BALLS_3D)
SWITCH = 1024                         # factors above which the launch takes four waves per block (plan_readout)


@functools.lru_cache(maxsize=None)
def field(P):
    if P == 2:
        return syn.circle_sdf(ORIGIN2, CELL2, ROWS2, COLS2, [c for c, _ in DISCS], [r for _, r in DISCS])
    return syn.sphere_sdf3d(ORIGIN3, CELL3, *SHAPE3, [c for c, _ in BALLS3], [r for _, r in BALLS3])


def grid_box(P):
    """(lo, hi) [P] of the grid in read-out coordinates (x -> columns, y -> rows, z -> slices)."""
    if P == 2:
        lo = np.array(ORIGIN2)
        return lo, lo + CELL2 * (np.array([COLS2, ROWS2]) - 1)
    lo = np.array(ORIGIN3)
    return lo, lo + CELL3 * (np.array([SHAPE3[1], SHAPE3[0], SHAPE3[2]]) - 1)


def well_conditioned_readouts(rng, K, J, P, d):
    """W [K][J][P][d]: P orthonormal rows of a random rotation, each scaled by a factor in (0.7, 1.3), so that the condition number
    of W Sigma W^T is at most 3.5 times that of Sigma (the reference refuses more than 1e4)."""
    Q = np.linalg.qr(rng.normal(size=(K, J, d, P)))[0]
    return np.transpose(Q, (0, 1, 3, 2)) * rng.uniform(0.7, 1.3, (K, J, P, 1))


def make_spec(kind, d, J, K, rng, live=3, clamp=False, p=None):
    """A set's spec with read-outs whose means lie on the rim of an obstacle.  sigma in (5, 20), r = 0.1, eps = 0.2 to start with."""
    P = rr.NPOS[kind]
    obstacles = DISCS if P == 2 else BALLS3
    centre = np.array([obstacles[k % 2][0] for k in range(K)])                            # [K][P]
    radius = np.array([obstacles[k % 2][1] for k in range(K)])
    u = rng.normal(size=(K, max(J, 1), P))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    target = centre[:, None, :] + (radius[:, None, None] + 0.3 + 0.1 * rng.uniform(-1, 1, (K, max(J, 1), 1))) * u   # sd about 0.3 = eps + r
    if clamp:
        target[:, :, 0] = grid_box(P)[1][0] - 0.02                                       # 0.02 inside the upper x edge: nodes go past it
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.004)       # read-out standard deviations below 0.17: the rule's nodes reach 0.8 at most
    sigma, eps, r = rng.uniform(5.0, 20.0, K), np.full(K, 0.2), 0.1
    spec = dict(kind=kind, d=d, p=p if p is not None else (3 if d <= 12 else 2), start=np.zeros(K, dtype=np.int32), temperature=rng.uniform(0.5, 5.0, K))
    if kind in LEAD:
        mu[:, :P] = target[:, 0]
        spec["params"] = np.stack([sigma, eps, np.full(K, r)], axis=1)
    else:
        W = well_conditioned_readouts(rng, K, J, P, d)
        c = target - np.einsum("kjpd,kd->kjp", W, mu)
        if kind in SEG:
            spec["params"] = syn.segment_params(sigma, eps, r, W, c)
        else:
            M = live
            cen = np.zeros((K, M, P)); vel = rng.normal(size=(K, M, P)) * 0.5; rad = rng.uniform(0.3, 0.8, (K, M))
            tau = np.tile(np.linspace(0.05, 0.2, J), (K, 1))
            for k in range(K):
                for m in range(M):                                      # ball m is 0.3 off check point m % J when that point is taken
                    j = m % J
                    v = rng.normal(size=P); v /= np.linalg.norm(v)
                    cen[k, m] = target[k, j] + (rad[k, m] + 0.3 + 0.1 * rng.uniform(-1, 1)) * v - tau[k, j] * vel[k, m]
            spec["params"] = syn.balls_params(sigma, eps, r, W, c, tau, cen, vel, rad)
    if kind not in BALLS:
        spec.update(sdf_origin=ORIGIN2 if P == 2 else ORIGIN3, sdf_cell=CELL2 if P == 2 else CELL3, sdf_field=field(P))
    return spec, mu, Sigma


def draw_case(kind, d, J, K, order, seed, live=3, clamp=False):
    """The spec of make_spec with eps moved per factor (see the module text), and what the reference says about its inputs."""
    rng = np.random.default_rng(seed)
    spec, mu, Sigma = make_spec(kind, d, J, K, rng, live, clamp)
    gaps, _ = rr.spec_gaps(spec, mu, Sigma, order)
    for k in range(K):
        g = np.sort(gaps[k][np.isfinite(gaps[k])])
        if g.size:                                                    # the median node goes on the boundary: nodes on both sides of it
            spec["params"][k, 1] += -g[g.size // 2 - (k % 2)] + (5e-7 if k % 2 == 0 else -5e-7)
    gaps, q = rr.spec_gaps(spec, mu, Sigma, order)
    allg = np.concatenate(gaps)
    lo, hi = grid_box(rr.NPOS[kind])
    props = dict(inside=bool((allg > 0).any()), outside=bool((allg <= 0).any()),
                 near_in=bool(((allg > 0) & (allg < 1e-6)).any()), near_out=bool(((allg <= 0) & (allg > -1e-6)).any()),
                 clamped=bool(kind not in BALLS and any(((v < lo) | (v > hi)).any() for v in q)))
    return spec, mu, Sigma, props


def load(spec):
    ctx = api.Context(0)
    ctx.chain_set(1, spec["d"])
    sid = ctx.factors_add(spec["d"], spec["p"], spec["start"], spec["kind"], spec["params"], spec["temperature"])
    if spec["kind"] in (api.PSI_HINGE_SDF_2D, api.PSI_HINGE_SDF_2D_SEG):
        ctx.factors_set_sdf2d(sid, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    if spec["kind"] in (api.PSI_HINGE_SDF_3D, api.PSI_HINGE_SDF_3D_SEG):
        ctx.factors_set_sdf3d(sid, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    return ctx, sid


def operators(ctx, sid, mu, Sigma):
    Ephi, Vdmu, Vddmu = ctx.moments(sid, mu, Sigma)
    E0, E1, E2 = ctx.raw_moments(sid, mu, Sigma)
    return dict(E_phi=Ephi, Vdmu=Vdmu, Vddmu=Vddmu, cost=ctx.costs(sid, mu, Sigma), E0=E0, E_xmuphi=E1, E_xxphi=E2)


def check_operators(got, ref, tag):
    errs = {k: rel(got[k], ref["E_phi" if k == "E0" else k]) for k in got}
    print(tag + ": " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < (TIGHT * 10 if k in ("Vddmu", "E_xxphi") else TIGHT), (tag, k, v)


# ---- 1. parity ----
KD = [(api.PSI_HINGE_SDF_2D, 2), (api.PSI_HINGE_SDF_2D, 4), (api.PSI_HINGE_SDF_2D, 6), (api.PSI_HINGE_SDF_3D, 3), (api.PSI_HINGE_SDF_3D, 6),
      (api.PSI_HINGE_SDF_2D_SEG, 4), (api.PSI_HINGE_SDF_2D_SEG, 8), (api.PSI_HINGE_SDF_2D_SEG, 12), (api.PSI_HINGE_SDF_2D_SEG, 32),
      (api.PSI_HINGE_SDF_3D_SEG, 6), (api.PSI_HINGE_SDF_3D_SEG, 12), (api.PSI_HINGE_BALLS_2D, 2), (api.PSI_HINGE_BALLS_2D, 8),
      (api.PSI_HINGE_BALLS_2D, 12), (api.PSI_HINGE_BALLS_3D, 3), (api.PSI_HINGE_BALLS_3D, 12)]
ORDERS = {2: [2, 7, 8, 9, 16], 3: [2, 4, 5, 10]}      # P = 2: below, at and just over one wave, then four passes


def parity_cases():
    """Every (kind, d) three times, J, K and the order rotating so that each value meets each kind; then every order once more on
    one shape per P, a K above the launch-shape switch, and the ball kinds with 0, 1, 3, 8 live slots."""
    out, n = [], 0
    for kind, d in KD:
        P = rr.NPOS[kind]
        for rep in range(3):
            J = 1 if kind in LEAD else [1, 3, 8][(n + rep) % 3]
            out.append((kind, d, J, [1, 5, 67][(n // 3 + rep) % 3], ORDERS[P][(n + rep) % len(ORDERS[P])], 3))
        n += 1
    for order in ORDERS[2]:
        out.append((api.PSI_HINGE_SDF_2D_SEG, 8, 3, 5, order, 3))
    for order in ORDERS[3]:
        out.append((api.PSI_HINGE_SDF_3D_SEG, 6, 3, 5, order, 3))
    out.append((api.PSI_HINGE_SDF_2D, 4, 1, SWITCH + 5, 7, 3))
    out.append((api.PSI_HINGE_SDF_2D_SEG, 8, 3, SWITCH, 8, 3))       # the largest launch of one wave per block
    for live in (0, 1, 3, 8):
        out.append((api.PSI_HINGE_BALLS_2D, 8, 3, 5, 8, live))
        out.append((api.PSI_HINGE_BALLS_3D, 6, 3, 5, 5, live))
    return out


def test_parity_cases_cover_the_issue():
    cases = parity_cases()
    assert {(c[0], c[1]) for c in cases} >= set(KD)
    assert {c[2] for c in cases} == {1, 3, 8} and {c[3] for c in cases} >= {1, 5, 67, SWITCH, SWITCH + 5}
    for P in (2, 3):
        assert {c[4] for c in cases if rr.NPOS[c[0]] == P} == set(ORDERS[P])
    assert {c[5] for c in cases if c[0] in BALLS} == {0, 1, 3, 8}


@pytest.mark.parametrize("kind,d,J,K,order,live", parity_cases())
def test_parity_vs_reference(kind, d, J, K, order, live):
    spec, mu, Sigma, props = draw_case(kind, d, J, K, order, 1000 * kind + 10 * d + J + K + order, live)
    if not (kind in BALLS and live == 0):
        assert props["inside"] and props["outside"], props
        assert props["near_in"] and (props["near_out"] or K == 1), props
    assert not props["clamped"] and (spec["temperature"] != 1).all()
    ref = rr.spec_moments(spec, mu, Sigma, order)
    if live:
        assert ref["E_phi"].max() > 1e-3
    ctx, sid = load(spec)
    ctx.factors_set_readout_rule(sid, order)
    P = rr.NPOS[kind]
    assert ctx.factors_readout_info(sid) == dict(order=order, P=P, J=J, points_per_check_point=order ** P)
    got = operators(ctx, sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] == 8
    check_operators(got, ref, f"kind {kind} d {d} J {J} K {K} order {order} live {live}")
    if kind in BALLS and live == 0:
        assert all((v == 0).all() for v in got.values())
    ctx.close()


def test_parity_with_nodes_clamped_at_the_grid_edge():
    spec, mu, Sigma, props = draw_case(api.PSI_HINGE_SDF_2D_SEG, 8, 3, 5, 8, 77, clamp=True)
    assert props["clamped"]
    ctx, sid = load(spec)
    ctx.factors_set_readout_rule(sid, 8)
    check_operators(operators(ctx, sid, mu, Sigma), rr.spec_moments(spec, mu, Sigma, 8), "clamped")
    ctx.close()


# ---- 2. exactness and 3. the kink: a grid that holds a linear field ----
NRM, B0 = np.array([0.6, -0.8]), 0.25


def plane_spec(kind, d, J, K, eps, rng):
    """sd(q) = NRM . q + B0 on the planar grid (the bilinear look-up reproduces it); read-out means within 0.3 of the origin."""
    xs, ys = ORIGIN2[0] + np.arange(COLS2) * CELL2, ORIGIN2[1] + np.arange(ROWS2) * CELL2
    fld = NRM[0] * xs[None, :] + NRM[1] * ys[:, None] + B0
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.02)
    sigma, r = rng.uniform(5.0, 20.0, K), 0.1
    spec = dict(kind=kind, d=d, p=3, start=np.zeros(K, dtype=np.int32), temperature=rng.uniform(0.5, 5.0, K), sdf_origin=ORIGIN2, sdf_cell=CELL2, sdf_field=fld)
    if kind in LEAD:
        mu[:, :2] = rng.uniform(-0.3, 0.3, (K, 2))
        spec["params"] = np.stack([sigma, np.full(K, eps), np.full(K, r)], axis=1)
    else:
        W = well_conditioned_readouts(rng, K, J, 2, d)
        c = rng.uniform(-0.3, 0.3, (K, J, 2)) - np.einsum("kjpd,kd->kjp", W, mu)
        spec["params"] = syn.segment_params(sigma, eps, r, W, c)
    return spec, mu, Sigma


@pytest.mark.parametrize("kind,d,J", [(api.PSI_HINGE_SDF_2D, 4, 1), (api.PSI_HINGE_SDF_2D_SEG, 8, 3)])
def test_exact_on_a_plane(kind, d, J):
    """eps so large that every node of both rules is inside the hinge and inside the grid (the reference asserts both): psi is a
    quadratic, and the read-out route at orders 3 and 8, the sparse route at p = 3 and o.batched_moments agree."""
    rng = np.random.default_rng(31 + d)
    spec, mu, Sigma = plane_spec(kind, d, J, 5, 6.0, rng)
    lo, hi = grid_box(2)
    for order in (3, 8):
        gaps, q = rr.spec_gaps(spec, mu, Sigma, order)
        assert all((g > 0).all() for g in gaps) and all(((v > lo) & (v < hi)).all() for v in q)
    Z, w = o.nwspgr_cached(d, 3)
    psi = o.psi_batch_hinge_sdf2d(spec["params"], ORIGIN2, CELL2, spec["sdf_field"]) if kind in LEAD else sr.spec_psi_batch(spec)
    ref = o.batched_moments(Z, w, mu, Sigma, psi, spec["temperature"])
    X = np.einsum("na,kba->knb", Z, ref["S"]) + mu[:, None, :]
    dist = sr.check_point_distances(spec["params"], 2, d, ORIGIN2, CELL2, spec["sdf_field"], X) if kind in SEG else \
        o.planar_sdf_lookup(X[:, :, 0], X[:, :, 1], ORIGIN2, CELL2, spec["sdf_field"])
    assert (dist < spec["params"][:, 1].min() + 0.1).all()                     # every sigma point inside the hinge
    ctx, sid = load(spec)
    sparse = operators(ctx, sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] in (1, 2)
    check_operators(sparse, ref, "plane, sparse route")
    for order in (3, 8):
        ctx.factors_set_readout_rule(sid, order)
        got = operators(ctx, sid, mu, Sigma)
        assert ctx.profile_geometry(sid)["variant"] == 8
        check_operators(got, ref, f"plane, read-out order {order} against the Gauss-Hermite sums")
        check_operators(got, rr.spec_moments(spec, mu, Sigma, order), f"plane, read-out order {order} against the reference")
    ctx.close()


def test_kink_through_the_mean():
    """The hinge boundary of the plane through every read-out mean: the device equals the reference to the parity bound, and the
    reference at order 16 is within 1e-3 of the exact moments of the equivalent half-space row a = -W^T n (halfspace_ref)."""
    rng = np.random.default_rng(77)
    d, K = 4, 5
    spec, mu, Sigma = plane_spec(api.PSI_HINGE_SDF_2D, d, 1, K, 0.0, rng)
    sd_mean = mu[:, :2] @ NRM + B0
    spec["params"][:, 1] = sd_mean - spec["params"][:, 2]                     # thr = eps + r = sd at the mean
    # psi = sigma max(0, thr - n.q - b0)^2 = sigma max(0, a^T x - (b - 0))^2 with a = -(n, 0, 0), b = b0 - thr
    A = np.zeros((K, 1, d)); A[:, 0, :2] = -NRM
    half = syn.halfspace_params(spec["params"][:, 0:1], 0.0, (B0 - sd_mean)[:, None], A)
    exact = hr.closed_moments(half, d, mu, Sigma, spec["temperature"])
    ref16 = rr.spec_moments(spec, mu, Sigma, 16)
    for k in ("E_phi", "Vdmu", "Vddmu", "E_xmuphi", "E_xxphi"):
        err = rel(ref16[k], exact[k])
        print(f"reference at order 16 against the closed form, {k}: {err:.2e}")
        assert err <= 1e-3, (k, err)
    ctx, sid = load(spec)
    for order in (8, 16):
        ctx.factors_set_readout_rule(sid, order)
        check_operators(operators(ctx, sid, mu, Sigma), rr.spec_moments(spec, mu, Sigma, order), f"kink, order {order}")
    ctx.close()


# ---- 4. degenerate read-outs ----
def test_zero_third_row_is_the_planar_scene():
    """_3D_SEG with W row 3 = 0 and c_3 = a time stamp, on a field whose every slice is the planar grid: finite, equal to the
    reference, and equal to the same scene posed as _2D_SEG to 1e-9."""
    rng = np.random.default_rng(41)
    d, J, K, order = 8, 3, 5, 8
    spec2, mu, Sigma, _ = draw_case(api.PSI_HINGE_SDF_2D_SEG, d, J, K, order, 411)
    _, _, _, W2, c2 = sr.unpack(spec2["params"], 2, d)
    W3 = np.concatenate([W2, np.zeros((K, J, 1, d))], axis=2)
    stamp = rng.uniform(0.0, 0.5, (K, J, 1))
    nz = 5
    spec3 = dict(spec2, kind=api.PSI_HINGE_SDF_3D_SEG, params=syn.segment_params(spec2["params"][:, 0], spec2["params"][:, 1], spec2["params"][:, 2], W3,
                                                                                  np.concatenate([c2, stamp], axis=2)),
                 sdf_origin=(ORIGIN2[0], ORIGIN2[1], -0.2), sdf_field=np.repeat(field(2)[:, :, None], nz, axis=2))
    ref = rr.spec_moments(spec3, mu, Sigma, order)
    assert all(np.isfinite(v).all() for v in ref.values())
    ctx, sid = load(spec3)
    ctx.factors_set_readout_rule(sid, order)
    got3 = operators(ctx, sid, mu, Sigma)
    ctx.close()
    assert all(np.isfinite(v).all() for v in got3.values())
    check_operators(got3, ref, "zero third row")
    ctx, sid = load(spec2)
    ctx.factors_set_readout_rule(sid, order)
    got2 = operators(ctx, sid, mu, Sigma)
    ctx.close()
    for k in got3:
        assert rel(got3[k], got2[k]) <= 1e-9, (k, rel(got3[k], got2[k]))


def test_parallel_rows_and_a_bad_sigma():
    """Two parallel rows of W (the second coordinate is dropped): finite and equal to the reference.  A Sigma_k that is not
    positive definite: NaN for that factor only."""
    d, J, K, order = 8, 3, 5, 8
    spec, mu, Sigma, _ = draw_case(api.PSI_HINGE_SDF_2D_SEG, d, J, K, order, 511)
    sig, eps, r, W, c = sr.unpack(spec["params"], 2, d)
    W = W.copy()
    W[:, :, 1, :] = -0.5 * W[:, :, 0, :]
    spec["params"] = syn.segment_params(sig, eps, r, W, c)
    diag = []
    ref = rr.moments(rr.spec_factors(spec), mu, Sigma, order, spec["temperature"], diag)
    assert all((e["keep"] == [True, False]).all() for dk in diag for e in dk)
    ctx, sid = load(spec)
    ctx.factors_set_readout_rule(sid, order)
    got = operators(ctx, sid, mu, Sigma)
    assert all(np.isfinite(v).all() for v in got.values()) and got["E_phi"].max() > 0
    check_operators(got, ref, "parallel rows")
    bad = Sigma.copy()
    lam, V = np.linalg.eigh(bad[2])
    lam[0] = -0.5 * lam[1]
    bad[2] = (V * lam) @ V.T
    got = operators(ctx, sid, mu, bad)
    for k, v in got.items():
        assert np.isnan(v[2]).all() and np.isfinite(np.delete(v, 2, axis=0)).all(), k
    ctx.close()


# ---- 5. determinism ----
def test_same_bits_from_run_to_run_and_for_any_K():
    spec, mu, Sigma, _ = draw_case(api.PSI_HINGE_SDF_2D_SEG, 8, 3, 67, 9, 611)
    ctx, sid = load(spec)
    ctx.factors_set_readout_rule(sid, 9)
    a, b = operators(ctx, sid, mu, Sigma), operators(ctx, sid, mu, Sigma)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    ctx.close()
    for k in (0, 33, 66):
        one = dict(spec, params=spec["params"][k:k + 1], start=spec["start"][:1], temperature=spec["temperature"][k:k + 1])
        ctx, sid = load(one)
        ctx.factors_set_readout_rule(sid, 9)
        got = operators(ctx, sid, mu[k:k + 1], Sigma[k:k + 1])
        assert all(np.array_equal(got[q][0], a[q][k]) for q in a), k
        ctx.close()


# ---- 6. switching ----
def test_switching():
    spec, mu, Sigma, _ = draw_case(api.PSI_HINGE_SDF_2D_SEG, 8, 3, 5, 8, 711)
    ctx, sid = load(spec)
    never = operators(ctx, sid, mu, Sigma)
    X = ctx.expand(sid, mu, Sigma)
    psi_vals = sr.spec_psi_batch(spec)(np.transpose(X, (0, 2, 1)))
    ext0 = ctx.moments_from_psi(sid, mu, Sigma, psi_vals)
    ctx.close()
    ctx, sid = load(spec)
    ctx.factors_set_readout_rule(sid, 8)
    on = operators(ctx, sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] == 8 and not np.array_equal(on["E_phi"], never["E_phi"])
    for variant in (1, 2, 0):                                        # the rule holds under every variant
        ctx.set_variant(variant)
        again = operators(ctx, sid, mu, Sigma)
        assert ctx.profile_geometry(sid)["variant"] == 8 and all(np.array_equal(again[k], on[k]) for k in on), variant
    assert np.array_equal(ctx.expand(sid, mu, Sigma), X)
    ext1 = ctx.moments_from_psi(sid, mu, Sigma, psi_vals)            # the caller's sigma points: the set's sparse table
    assert all(np.array_equal(a, b) for a, b in zip(ext0, ext1))
    ctx.factors_set_params(sid, spec["params"])                      # the rule survives new blocks
    assert ctx.factors_readout_info(sid)["order"] == 8
    kept = operators(ctx, sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] == 8 and all(np.array_equal(kept[k], on[k]) for k in on)
    ctx.factors_set_readout_rule(sid, 0)
    off = operators(ctx, sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] in (1, 2) and all(np.array_equal(off[k], never[k]) for k in off)
    ctx.close()


def test_sample_costs_and_clearance_ignore_the_rule():
    ch = graph("seg")
    out = {}
    for order in (0, 8):
        ctx, ids = api.context_for_chain(ch)
        ctx.factors_set_readout_rule(ids[2], order)
        smp = ch["mu0"][None] + 0.05 * np.random.default_rng(3).normal(size=(6,) + ch["mu0"].shape)
        out[order] = (ctx.sample_factor_costs(ids[2], smp), ctx.sample_clearance(ids[2], smp))
        ctx.close()
    assert np.array_equal(out[0][0], out[8][0]) and np.array_equal(out[0][1], out[8][1])


def test_argument_rules():
    spec, mu, Sigma, _ = draw_case(api.PSI_HINGE_SDF_3D_SEG, 6, 1, 1, 4, 811)
    ctx, sid = load(spec)
    for order in (1, -1, 11, 16, 17):                               # P = 3: order <= 10
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_readout_rule(sid, order)
        assert e.value.status == 1 and "order^P <= 1024" in str(e.value), order
        assert ctx.factors_readout_info(sid)["order"] == 0
    ctx.factors_set_readout_rule(sid, 10)
    assert ctx.factors_readout_info(sid) == dict(order=10, P=3, J=1, points_per_check_point=1000)
    with pytest.raises(api.GviError):
        ctx.factors_set_readout_rule(sid, 11)
    assert ctx.factors_readout_info(sid)["order"] == 10              # a refusal leaves the set as it was
    with pytest.raises(api.GviError):
        ctx.factors_set_readout_rule(sid + 1, 4)
    ctx.close()
    spec2, _, _, _ = draw_case(api.PSI_HINGE_SDF_2D, 4, 1, 1, 4, 812)
    ctx, sid = load(spec2)
    for order in (16, 2):
        ctx.factors_set_readout_rule(sid, order)
    with pytest.raises(api.GviError):
        ctx.factors_set_readout_rule(sid, 17)
    ctx.close()
    # kinds without a linear read-out
    ctx = api.Context(0)
    ctx.chain_set(1, 4)
    K = 2
    others = [(api.PSI_FIXED_PRIOR, np.concatenate([np.zeros((K, 4)), np.tile(np.eye(4).ravel(), (K, 1))], axis=1)),
              (api.PSI_HOST_CALLBACK, None), (api.PSI_HINGE_SDF_2D_BODY, np.tile([15.5, 0.5, 0.3, 5.0, 5.0, 1.0], (K, 1))),
              (api.PSI_HINGE_BOX, np.tile(syn.box_params(2.0, 0.1, np.full(4, -1.0), np.full(4, 1.0)), (K, 1))),
              (api.PSI_HINGE_HALFSPACE, np.tile(syn.halfspace_params(2.0, 0.1, 1.0, np.ones((1, 4))), (K, 1)))]
    for kind, prm in others:
        sid = ctx.factors_add(4, 3, np.zeros(K, dtype=np.int32), kind, prm)
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_readout_rule(sid, 4)
        assert e.value.status == 1 and "linear read-outs" in str(e.value), kind
        assert ctx.factors_readout_info(sid) == dict(order=0, P=0, J=0, points_per_check_point=0)
    empty = ctx.factors_add(4, 3, np.zeros(0, dtype=np.int32), api.PSI_HINGE_SDF_2D, np.zeros((0, 3)))
    ctx.factors_set_readout_rule(empty, 8)                            # an empty set accepts the call
    assert ctx.factors_readout_info(empty)["order"] == 8
    ctx.close()


# ---- 7. iterations ----
class ReadoutProx(box_gpu.ClosedProx):
    """box_gpu.ClosedProx with the raw integrals of a rule-on set from readout_ref."""

    def raw(self, fs, mk, Sk):
        if getattr(fs, "readout_spec", None) is not None:
            return rr.spec_moments(fs.readout_spec, mk, Sk, fs.readout_spec["readout_order"], 1.0)
        return o.batched_moments(fs.Z, fs.w, mk, Sk, fs.psi_batch, 1.0)


def attach_oracle(ch):
    """tests/chains.py's glue: a set with readout_order gets readout_ref's moments as fast_moments."""
    from chains import oracle_psi_batch
    for spec in ch["specs"]:
        spec["psi_batch"] = sr.spec_psi_batch(spec) if spec["kind"] in SEG else br.spec_psi_batch(spec) if spec["kind"] in BALLS else oracle_psi_batch(spec)

    def oracle_sets():
        out = []
        for spec in ch["specs"]:
            fs = o.FactorSet(spec["start"], spec["d"], spec["p"], spec["psi_batch"])
            fs.temperature = np.asarray(spec["temperature"], dtype=np.float64)
            if spec.get("readout_order"):
                fs.fast_moments = rr.fast_moments(spec, spec["readout_order"])
                fs.readout_spec = spec
            out.append(fs)
        return out
    ch["oracle_sets"] = oracle_sets
    return ch


@functools.lru_cache(maxsize=None)
def graph(name):
    """seg: planar at T = 9 with a _2D_SEG set (d = 8, J = 3) at order 8, sets = priors, obstacles, segments, anchors.
    balls: the crossing-ball graph of tests/test_balls_gpu.py (binary, d = 8, J = 3) at order 8.
    planar3: the three-set planning graph with the rule on its obstacle set."""
    if name == "seg":
        return attach_oracle(syn.make_planar_chain(T=9, p=3, segment_taus=[0.0625, 0.125, 0.1875], readout_order=8))
    if name == "balls":
        import test_balls_gpu as bg
        base = syn.make_planar_chain(T=9, p=3)
        pri, _, anc = base["specs"]
        B = bg.BALL
        return attach_oracle(syn.add_moving_obstacle_set(dict(base, specs=[pri, anc]), B["centre0"], B["velocity"], B["radius"], sigma=B["sigma"], eps=B["eps"],
                                                         r=B["r"], p=3, taus=bg.TAUS, dt=bg.DT, temperature=B["temperature"], readout_order=8))
    ch = syn.make_planar_chain(T=9, p=3)
    ch["specs"][1]["readout_order"] = 8
    return attach_oracle(ch)


def check_state(ctx, chain, tag):
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D), rel(st["SigD"], chain.SigD)]
    print(f"{tag}: mu {errs[0]:.2e}, D {errs[1]:.2e}, SigD {errs[2]:.2e}")
    assert max(errs) <= 1e-7, (tag, errs)


@pytest.mark.parametrize("name", ["seg", "balls"])
def test_ngd_iterations_vs_oracle(name):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    rule_on = [i for i, s in zip(ids, ch["specs"]) if s.get("readout_order")]
    assert len(rule_on) == 1 and ctx.factors_readout_info(rule_on[0])["order"] == 8
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    log = []
    for it in range(5):
        r = ctx.ngd_step(0.55, 10)
        ok, cost, ntr = chain.step()
        print(f"{name} iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
        check_state(ctx, chain, f"{name} iteration {it}")
        log.append(r)
    assert ctx.profile_geometry(rule_on[0])["variant"] == 8
    assert ctx.ngd_factor_costs(rule_on[0]).max() > 0
    state = ctx.ngd_get_state()
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])                       # the same iterations in one call
    assert ctx.ngd_run(5, 0.55, 10) == log
    st = ctx.ngd_get_state()
    assert all(np.array_equal(st[k], state[k]) for k in state)
    ctx.close()


@pytest.mark.parametrize("name", ["seg", "balls"])
def test_prox_step_vs_oracle(name):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = ReadoutProx(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.3)
    r = ctx.prox_step(0.3, 10)
    ok, cost, ntr = chain.step()
    print(f"{name}: device {r}, oracle {(ok, cost, ntr)}")
    assert r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D)]
    print(f"{name}: mu {errs[0]:.2e}, D {errs[1]:.2e}")
    assert max(errs) <= 1e-7
    ctx.close()


def test_planar_graph_with_the_rule_takes_one_launch_per_set():
    """The three-set planning graph with the rule on its obstacle set: no factor_block3_kernel launch, and two iterations match
    the oracle."""
    ch = graph("planar3")
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    before = api.block3_launches()
    for it in range(2):
        r = ctx.ngd_step(0.55, 10)
        ok, cost, ntr = chain.step()
        print(f"planar3 iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
        check_state(ctx, chain, f"planar3 iteration {it}")
    assert api.block3_launches() == before
    assert ctx.profile_geometry(ids[1])["variant"] == 8
    ctx.close()
    # the same graph without the rule does take the one-launch factor stage: the counter can see it
    plain = syn.make_planar_chain(T=9, p=3)
    ctx, ids = api.context_for_chain(plain)
    ctx.ngd_init(plain["mu0"], plain["D0"], plain["U0"])
    ctx.ngd_step(0.55, 10)
    assert api.block3_launches() > before
    ctx.close()


def test_shim_readout_callsite(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "readout_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "readout_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "device"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
