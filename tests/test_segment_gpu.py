"""Obstacle factors on the segment between two support states (GVI_PSI_HINGE_SDF_2D_SEG / _3D_SEG) on
the device, against the numpy reference of tests/segment_ref.py plugged into the oracle (o.batched_moments, o.ChainNGD,
o.ChainProx).

Bounds, max-norm relative (rel of tests/test_gpu_parity.py): operators 1e-9 (Vddmu, E_xxphi 1e-8) -- TIGHT of that file; the
register and the generic route against each other 1e-12 (same table, same prep and epilogue, sums of <= 849 terms in another
order); chain iterates 1e-7 (RTOL / 10) and costs 1e-9; sample costs and clearance 1e-8 (non-polynomial
kinds)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o
import segment_ref as sr
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import RTOL, TIGHT, rel
from test_sample_cost_host import factor_slices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.25
TAUS = [DT / 4, DT / 2, 3 * DT / 4]
KIND = {2: api.PSI_HINGE_SDF_2D_SEG, 3: api.PSI_HINGE_SDF_3D_SEG}
REG = {2: (4, 8, 12), 3: (6,)}            # dimensions with a register instance (PsiHingeSeg); every other d: generic kernel

FIELD2 = dict(origin=(-5.0, -4.0), cell=0.1)
FIELD2["field"] = syn.circle_sdf(FIELD2["origin"], 0.1, 81, 101, [(0.0, 1.6), (-1.0, -2.2)], [1.2, 0.9])
FIELD3 = dict(origin=(-4.0, -3.0, -2.0), cell=0.2)
FIELD3["field"] = syn.sphere_sdf3d(FIELD3["origin"], 0.2, 31, 41, 21, [(0.0, 1.4, 0.3), (-0.5, -1.8, 0.0)], [1.0, 0.8])
# (first pose, last pose) of a factor: 0 crosses an obstacle with both ends clear, 1 inside, 2 and 5 on a rim, 3 far, 4 outside
# the grid (clamped), 6 and 7 pass by
ENDS2 = [((-2.0, 1.6), (2.0, 1.6)), ((0.0, 1.5), (0.2, 1.4)), ((0.1, 0.2), (0.3, 0.4)), ((3.0, 3.0), (3.5, 3.0)),
         ((6.5, 0.0), (7.0, 0.5)), ((-1.0, -1.2), (-1.0, -1.0)), ((-0.3, 2.9), (0.5, 3.1)), ((2.0, -1.0), (-2.5, -2.0))]
ENDS3 = [((-2.0, 1.4, 0.3), (2.0, 1.4, 0.3)), ((0.0, 1.3, 0.3), (0.2, 1.2, 0.2)), ((0.0, 0.2, 0.3), (0.2, 0.1, 0.3)),
         ((3.0, -2.0, 1.5), (3.2, -2.0, 1.0)), ((5.5, 0.0, 0.0), (6.0, 0.5, 0.0)), ((-0.5, -0.8, 0.0), (-0.4, -0.9, 0.1)),
         ((-0.3, 2.6, 0.5), (0.5, 2.7, 0.6)), ((2.0, -1.0, 0.0), (-2.5, -2.0, 0.0))]


def field_of(P):
    return FIELD2 if P == 2 else FIELD3


def set_field(ctx, sid, P):
    F = field_of(P)
    (ctx.factors_set_sdf2d if P == 2 else ctx.factors_set_sdf3d)(sid, F["origin"], F["cell"], F["field"])


def operator_case(P, d, J, K, seed=0):
    """Per-factor W, c, sigma, eps, r, temperature and marginals of K factors with J check points between the poses of ENDS:
    a binary factor (d = 8, 12: n = d / 2) reads them from its two states, a unary one (n = d) from its state plus c_j."""
    rng = np.random.default_rng(1000 * P + 10 * d + J + 100 * K + seed)
    binary = d in (8, 12)
    n = d // 2 if binary else d
    ends = np.array((ENDS2 if P == 2 else ENDS3)[:K])
    a = (np.arange(J) + 1.0) / (J + 1.0)
    W = 0.02 * rng.normal(size=(K, J, P, d))
    c = 0.02 * rng.normal(size=(K, J, P))
    for j in range(J):
        for r in range(P):
            if binary:
                W[:, j, r, r] += 1.0 - a[j]
                W[:, j, r, n + r] += a[j]
            else:
                W[:, j, r, r] += 1.0
                c[:, j, r] += a[j] * (ends[:, 1, r] - ends[:, 0, r])
    head = np.stack([rng.uniform(5, 20, K), rng.uniform(0.1, 0.25, K), rng.uniform(0.05, 0.12, K)], axis=1)
    params = syn.segment_params(head[:, 0], head[:, 1], head[:, 2], W, c)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.2)
    mu[:, :P] = ends[:, 0]
    if binary:
        mu[:, n:n + P] = ends[:, 1]
    return dict(P=P, d=d, n=n, J=J, K=K, binary=binary, params=params, head=head, mu=mu, Sigma=Sigma,
                temperature=rng.uniform(0.5, 5.0, K))


def seg_ctx(case, p):
    ctx = api.Context(0)
    ctx.chain_set(2 if case["binary"] else 1, case["n"])
    sid = ctx.factors_add(case["d"], p, np.zeros(case["K"], dtype=np.int32), KIND[case["P"]], case["params"], case["temperature"])
    return ctx, sid


SHAPES = [(2, 4, 4), (2, 8, 3), (2, 8, 4), (2, 12, 3), (2, 6, 3), (3, 6, 3), (3, 12, 3), (3, 8, 3)]


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("J", [1, 3, 8])
@pytest.mark.parametrize("P,d,p", SHAPES)
def test_operators_vs_oracle(P, d, p, J, K):
    """gvi_moments, gvi_costs and gvi_raw_moments of one segment set: the register instances (2-D at d = 4, 8, 12; 3-D at d = 6)
    and the generic kernel (every other d, and every d under variant 1), each against the oracle and against each other."""
    case = operator_case(P, d, J, K)
    F = field_of(P)
    mu, Sigma = case["mu"], case["Sigma"]
    psi = sr.psi_batch_hinge_seg(case["params"], P, d, F["origin"], F["cell"], F["field"])
    Z, w = o.nwspgr_cached(d, p)
    r = o.batched_moments(Z, w, mu, Sigma, psi, case["temperature"])
    assert np.abs(r["E_phi"]).max() > 0.05
    if case["binary"] and J == 3:
        # the case the feature exists for: both end poses of factor 0 are outside the hinge, the middle check point is inside
        # the obstacle, and psi at the mean is positive
        look = o.planar_sdf_lookup if P == 2 else o.sdf3d_lookup
        n, thr = case["n"], case["head"][0, 1] + case["head"][0, 2]
        sd_ends = [look(*mu[0, e:e + P], F["origin"], F["cell"], F["field"]) for e in (0, n)]
        sd_mid = sr.check_point_distances(case["params"], P, d, F["origin"], F["cell"], F["field"], mu[:, None, :])[0, 1, 0]
        print(f"factor 0: sd at the ends {sd_ends[0]:.3f}, {sd_ends[1]:.3f} (threshold {thr:.3f}), at the middle check point {sd_mid:.3f}")
        psi_mean = psi(mu[:, None, :])[0, 0]
        assert min(sd_ends) > thr and sd_mid < 0 and psi_mean > 0.05
    ctx, sid = seg_ctx(case, p)
    set_field(ctx, sid, P)
    reg = d in REG[P]
    out = {}
    for variant in (0, 1):
        ctx.set_variant(variant)
        Ephi, Vdmu, Vddmu = ctx.moments(sid, mu, Sigma)
        geo = ctx.profile_geometry(sid)
        assert geo["variant"] == (2 if reg and variant == 0 else 1), geo
        if (P, d, p) == (2, 8, 4) and K == 1 and variant == 0:
            assert geo["nchunk"] > 1, geo                  # 849 points = four 256-point tiles: one factor, several chunks
        cost = ctx.costs(sid, mu, Sigma)
        E0, E1, E2 = ctx.raw_moments(sid, mu, Sigma)
        errs = dict(Ephi=rel(Ephi, r["E_phi"]), Vdmu=rel(Vdmu, r["Vdmu"]), Vddmu=rel(Vddmu, r["Vddmu"]), cost=rel(cost, r["cost"]),
                    E0=rel(E0, r["E_phi"]), E1=rel(E1, r["E_xmuphi"]), E2=rel(E2, r["E_xxphi"]))
        print(f"P {P} d {d} p {p} J {J} K {K} variant {variant} -> kernel {geo['variant']}, chunks {geo['nchunk']}: " +
              ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < (TIGHT * 10 if k in ("Vddmu", "E2") else TIGHT), (k, v)
        out[variant] = (Ephi, Vdmu, Vddmu, cost, E0, E1, E2)
    if reg:
        gap = max(rel(a, b) for a, b in zip(out[0], out[1]))
        print(f"register against generic: {gap:.2e}")
        assert gap <= 1e-12, gap
    ctx.set_variant(2)                                         # the register kernel on demand: refused where none exists
    if reg:
        ctx.moments(sid, mu, Sigma)
    else:
        with pytest.raises(api.GviError) as e:
            ctx.moments(sid, mu, Sigma)
        assert e.value.status == 3
    ctx.close()


@pytest.mark.parametrize("P,d,p", [(2, 4, 4), (3, 6, 3)])
def test_degenerate_set_equals_the_single_point_kind(P, d, p):
    """J = 1, W = [I 0], c = 0 against PSI_HINGE_SDF_2D / _3D at the same d on the same marginals."""
    rng = np.random.default_rng(40 + d)
    K = 6
    F = field_of(P)
    head = np.stack([rng.uniform(5, 20, K), rng.uniform(0.2, 0.8, K), rng.uniform(0.1, 0.5, K)], axis=1)
    W = np.zeros((1, P, d))
    W[0, :, :P] = np.eye(P)
    params = syn.segment_params(head[:, 0], head[:, 1], head[:, 2], W, np.zeros((1, P)))
    mu, Sigma = syn.random_marginals(rng, K, d, 0.2)
    mu[:, :P] = np.array((ENDS2 if P == 2 else ENDS3)[:K])[:, 0]
    ctx = api.Context(0)
    ctx.chain_set(1, d)
    start = np.zeros(K, dtype=np.int32)
    seg = ctx.factors_add(d, p, start, KIND[P], params)
    one = ctx.factors_add(d, p, start, api.PSI_HINGE_SDF_2D if P == 2 else api.PSI_HINGE_SDF_3D, head)
    for sid in (seg, one):
        set_field(ctx, sid, P)
    a, b = ctx.moments(seg, mu, Sigma), ctx.moments(one, mu, Sigma)
    assert ctx.profile_geometry(seg)["variant"] == 2 and ctx.profile_geometry(one)["variant"] == 2
    ca, cb = ctx.costs(seg, mu, Sigma), ctx.costs(one, mu, Sigma)
    assert np.abs(b[0]).max() > 0.05
    gap = max([rel(x, y) for x, y in zip(a, b)] + [rel(ca, cb)])
    bits = all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ca, cb)
    print(f"P {P} d {d}: segment set against the single-point kind {gap:.2e}; bit-equal: {bits}")
    assert gap <= 1e-13, gap
    ctx.close()


def test_argument_rules():
    rng = np.random.default_rng(5)
    ctx = api.Context(0)
    ctx.chain_set(2, 4)
    start = np.zeros(2, dtype=np.int32)
    for P, d in ((2, 8), (2, 4), (3, 8)):
        per = P * (d + 1)
        for width in (3 + per + 1, 3 + per - 1, 3, 3 + 9 * per, 2):           # ragged (twice), J = 0, J = 9, too short
            with pytest.raises(api.GviError) as e:
                ctx.factors_add(d, 3, start, KIND[P], rng.normal(size=(2, width)))
            assert e.value.status == 1, (P, d, width)
            if width > 2:
                assert "J P (d + 1)" in str(e.value) and "1 <= J <= 8" in str(e.value)
        for J in (1, 8):
            ctx.factors_add(d, 3, start, KIND[P], rng.normal(size=(2, 3 + J * per)))
    with pytest.raises(api.GviError) as e:                                    # no parameter block at all
        ctx.factors_add(8, 3, start, KIND[2], None)
    assert e.value.status == 1
    assert len(ctx.sets) == 6
    ctx.close()
    case = operator_case(2, 8, 3, 2)
    ctx, s2 = seg_ctx(case, 3)
    s3 = ctx.factors_add(8, 3, np.zeros(2, dtype=np.int32), KIND[3], operator_case(3, 8, 3, 2)["params"])
    for sid in (s2, s3):                                                      # no grid yet: as for the existing kinds
        with pytest.raises(api.GviError) as e:
            ctx.moments(sid, case["mu"], case["Sigma"])
        assert e.value.status == 5
        with pytest.raises(api.GviError) as e:
            ctx.sample_clearance(sid, np.zeros((1, 2, 4)))
        assert e.value.status == 5
    with pytest.raises(api.GviError) as e:                                    # the wrong setter for the kind
        set_field(ctx, s2, 3)
    assert e.value.status == 1
    with pytest.raises(api.GviError) as e:
        set_field(ctx, s3, 2)
    assert e.value.status == 1
    set_field(ctx, s2, 2)
    set_field(ctx, s3, 3)
    assert np.isfinite(ctx.moments(s2, case["mu"], case["Sigma"])[0]).all()
    assert np.isfinite(ctx.moments(s3, case["mu"], case["Sigma"])[0]).all()
    ctx.close()


@functools.lru_cache(maxsize=None)
def graph(name):
    """planar / pr3d at T = 9 with a J = 3 segment set behind the obstacle set; the oracle closures attached.  pr3d runs its
    obstacle and segment sets at the high temperature the planning benchmarks use (synthetic.make_chain, "planar1k"): at
    temperature 1 the oracle itself backtracks 9 or 10 times per iteration on this graph, and an accept decision that close to
    the end of the line search says little about either implementation."""
    if name == "planar":
        ch = syn.make_planar_chain(T=9, p=3, segment_taus=TAUS)
    else:
        ch = syn.make_obstacle_chain("pr3d", T=9, segment_taus=TAUS, segment_p=3)
        for spec in ch["specs"][1:3]:
            spec["temperature"] = np.full(len(spec["start"]), 30.0)
    return sr.attach_oracle(ch)


def check_state(ctx, chain, tag):
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D), rel(st["SigD"], chain.SigD)]
    print(f"{tag}: mu {errs[0]:.2e}, D {errs[1]:.2e}, SigD {errs[2]:.2e}")
    assert max(errs) < RTOL / 10, (tag, errs)


@pytest.mark.parametrize("name", ["planar", "pr3d"])
def test_graph_ngd_iterations_vs_oracle(name):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    before = api.asm_launches()
    log = []
    for it in range(5):
        r = ctx.ngd_step(0.55, 10)
        ok, cost, ntr = chain.step()
        print(f"{name} iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
        check_state(ctx, chain, f"{name} iteration {it}")
        log.append(r)
    after = api.asm_launches()
    assert sum(after) > sum(before), (before, after)            # the chain launches assembled while loading
    geo = ctx.profile_geometry(ids[2])
    assert geo["variant"] == (2 if name == "planar" else 1)     # d = 8: PsiHingeSeg<8, 2>; 3-D d = 12: the generic kernel
    fc = ctx.ngd_factor_costs(ids[2])
    assert fc.shape == (ch["T"] - 1,) and fc.max() > 0           # the segment factors are active on this path
    state = ctx.ngd_get_state()
    # the same five iterations in one call (pipelined where the graph allows it)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    assert ctx.ngd_run(5, 0.55, 10) == log
    st = ctx.ngd_get_state()
    assert all(np.array_equal(st[k], state[k]) for k in state)
    ctx.close()


def test_pr3d_graph_as_built_first_iteration_vs_oracle():
    """The pr3d graph exactly as the builder returns it (temperature 1, segment set at the obstacle factors' degree, (12, 4) =
    2649 points on the generic kernel): the first iteration, which the oracle accepts at its first trial.  From the second
    iteration on the oracle exhausts its line search at this temperature, which is why graph("pr3d") raises it."""
    ch = sr.attach_oracle(syn.make_obstacle_chain("pr3d", T=9, segment_taus=TAUS))
    assert ch["specs"][2]["p"] == 4 and (ch["specs"][2]["temperature"] == 1).all()
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    r = ctx.ngd_step(0.55, 10)
    ok, cost, ntr = chain.step()
    print(f"pr3d as built: device {r}, oracle {(ok, cost, ntr)}")
    assert ok and ntr == 1 and r["accepted"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
    check_state(ctx, chain, "pr3d as built")
    assert ctx.ngd_factor_costs(ids[2]).max() > 0
    ctx.close()


@pytest.mark.parametrize("name", ["planar", "pr3d"])
def test_graph_prox_step_vs_oracle(name):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    # base 0.3: the oracle's line search ends on a decrease (7 and 6 trials); at 0.55 it is exhausted on both graphs
    chain = o.ChainProx(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.3)
    r = ctx.prox_step(0.3, 10)
    ok, cost, ntr = chain.step()
    print(f"{name}: device {r}, oracle {(ok, cost, ntr)}")
    assert ok and r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D)]
    print(f"{name}: mu {errs[0]:.2e}, D {errs[1]:.2e}")
    assert max(errs) < RTOL / 10
    ctx.close()


def support_time_graphs():
    """A: priors + a J = 1 segment set at tau = 0 + anchors.  B: the same priors + a unary HINGE_SDF_2D set on states
    0 .. T - 2 at the same GH degree + anchors.  psi_A(x_i, x_i+1) = psi_B(x_i) pointwise."""
    base = syn.make_planar_chain(T=9, p=3, segment_taus=[0.0], segment_p=3)
    pri, ob, seg, anc = base["specs"]
    K = base["T"] - 1
    unary = dict(ob, p=3, start=ob["start"][:K], params=ob["params"][:K], temperature=ob["temperature"][:K])
    A = sr.attach_oracle(dict(base, specs=[pri, seg, anc]))
    B = sr.attach_oracle(dict(base, specs=[dict(pri), unary, dict(anc)]))
    return A, B


def test_support_time_identity():
    A, B = support_time_graphs()
    W = A["specs"][1]["seg_W"]
    assert W.shape == (1, 2, 8) and np.array_equal(W[0], np.eye(2, 8))
    sampler = api.Context(0)
    sampler.chain_set(A["T"], A["n"])
    X = sampler.bt_sample(A["D0"], A["U0"], A["mu0"], 33, seed=77)
    sampler.close()
    J = []
    for tag, ch in (("A", A), ("B", B)):
        ctx, ids = api.context_for_chain(ch)
        J.append(ctx.sample_costs(X))
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
        for it in range(3):
            r = ctx.ngd_step(0.55, 10)
            ok, cost, ntr = chain.step()
            assert r["accepted"] == ok and r["ntrials"] == ntr
            assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
            check_state(ctx, chain, f"graph {tag} iteration {it}")
        assert ctx.ngd_factor_costs(ids[1]).max() > 0
        ctx.close()
    gap = rel(J[0], J[1])
    print(f"sample costs of the two graphs on the same samples: {gap:.2e}")
    assert np.isfinite(J[0]).all() and gap <= 1e-12, gap


@pytest.mark.parametrize("name", ["planar", "pr3d"])
def test_sample_costs_and_clearance(name):
    ch = graph(name)
    T, n, S = ch["T"], ch["n"], 33
    seg = ch["specs"][2]
    ctx, ids = api.context_for_chain(ch)
    X = ctx.bt_sample(ch["D0"], ch["U0"], ch["mu0"], S, seed=4100)
    Xk = factor_slices(X, seg, n)
    ref_cost = (seg["psi_batch"](Xk) / np.asarray(seg["temperature"])[:, None]).T
    ref_clr = sr.spec_clearance(seg, Xk).T
    share = float((ref_cost > 0).mean())
    print(f"{name}: share of (sample, factor) pairs with psi > 0: {share:.3f}; clearance min {ref_clr.min():.3f}")
    assert 0.03 <= share <= 0.97, "both hinge branches must be exercised"
    cost = ctx.sample_factor_costs(ids[2], X)
    clr = ctx.sample_clearance(ids[2], X)
    errs = (rel(cost, ref_cost), rel(clr, ref_clr))
    print(f"{name}: cost {errs[0]:.2e}, clearance {errs[1]:.2e}")
    assert cost.shape == (S, T - 1) and clr.shape == (S, T - 1) and max(errs) <= 1e-8, errs
    # J and the minimum clearance are consistent with the per-set rows
    rows = [ctx.sample_factor_costs(sid, X) for sid in ids]
    Jrows = np.sum([r.sum(axis=1) for r in rows], axis=0)
    J = ctx.sample_costs(X)
    assert np.abs(J - Jrows).max() <= 1e-10 * np.abs(Jrows).max()
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    r = ctx.ngd_sample_costs(S, seed=5, clearance_set=ids[2])
    assert np.array_equal(r["clr_min"], ctx.sample_clearance(ids[2], r["X"]).min(axis=1))
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    # a NaN in state i: factors i - 1 and i of the segment set give NaN, the rest stay as they were
    i = 4
    Xb = X.copy()
    Xb[2, i, 1] = np.nan
    bad = np.zeros((S, T - 1), dtype=bool)
    bad[2, i - 1:i + 1] = True
    for got, clean in ((ctx.sample_factor_costs(ids[2], Xb), cost), (ctx.sample_clearance(ids[2], Xb), clr)):
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean[~bad]) and np.isfinite(got[~bad]).all()
    Jb = ctx.sample_costs(Xb)
    assert np.isnan(Jb[2]) and np.array_equal(np.delete(Jb, 2), np.delete(J, 2))
    ctx.close()


def test_shim_segment_callsite(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "segment_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "segment_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
