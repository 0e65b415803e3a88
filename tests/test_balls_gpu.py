"""Moving obstacles as analytic balls (GVI_PSI_HINGE_BALLS_2D / _3D) on the device, against the numpy
reference of tests/balls_ref.py plugged into the oracle (o.batched_moments, o.ChainNGD, o.ChainProx), and
gvi_factors_set_params.

Bounds, max-norm relative (rel of tests/test_gpu_parity.py), the numbers tests/test_segment_gpu.py uses: operators 1e-9 (Vddmu,
E_xxphi 1e-8) -- TIGHT of that file; the register and the generic route against each other 1e-12 (same table, same prep and
epilogue, sums of <= 849 terms in another order); chain iterates 1e-7 (RTOL / 10) and costs 1e-9; sample costs and clearance
1e-8; identities 1e-13 or bit-equal."""
import functools
import os
import subprocess

import numpy as np
import pytest

import balls_ref as br
import gvi_oracle as o
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import RTOL, TIGHT, rel
from test_sample_cost_host import factor_slices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.25
TAUS = [DT / 4, DT / 2, 3 * DT / 4]
KIND = {2: api.PSI_HINGE_BALLS_2D, 3: api.PSI_HINGE_BALLS_3D}
REG = {2: (2, 4, 8, 12), 3: (3, 6, 12)}    # dimensions with a register instance (PsiHingeBalls); every other d: generic kernel
SLOT_ORDER = [5, 2, 7, 0, 3, 6, 1, 4]      # where the operator cases put their slots: live balls in any position
SHAPES = [(2, 2, 4), (2, 4, 4), (2, 8, 3), (2, 8, 4), (2, 12, 3), (2, 6, 3), (3, 3, 3), (3, 6, 3), (3, 12, 3), (3, 8, 3)]
ACTIVE = (0, 1, 3, 8)


def permute_slots(params, P, order):
    """The same blocks with slot m moved to position order[m]."""
    params = np.array(params, dtype=np.float64)
    tail = 8 * (2 * P + 1)
    slots = params[:, -tail:].reshape(len(params), 8, 2 * P + 1).copy()
    out = np.empty_like(slots)
    out[:, order] = slots
    params[:, -tail:] = out.reshape(len(params), -1)
    return params


def operator_case(P, d, J, K, M, seed=0, p=3):
    """The first draw of draw_case whose share of sigma points (degree p) with psi > 0 lies in [0.1, 0.9], judged by the reference
    alone: with eight balls around eight check points nearly every draw of some shapes has every sigma point inside a hinge."""
    for attempt in range(50):
        case = draw_case(P, d, J, K, M, seed + 7919 * attempt)
        if M == 0 or 0.1 <= input_properties(case, p)[0] <= 0.9:
            return case
    raise AssertionError("no draw with both hinge branches")


def draw_case(P, d, J, K, M, seed):
    """K factors with J check points and M live balls each.  A binary factor (d = 8, 12: n = d / 2) reads its check points
    from its two states, a unary one (n = d) from its state plus c_j.  Check point 0 of factor k sits at the distance
    R_0 + eps + r + delta_k from the centre of its ball 0 at that check point's time, i.e. delta_k off the hinge boundary at
    the mean: with K > 1 delta = +5e-7 (factor 0) and -5e-7 (factor 1) and draws from [-0.25, -0.05] for the others, +0.03 for the
    one factor of K = 1, so that a good part of the sigma points is inside the hinge and, with one ball, the centre sigma points of factors 0 and 1 lie within 1e-6
    of the boundary on either side."""
    rng = np.random.default_rng(100000 * P + 1000 * d + 100 * J + 10 * K + M + seed)
    binary = d in (8, 12)
    n = d // 2 if binary else d
    a = (np.arange(J) + 1.0) / (J + 1.0)
    W = 0.02 * rng.normal(size=(K, J, P, d))
    c = 0.02 * rng.normal(size=(K, J, P))
    u = _unit(rng, (K, P))                  # the direction from ball 0 to check point 0; the later check points lie further out
    step = 0.3 * u
    for j in range(J):
        for r in range(P):
            if binary:
                W[:, j, r, r] += 1.0 - a[j]
                W[:, j, r, n + r] += a[j]
            else:
                W[:, j, r, r] += 1.0
                c[:, j, r] += a[j] * step[:, r]
    tau = rng.uniform(-0.2, 0.2, (K, J))
    head = np.stack([rng.uniform(5, 20, K), rng.uniform(0.1, 0.25, K), rng.uniform(0.05, 0.12, K)], axis=1)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.2)
    if binary:
        mu[:, n:n + P] = mu[:, :P] + step
    centres = rng.uniform(-1.5, 1.5, (K, M, P))
    vel = rng.uniform(-1.0, 1.0, (K, M, P))
    radii = rng.uniform(0.3, 0.8, (K, M))
    if M:
        delta = rng.uniform(-0.25, -0.05, K)
        delta[:2] = [5e-7, -5e-7] if K > 1 else [0.03]
        thr = head[:, 1] + head[:, 2]
        q0 = np.einsum("kpd,kd->kp", W[:, 0], mu) + c[:, 0]
        at = centres[:, 0] + tau[:, 0, None] * vel[:, 0] + u * (radii[:, 0] + thr + delta)[:, None]       # where check point 0 goes
        c[:, 0] += at - q0
        if M > 1:       # the other balls stand around that place, their hinges up to 1.2 away from it (K = 1: at least 0.5, or
            #             the one factor's check points, 0.3 apart, would all lie in some hinge at every sigma point)
            off = radii[:, 1:] + thr[:, None] + rng.uniform(0.5 if K == 1 else 0.0, 1.2, (K, M - 1))
            centres[:, 1:] = at[:, None, :] + off[:, :, None] * _unit(rng, (K, M - 1, P)) - tau[:, 0, None, None] * vel[:, 1:]
    params = permute_slots(syn.balls_params(head[:, 0], head[:, 1], head[:, 2], W, c, tau, centres, vel, radii), P, SLOT_ORDER)
    return dict(P=P, d=d, n=n, J=J, K=K, M=M, binary=binary, params=params, head=head, mu=mu, Sigma=Sigma,
                temperature=rng.uniform(0.5, 5.0, K))


def _unit(rng, shape):
    v = rng.normal(size=shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sigma_points(case, p):
    Z, _ = o.nwspgr_cached(case["d"], p)
    S = np.stack([o.sym_sqrt(s) for s in case["Sigma"]])
    return np.einsum("na,kba->knb", Z, S) + case["mu"][:, None, :]


def input_properties(case, p):
    """(share of sigma points with psi > 0, smallest sd - thr > 0, largest sd - thr < 0 over every check point of every sigma
    point) from the reference alone."""
    X = sigma_points(case, p)
    psi = br.psi(case["params"], case["P"], case["d"], X)
    gap = br.check_point_distances(case["params"], case["P"], case["d"], X) - (case["head"][:, 1] + case["head"][:, 2])[:, None, None]
    out, ins = gap[gap > 0], gap[gap < 0]
    return float((psi > 0).mean()), (out.min() if out.size else np.inf), (ins.max() if ins.size else -np.inf)


def balls_ctx(case):
    ctx = api.Context(0)
    ctx.chain_set(2 if case["binary"] else 1, case["n"])
    return ctx


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("J", [1, 3, 8])
@pytest.mark.parametrize("P,d,p", SHAPES)
def test_operators_vs_oracle(P, d, p, J, K):
    """(a) gvi_moments, gvi_costs and gvi_raw_moments of one ball set with 0, 1, 3 and 8 live balls (four sets of one context):
    the register instances (2-D at d = 2, 4, 8, 12; 3-D at d = 3, 6, 12) and the generic kernel (every other d, and every d
    under variant 1), each against the oracle and against each other."""
    reg = d in REG[P]
    Z, w = o.nwspgr_cached(d, p)
    cases = [operator_case(P, d, J, K, M, p=p) for M in ACTIVE]
    ctx = balls_ctx(cases[0])
    start = np.zeros(K, dtype=np.int32)
    for case in cases:
        M, mu, Sigma = case["M"], case["mu"], case["Sigma"]
        # the inputs, checked with the reference alone
        share, out, ins = input_properties(case, p)
        print(f"P {P} d {d} p {p} J {J} K {K} M {M}: share of sigma points with psi > 0 {share:.3f}, nearest to a boundary +{out:.1e} / {ins:.1e}")
        if M:
            assert 0.03 <= share <= 0.97, "both hinge branches must run"
        else:
            assert share == 0.0
        if M == 1 and K >= 5:
            assert 0 < out < 1e-6 and -1e-6 < ins < 0, "a sigma point on each side of a hinge boundary"
        r = o.batched_moments(Z, w, mu, Sigma, br.psi_batch_hinge_balls(case["params"], P, d), case["temperature"])
        assert (np.abs(r["E_phi"]).max() > 1e-3) == (M > 0)
        sid = ctx.factors_add(d, p, start, KIND[P], case["params"], case["temperature"])
        res = {}
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
            print(f"  variant {variant} -> kernel {geo['variant']}, chunks {geo['nchunk']}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            for k, v in errs.items():
                assert v < (TIGHT * 10 if k in ("Vddmu", "E2") else TIGHT), (k, v)
            res[variant] = (Ephi, Vdmu, Vddmu, cost, E0, E1, E2)
            if M == 0:
                assert all((x == 0).all() for x in res[variant]), "every slot empty: exactly 0"
        if reg:
            gap = max(rel(x, y) for x, y in zip(res[0], res[1]))
            print(f"  register against generic: {gap:.2e}")
            assert gap <= 1e-12, gap
        ctx.set_variant(2)                                     # the register kernel on demand: refused where none exists
        if reg:
            ctx.moments(sid, mu, Sigma)
        else:
            with pytest.raises(api.GviError) as e:
                ctx.moments(sid, mu, Sigma)
            assert e.value.status == 3
    ctx.close()


def all_results(ctx, sid, mu, Sigma):
    out = []
    for variant in (0, 1):
        ctx.set_variant(variant)
        out += list(ctx.moments(sid, mu, Sigma)) + [ctx.costs(sid, mu, Sigma)]
    ctx.set_variant(0)
    return out


@pytest.mark.parametrize("P,d,p", [(2, 4, 4), (2, 8, 3), (3, 6, 3), (3, 8, 3)])
def test_slot_identities(P, d, p):
    """(b) Permuting the eight slots, and empty slots in any position: bit-equal on both routes.  Every slot empty: exactly 0."""
    J, K = 3, 5
    case = operator_case(P, d, J, K, 3)
    base = permute_slots(case["params"], P, np.argsort(SLOT_ORDER))                     # live slots 0, 1, 2
    assert (base[:, -1] == -np.inf).all() and (base[:, -(7 * (2 * P + 1)) - 1] != -np.inf).all()
    moved = [permute_slots(base, P, order) for order in ([7, 6, 5, 4, 3, 2, 1, 0], [1, 3, 6, 0, 2, 4, 5, 7], SLOT_ORDER)]
    empty = base.copy()
    empty.reshape(K, -1)[:, -8 * (2 * P + 1):].reshape(K, 8, 2 * P + 1)[:, :, 2 * P] = -np.inf
    ctx = balls_ctx(case)
    start = np.zeros(K, dtype=np.int32)
    ref = all_results(ctx, ctx.factors_add(d, p, start, KIND[P], base, case["temperature"]), case["mu"], case["Sigma"])
    assert np.abs(ref[0]).max() > 0.05
    for params in moved:
        got = all_results(ctx, ctx.factors_add(d, p, start, KIND[P], params, case["temperature"]), case["mu"], case["Sigma"])
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
    got = all_results(ctx, ctx.factors_add(d, p, start, KIND[P], empty, case["temperature"]), case["mu"], case["Sigma"])
    assert all((x == 0).all() for x in got)
    ctx.close()


@pytest.mark.parametrize("P,d,p", [(2, 4, 4), (3, 6, 3), (2, 6, 3)])
def test_moving_ball_equals_the_static_ball_at_its_place(P, d, p):
    """(b) J = 1: a ball (o, v, tau) against the static ball (o + tau v, 0, any tau)."""
    K = 5
    case = operator_case(P, d, 1, K, 3)
    u = br.unpack(permute_slots(case["params"], P, np.argsort(SLOT_ORDER)), P, d)
    at = u["o"][:, :3] + u["tau"][:, 0, None, None] * u["v"][:, :3]
    static = syn.balls_params(u["sigma"], u["eps"], u["r"], u["W"], u["c"], u["tau"] + 0.37, at, np.zeros_like(at), u["R"][:, :3])
    ctx = balls_ctx(case)
    start = np.zeros(K, dtype=np.int32)
    a = all_results(ctx, ctx.factors_add(d, p, start, KIND[P], case["params"], case["temperature"]), case["mu"], case["Sigma"])
    b = all_results(ctx, ctx.factors_add(d, p, start, KIND[P], static, case["temperature"]), case["mu"], case["Sigma"])
    gap = max(rel(x, y) for x, y in zip(a, b))
    print(f"P {P} d {d}: moving against static {gap:.2e}")
    assert np.abs(b[0]).max() > 0.05 and gap <= 1e-13, gap
    ctx.close()


@pytest.mark.parametrize("P,n", [(2, 4), (3, 6)])
def test_unary_set_equals_the_binary_set_that_reads_the_first_state(P, n):
    """(b) A unary set at d = n against the binary set at d = 2n whose W reads only the first state.  The two are the same
    function of the trajectory, which is what is compared: cost and clearance at the same samples.  Their Gauss-Hermite moments
    are sums over two different tables (d = n and d = 2n) of a non-polynomial psi and agree to the quadrature error only."""
    K, J, S = 5, 3, 33
    case = operator_case(P, n, J, K, 3)
    u = br.unpack(case["params"], P, n)
    W2 = np.concatenate([u["W"], np.zeros_like(u["W"])], axis=3)
    wide = syn.balls_params(u["sigma"], u["eps"], u["r"], W2, u["c"], u["tau"], u["o"], u["v"], u["R"])
    assert np.array_equal(br.unpack(wide, P, 2 * n)["R"], u["R"])
    rng = np.random.default_rng(77 + P)
    X = np.concatenate([case["mu"][None, :, :] + 0.3 * rng.normal(size=(S, K, n)), rng.normal(size=(S, 1, n))], axis=1)   # [S][K + 1][n]
    ctx = api.Context(0)
    ctx.chain_set(K + 1, n)
    one = ctx.factors_add(n, 3, np.arange(K, dtype=np.int32), KIND[P], case["params"], case["temperature"])
    two = ctx.factors_add(2 * n, 3, np.arange(K, dtype=np.int32), KIND[P], wide, case["temperature"])
    ca, cb = ctx.sample_factor_costs(one, X), ctx.sample_factor_costs(two, X)
    la, lb = ctx.sample_clearance(one, X), ctx.sample_clearance(two, X)
    share = float((ca > 0).mean())
    print(f"P {P}: share of psi > 0 {share:.2f}; cost {rel(ca, cb):.2e}, clearance {rel(la, lb):.2e}")
    assert 0.03 <= share <= 0.97 and rel(ca, cb) <= 1e-13 and rel(la, lb) <= 1e-13
    ref = (br.psi(case["params"], P, n, np.transpose(X[:, :K], (1, 0, 2))) / case["temperature"][:, None]).T
    assert rel(ca, ref) <= 1e-8
    ctx.close()


# ---- (c) the feature's own case: a ball that crosses the straight path of a planar chain at mid-horizon ----
BALL = dict(centre0=np.array([[0.3, 1.6]]), velocity=np.array([[0.0, -1.6]]), radius=np.array([0.5]), sigma=15.0, eps=0.2, r=0.1,
            temperature=5.0)        # at temperature 1 the oracle exhausts its line search on this graph, as on pr3d (test_segment_gpu.py)


def crossing_chain(taus, centre0=None, velocity=None):
    """planar at T = 9, p = 3 without its static obstacles: priors, anchors and the moving-ball set (unary, or binary on the
    interpolated positions at `taus`).  The straight path passes (0, 0) at t = 1; the ball comes down x = 0.3 and is at
    (0.3, 0) then."""
    base = syn.make_planar_chain(T=9, p=3)
    pri, _, anc = base["specs"]
    ch = syn.add_moving_obstacle_set(dict(base, specs=[pri, anc]), BALL["centre0"] if centre0 is None else centre0,
                                     BALL["velocity"] if velocity is None else velocity, BALL["radius"], sigma=BALL["sigma"], eps=BALL["eps"],
                                     r=BALL["r"], p=3, taus=taus, dt=DT, temperature=BALL["temperature"])
    return br.attach_oracle(ch)


@functools.lru_cache(maxsize=None)
def graph(name):
    return crossing_chain(None if name == "unary" else TAUS)


def mean_slices(ch, spec, mu=None):
    mu = ch["mu0"] if mu is None else mu
    return factor_slices(np.asarray(mu)[None], spec, ch["n"])                      # [K][1][d]


def test_the_moving_scene_is_not_one_of_its_static_scenes():
    """(c) The static scene at the ball's first position and the static scene at its last position both give psi = 0 at every
    mean state; the moving scene gives psi > 0.05 at some mean state.  With the reference."""
    T = 9
    last = BALL["centre0"] + (T - 1) * DT * BALL["velocity"]
    for name in ("unary", "binary"):
        taus = None if name == "unary" else TAUS
        moving = graph(name)
        psi = {}
        for tag, ch in (("first", crossing_chain(taus, velocity=np.zeros((1, 2)))), ("last", crossing_chain(taus, centre0=last, velocity=np.zeros((1, 2)))),
                        ("moving", moving)):
            spec = ch["specs"][2]
            psi[tag] = spec["psi_batch"](mean_slices(ch, spec))[:, 0]
        print(f"{name}: psi at the mean states, moving scene: {np.round(psi['moving'], 3)}")
        assert (psi["first"] == 0).all() and (psi["last"] == 0).all() and psi["moving"].max() > 0.05


def check_state(ctx, chain, tag):
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D), rel(st["SigD"], chain.SigD)]
    print(f"{tag}: mu {errs[0]:.2e}, D {errs[1]:.2e}, SigD {errs[2]:.2e}")
    assert max(errs) < RTOL / 10, (tag, errs)


@pytest.mark.parametrize("name", ["unary", "binary"])
def test_graph_ngd_iterations_vs_oracle(name):
    ch = graph(name)
    spec = ch["specs"][2]
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"])
    clr0 = ctx.sample_clearance(ids[2], ch["mu0"][None])
    assert rel(clr0, br.spec_clearance(spec, mean_slices(ch, spec)).T) <= 1e-8
    log = []
    for it in range(5):
        r = ctx.ngd_step(0.55, 10)
        ok, cost, ntr = chain.step()
        print(f"{name} iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
        check_state(ctx, chain, f"{name} iteration {it}")
        log.append(r)
    geo = ctx.profile_geometry(ids[2])
    assert geo["variant"] == 2, geo                                 # d = 4 and d = 8: PsiHingeBalls
    state = ctx.ngd_get_state()
    clr1 = ctx.sample_clearance(ids[2], state["mu"][None])
    print(f"{name}: minimum clearance of the mean path {clr0.min():.3f} -> {clr1.min():.3f}")
    assert clr1.min() > clr0.min()
    # the same five iterations in one call
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    assert ctx.ngd_run(5, 0.55, 10) == log
    st = ctx.ngd_get_state()
    assert all(np.array_equal(st[k], state[k]) for k in state)
    ctx.close()


@pytest.mark.parametrize("name", ["unary", "binary"])
def test_graph_prox_step_vs_oracle(name):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    chain = o.ChainProx(ch["T"], ch["n"], ch["oracle_sets"](), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.3)
    r = ctx.prox_step(0.3, 10)
    ok, cost, ntr = chain.step()
    print(f"{name}: device {r}, oracle {(ok, cost, ntr)}")
    assert r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D)]
    print(f"{name}: mu {errs[0]:.2e}, D {errs[1]:.2e}")
    assert max(errs) < RTOL / 10
    ctx.close()


@pytest.mark.parametrize("name", ["unary", "binary"])
def test_sample_costs_and_clearance(name):
    """(d)"""
    ch = graph(name)
    T, n, S = ch["T"], ch["n"], 33
    spec = ch["specs"][2]
    K = len(spec["start"])
    ctx, ids = api.context_for_chain(ch)
    X = ctx.bt_sample(ch["D0"], ch["U0"], ch["mu0"], S, seed=4100)
    Xk = factor_slices(X, spec, n)
    ref_cost = (spec["psi_batch"](Xk) / np.asarray(spec["temperature"])[:, None]).T
    ref_clr = br.spec_clearance(spec, Xk).T
    share = float((ref_cost > 0).mean())
    print(f"{name}: share of (sample, factor) pairs with psi > 0: {share:.3f}; clearance min {ref_clr.min():.3f}")
    assert 0.03 <= share <= 0.97, "both hinge branches must be exercised"
    cost = ctx.sample_factor_costs(ids[2], X)
    clr = ctx.sample_clearance(ids[2], X)                      # no grid anywhere in this context
    errs = (rel(cost, ref_cost), rel(clr, ref_clr))
    print(f"{name}: cost {errs[0]:.2e}, clearance {errs[1]:.2e}")
    assert cost.shape == (S, K) and clr.shape == (S, K) and max(errs) <= 1e-8, errs
    # J and the minimum clearance are consistent with the per-set rows
    rows = [ctx.sample_factor_costs(sid, X) for sid in ids]
    Jrows = np.sum([r.sum(axis=1) for r in rows], axis=0)
    J = ctx.sample_costs(X)
    assert np.abs(J - Jrows).max() <= 1e-10 * np.abs(Jrows).max()
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    r = ctx.ngd_sample_costs(S, seed=5, clearance_set=ids[2])
    assert np.array_equal(r["clr_min"], ctx.sample_clearance(ids[2], r["X"]).min(axis=1))
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    # a NaN in state i taints exactly the factors that read it
    i = 4
    Xb = X.copy()
    Xb[2, i, 1] = np.nan
    bad = np.zeros((S, K), dtype=bool)
    bad[2, (i - 1 if name == "binary" else i):i + 1] = True
    for got, clean in ((ctx.sample_factor_costs(ids[2], Xb), cost), (ctx.sample_clearance(ids[2], Xb), clr)):
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean[~bad]) and np.isfinite(got[~bad]).all()
    Jb = ctx.sample_costs(Xb)
    assert np.isnan(Jb[2]) and np.array_equal(np.delete(Jb, 2), np.delete(J, 2))
    ctx.close()


# ---- (e) gvi_factors_set_params ----
def fresh_results(case, kind, params, p, setup=None):
    ctx = balls_ctx(case)
    sid = ctx.factors_add(case["d"], p, np.zeros(case["K"], dtype=np.int32), kind, params, case["temperature"])
    if setup:
        setup(ctx, sid)
    out = all_results(ctx, sid, case["mu"], case["Sigma"])
    ctx.close()
    return out


@pytest.mark.parametrize("P,d,p", [(2, 4, 4), (3, 6, 3), (3, 8, 3)])
def test_set_params_equals_a_fresh_context(P, d, p):
    old, new = operator_case(P, d, 3, 5, 3), operator_case(P, d, 3, 5, 8, seed=1)
    new = dict(old, params=new["params"])
    want = fresh_results(new, KIND[P], new["params"], p)
    ctx = balls_ctx(old)
    sid = ctx.factors_add(d, p, np.zeros(5, dtype=np.int32), KIND[P], old["params"], old["temperature"])
    before = all_results(ctx, sid, old["mu"], old["Sigma"])
    ctx.factors_set_params(sid, new["params"])
    got = all_results(ctx, sid, old["mu"], old["Sigma"])
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and not np.array_equal(got[0], before[0])
    # refusals: another J, another block size, values the kind refuses; the set keeps its old blocks bit for bit
    bad = new["params"].copy()
    bad[3, 0] = -1.0
    for params, text in ((operator_case(P, d, 1, 5, 3)["params"], "the layout of a set is fixed at gvi_factors_add"),
                         (new["params"][:, :-1], "the layout of a set is fixed at gvi_factors_add"),
                         (np.concatenate([new["params"], np.zeros((5, 1))], axis=1), "the layout of a set is fixed at gvi_factors_add"),
                         (bad, "HINGE_BALLS: sigma must be finite and >= 0")):
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_params(sid, params)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
        again = all_results(ctx, sid, old["mu"], old["Sigma"])
        assert all(np.array_equal(x, y) for x, y in zip(again, want))
    ctx.close()


def test_set_params_on_the_other_kinds():
    """A HINGE_BOX set (quadrature and closed form) and a HINGE_SDF_2D_SEG set take new blocks; a QUAD_PRIOR set refuses."""
    rng = np.random.default_rng(31)
    K, d = 5, 4
    mu, Sigma = syn.random_marginals(rng, K, d, 0.2)
    case = dict(d=d, n=d, K=K, binary=False, mu=mu, Sigma=Sigma, temperature=rng.uniform(0.5, 5.0, K))
    box = [syn.box_params(10.0, 0.05, np.full((K, d), -lim), np.full((K, d), lim)) for lim in (0.3, 0.2)]
    W = np.zeros((1, 2, d))
    W[0, :, :2] = np.eye(2)
    seg = [syn.segment_params(sig, 0.3, 0.1, W, np.zeros((1, 2))) * np.ones((K, 1)) for sig in (5.0, 9.0)]
    field = syn.circle_sdf((-3.0, -3.0), 0.1, 61, 61, [(0.2, 0.1)], [0.5])
    grid = lambda ctx, sid: ctx.factors_set_sdf2d(sid, (-3.0, -3.0), 0.1, field)
    quad = lambda ctx, sid: ctx.factors_set_closed_form(sid, False)
    for kind, blocks, setup in ((api.PSI_HINGE_BOX, box, None), (api.PSI_HINGE_BOX, box, quad), (api.PSI_HINGE_SDF_2D_SEG, seg, grid)):
        want = fresh_results(case, kind, blocks[1], 4, setup)
        ctx = balls_ctx(case)
        sid = ctx.factors_add(d, 4, np.zeros(K, dtype=np.int32), kind, blocks[0], case["temperature"])
        if setup:
            setup(ctx, sid)
        before = all_results(ctx, sid, mu, Sigma)
        ctx.factors_set_params(sid, blocks[1])
        got = all_results(ctx, sid, mu, Sigma)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and not np.array_equal(got[0], before[0]) and np.abs(got[0]).max() > 0
        ctx.close()
    ch = graph("unary")
    ctx, ids = api.context_for_chain(ch)
    with pytest.raises(api.GviError) as e:
        ctx.factors_set_params(ids[0], ch["specs"][0]["params"])
    assert e.value.status == 1 and "only the kinds that keep their parameter block" in str(e.value)
    with pytest.raises(api.GviError) as e:
        ctx.factors_set_params(ids[1], ch["specs"][1]["params"])
    assert e.value.status == 1 and "only the kinds that keep their parameter block" in str(e.value)
    ctx.close()


def test_ngd_step_after_set_params():
    """A resident iteration on the old scene, new blocks, the state put back with ngd_init: the step is the fresh context's."""
    old = crossing_chain(TAUS, centre0=np.array([[-0.6, 1.2]]), velocity=np.array([[0.3, -1.3]]))
    new = graph("binary")
    fresh, ids = api.context_for_chain(new)
    fresh.ngd_init(new["mu0"], new["D0"], new["U0"])
    want = fresh.ngd_step(0.55, 10)
    want_state = fresh.ngd_get_state()
    fresh.close()
    ctx, ids = api.context_for_chain(old)
    ctx.ngd_init(old["mu0"], old["D0"], old["U0"])
    first = ctx.ngd_step(0.55, 10)
    ctx.factors_set_params(ids[2], new["specs"][2]["params"])
    ctx.ngd_init(new["mu0"], new["D0"], new["U0"])
    got = ctx.ngd_step(0.55, 10)
    st = ctx.ngd_get_state()
    print(f"old scene {first}, new scene {got}, fresh context {want}")
    assert got["accepted"] == want["accepted"] and got["ntrials"] == want["ntrials"] and first["new_cost"] != got["new_cost"]
    assert max(rel(st[k], want_state[k]) for k in st) <= 1e-12
    ctx.close()


def test_argument_rules():
    """(f)"""
    rng = np.random.default_rng(5)
    ctx = api.Context(0)
    ctx.chain_set(2, 4)
    start = np.zeros(2, dtype=np.int32)
    for P, d in ((2, 8), (2, 4), (3, 8)):
        good = {J: operator_case(P, d, J, 2, 3)["params"] for J in (1, 8)}
        per, tail = P * (d + 1) + 1, 8 * (2 * P + 1)
        assert good[1].shape[1] == 3 + per + tail
        for width in (3 + per + tail + 1, 3 + per + tail - 1, 3 + tail, 3 + 9 * per + tail, 3, 2):   # ragged (twice), J = 0, J = 9, too short
            with pytest.raises(api.GviError) as e:
                ctx.factors_add(d, 3, start, KIND[P], rng.normal(size=(2, width)))
            assert e.value.status == 1, (P, d, width)
            assert "J (P (d + 1) + 1) + 8 (2 P + 1)" in str(e.value) and "1 <= J <= 8" in str(e.value)
        for J in (1, 8):
            ctx.factors_add(d, 3, start, KIND[P], good[J])
    with pytest.raises(api.GviError) as e:                                    # no parameter block at all
        ctx.factors_add(8, 3, start, KIND[2], None)
    assert e.value.status == 1
    assert len(ctx.sets) == 6
    ctx.close()
    case = operator_case(2, 8, 3, 2, 3)
    ctx = balls_ctx(case)
    s2 = ctx.factors_add(8, 3, start, KIND[2], case["params"])
    s3 = ctx.factors_add(8, 3, start, KIND[3], operator_case(3, 8, 3, 2, 3)["params"])
    field2 = syn.circle_sdf((-1.0, -1.0), 0.1, 21, 21, [(0.0, 0.0)], [0.5])
    field3 = syn.sphere_sdf3d((-1.0, -1.0, -1.0), 0.2, 11, 11, 11, [(0.0, 0.0, 0.0)], [0.5])
    for sid in (s2, s3):                                                      # no grid, no arm model, no closed form
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_sdf2d(sid, (-1.0, -1.0), 0.1, field2)
        assert e.value.status == 1
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_sdf3d(sid, (-1.0, -1.0, -1.0), 0.2, field3)
        assert e.value.status == 1
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_arm(sid, syn.wam_like_arm())
        assert e.value.status == 1
        with pytest.raises(api.GviError) as e:
            ctx.factors_set_closed_form(sid, True)
        assert e.value.status == 1
        ctx.factors_set_closed_form(sid, False)                               # the quadrature it already runs
        assert np.isfinite(ctx.moments(sid, case["mu"], case["Sigma"])[0]).all()
        clr = ctx.sample_clearance(sid, np.zeros((1, 2, 4)))                  # the clearance needs no grid
        assert clr.shape == (1, 2) and np.isfinite(clr).all()
    ctx.close()


def test_shim_balls_callsite(tmp_path):
    """(g)"""
    build.build_lib()
    exe = str(tmp_path / "balls_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "balls_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
