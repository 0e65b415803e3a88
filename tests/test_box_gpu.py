"""Limit factors (GVI_PSI_HINGE_BOX) on the device, against tests/box_ref.py: the closed-form route against
the exact moments, the quadrature route against the oracle's Gauss-Hermite sums of the same psi (o.batched_moments), both inside
the iteration (o.ChainNGD, o.ChainProx and, for the closed route under the proximal rule, the ClosedProx wrapper below), and the posterior queries.

Bounds, max-norm relative (rel of tests/test_gpu_parity.py): operators 1e-9 (Vddmu, E_xxphi 1e-8) -- TIGHT of that file; a
register instance against the generic kernel 1e-12; chain iterates RTOL / 10 and costs 1e-9 (1e-8 on the arm graph), the bounds
of test_obstacle_chains_vs_oracle there; sample costs 1e-11, margins exact (a subtraction and a minimum).

The two routes compute DIFFERENT numbers on purpose -- the sparse rule is poor on a kink -- so each is held to its
own reference, and to each other only where psi is a plain quadratic over the whole grid (test_edges)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import box_ref as br
import gvi_oracle as o
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import RTOL, TIGHT, rel
from test_sample_cost_host import factor_slices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
REG = (2, 4, 6, 8)                    # dimensions with a register instance (PsiBoxHinge); every other d: the generic kernel
DIMS = [1, 2, 3, 4, 6, 7, 8, 12, 14]
TSEQ = [0.0, 1.5, -1.5, 4.0, -4.0]


def operator_case(d, K, place=None, single_sided=False, seed=0):
    """K factors of dimension d: limits +-1, eps 0.1, sigma in (1, 5); coordinate 0 without an upper limit, coordinate d - 1
    without a lower one (d > 1), coordinate 1 without any (d > 2).  mu is PLACED: entry e = k d + i sits t standard deviations
    inside the hinge of its upper side (e even and that side finite) or lower side, t = TSEQ[e % 5] (or `place` everywhere)."""
    rng = np.random.default_rng(7000 + 100 * d + K + seed)
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.05)
    lo, hi = np.full((K, d), -1.0), np.full((K, d), 1.0)
    if single_sided:
        hi[:, 0::2], lo[:, 1::2] = INF, -INF
    else:
        hi[:, 0] = INF
        if d > 1:
            lo[:, d - 1] = -INF
        if d > 2:
            lo[:, 1], hi[:, 1] = -INF, INF
    params = syn.box_params(rng.uniform(1.0, 5.0, (K, d)), 0.1, lo, hi)
    sd = np.sqrt(np.einsum("kii->ki", Sigma))
    for k in range(K):
        for i in range(d):
            e = k * d + i
            t = TSEQ[e % 5] if place is None else place
            upper = (e % 2 == 0 and np.isfinite(hi[k, i])) or not np.isfinite(lo[k, i])
            if upper and np.isfinite(hi[k, i]):
                mu[k, i] = (hi[k, i] - 0.1) + t * sd[k, i]
            elif np.isfinite(lo[k, i]):
                mu[k, i] = (lo[k, i] + 0.1) - t * sd[k, i]
    return dict(d=d, K=K, params=params, mu=mu, Sigma=Sigma, temperature=rng.uniform(0.5, 5.0, K))


def box_ctx(case, p=3):
    ctx = api.Context(0)
    ctx.chain_set(1, case["d"])
    sid = ctx.factors_add(case["d"], p, np.zeros(case["K"], dtype=np.int32), api.PSI_HINGE_BOX, case["params"], case["temperature"])
    return ctx, sid


def near_share(case):
    """Share of the entries with a finite side whose nearest hinge is within 3 standard deviations of the mean."""
    t = br.t_values(case["params"], case["d"], case["mu"], case["Sigma"])
    fin = ~np.isnan(t).all(axis=2)
    return float((np.nanmin(np.abs(np.where(np.isnan(t), INF, t)), axis=2)[fin] < 3).mean())


def operators(ctx, sid, case):
    mu, Sigma = case["mu"], case["Sigma"]
    Ephi, Vdmu, Vddmu = ctx.moments(sid, mu, Sigma)
    E0, E1, E2 = ctx.raw_moments(sid, mu, Sigma)
    return dict(E_phi=Ephi, Vdmu=Vdmu, Vddmu=Vddmu, cost=ctx.costs(sid, mu, Sigma), E0=E0, E_xmuphi=E1, E_xxphi=E2)


def check_operators(got, ref, tag):
    errs = {k: rel(got[k], ref["E_phi" if k == "E0" else k]) for k in got}
    print(tag + ": " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < (TIGHT * 10 if k in ("Vddmu", "E_xxphi") else TIGHT), (tag, k, v)
    return errs


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("d", DIMS)
def test_closed_route_vs_closed_form(d, K):
    case = operator_case(d, K)
    share = near_share(case)
    assert share >= 0.6, share                     # the violated regime and the far-inside one are both present
    ref = br.closed_moments(case["params"], d, case["mu"], case["Sigma"], case["temperature"])
    assert ref["E_phi"].max() > 1e-3 and (case["temperature"] != 1).all()
    ctx, sid = box_ctx(case)
    got = operators(ctx, sid, case)
    assert ctx.profile_geometry(sid)["variant"] == 0          # no sigma points
    check_operators(got, ref, f"closed d {d} K {K} (share of |t| < 3: {share:.2f})")
    V = got["Vddmu"]
    diag = np.abs(np.einsum("kii->ki", V)).max()
    off = np.abs(V - np.einsum("ki,ij->kij", np.einsum("kii->ki", V), np.eye(d))).max()
    print(f"  Vddmu off-diagonal / diagonal: {off / diag:.2e}")
    assert off <= 1e-12 * diag
    ctx.close()


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", DIMS)
def test_quadrature_route_vs_oracle(d, p, K):
    case = operator_case(d, K)
    Z, w = o.nwspgr_cached(d, p)
    ref = o.batched_moments(Z, w, case["mu"], case["Sigma"], br.psi_batch(case["params"], d), case["temperature"])
    ctx, sid = box_ctx(case, p)
    ctx.factors_set_closed_form(sid, 0)
    out = {}
    for variant in (0, 1):
        ctx.set_variant(variant)
        got = operators(ctx, sid, case)
        geo = ctx.profile_geometry(sid)
        assert geo["variant"] == (2 if d in REG and variant == 0 else 1), geo
        check_operators(got, ref, f"quadrature d {d} p {p} K {K} variant {variant} -> kernel {geo['variant']}")
        out[variant] = got
    if d in REG:
        gap = max(rel(out[0][k], out[1][k]) for k in out[0])
        print(f"  register against generic: {gap:.2e}")
        assert gap <= 1e-12, gap
    ctx.close()


def test_edges():
    # every side infinite: exact zeros on both routes
    case = operator_case(4, 5)
    case["params"] = np.tile(syn.box_params(2.0, 0.1, np.full(4, -INF), np.full(4, INF)), (5, 1))
    ctx, sid = box_ctx(case)
    for on in (1, 0):
        ctx.factors_set_closed_form(sid, on)
        assert all((v == 0).all() for v in operators(ctx, sid, case).values()), on
    ctx.close()
    # 40 standard deviations inside the limits (one limit per coordinate: a band of +-1 is narrower than that): finite, and
    # zero to 1e-300 sigma sd^2
    for d in (3, 6):
        case = operator_case(d, 5, place=-40.0, single_sided=True)
        ctx, sid = box_ctx(case)
        for on in (1, 0):
            ctx.factors_set_closed_form(sid, on)
            got = operators(ctx, sid, case)
            bound = 1e-300 * (br.unpack(case["params"], d)[0] * np.einsum("kii->ki", case["Sigma"])).min()      # 1e-300 sigma sd^2
            assert all(np.isfinite(v).all() and (np.abs(v) <= bound).all() for v in got.values()), (d, on)
        ctx.close()
    # 40 standard deviations past single-sided limits: psi is a plain quadratic over the whole grid, the rule is exact
    for d in (3, 6, 12):
        case = operator_case(d, 5, place=40.0, single_sided=True)
        ref = br.closed_moments(case["params"], d, case["mu"], case["Sigma"], case["temperature"])
        ctx, sid = box_ctx(case, 3)
        a = operators(ctx, sid, case)
        ctx.factors_set_closed_form(sid, 0)
        b = operators(ctx, sid, case)
        check_operators(a, ref, f"t = +40, d {d}, closed against the reference")
        errs = {k: rel(b[k], a[k]) for k in a}
        print(f"t = +40, d {d}, quadrature against closed: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-9, errs
        # back and forth: each route returns its own bits
        ctx.factors_set_closed_form(sid, 1)
        a2 = operators(ctx, sid, case)
        ctx.factors_set_closed_form(sid, 0)
        b2 = operators(ctx, sid, case)
        assert all(np.array_equal(a[k], a2[k]) and np.array_equal(b[k], b2[k]) for k in a)
        ctx.close()
    # the same toggle on the standard inputs, where the routes differ
    case = operator_case(4, 5)
    ctx, sid = box_ctx(case)
    runs = []
    for on in (1, 0, 1, 0):
        ctx.factors_set_closed_form(sid, on)
        runs.append(operators(ctx, sid, case))
    assert all(np.array_equal(runs[0][k], runs[2][k]) and np.array_equal(runs[1][k], runs[3][k]) for k in runs[0])
    assert rel(runs[1]["E_phi"], runs[0]["E_phi"]) > 1e-6          # the rule's error on the kink, not rounding
    ctx.close()
    # K = 0 (the shard of a rank that holds none of the set's factors): every launch skips the set on both routes, and the
    # iteration is the one of the graph without it
    base = attach_oracle(dict(syn.make_planar_chain(T=9)))
    empty = dict(kind=api.PSI_HINGE_BOX, d=4, p=3, start=np.zeros(0, dtype=np.int32), params=np.zeros((0, 16)), temperature=np.ones(0))
    res = []
    for specs, on in ((base["specs"], None), (base["specs"] + [empty], 1), (base["specs"] + [empty], 0)):
        ctx, ids = api.context_for_chain(base, specs=specs)
        if on is not None:
            ctx.factors_set_closed_form(ids[-1], on)
        ctx.ngd_init(base["mu0"], base["D0"], base["U0"])
        res.append((ctx.ngd_step(0.55, 10), ctx.ngd_get_state()))
        ctx.close()
    (r0, st0), (r1, st1), (r2, st2) = res
    assert r1 == r2 and all(np.array_equal(st1[k], st2[k]) for k in st1)          # the route of an empty set changes nothing
    assert r1["accepted"] == r0["accepted"] and r1["ntrials"] == r0["ntrials"]
    assert np.isclose(r1["new_cost"], r0["new_cost"], rtol=1e-12, atol=0)
    gaps = {k: rel(st1[k], st0[k]) for k in st0}                                  # a fourth set takes other launches: rounding
    print("K = 0 against the graph without the set: " + ", ".join(f"{k} {v:.1e}" for k, v in gaps.items()))
    assert max(gaps.values()) <= 1e-12, gaps


def test_argument_rules():
    ctx = api.Context(0)
    ctx.chain_set(2, 3)
    start = np.zeros(2, dtype=np.int32)
    good = syn.box_params([1.0, 2.0, 0.0], [0.1, 0.0, -0.1], [-1.0, -INF, -2.0], [1.0, INF, INF])
    good = np.tile(good, (2, 1))

    def refused(params, d=3):
        with pytest.raises(api.GviError) as e:
            ctx.factors_add(d, 3, start, api.PSI_HINGE_BOX, params)
        assert e.value.status == 1, str(e.value)

    for width in (11, 13, 3, 24):                                              # params_per_factor != 4 d
        refused(np.zeros((2, width)) + np.arange(width) * 0.01)
    refused(None)
    for col, val in ((0, np.nan), (4, np.nan), (7, np.nan), (10, np.nan),      # a NaN in sigma, eps, lo, hi
                     (1, -1.0), (1, INF), (2, -INF),                           # sigma < 0 or not finite
                     (3, INF), (5, -INF),                                      # eps not finite
                     (6, 1.0), (6, 1.5), (9, -1.0),                            # lo >= hi
                     (6, INF), (7, INF), (9, -INF), (10, -INF)):               # lo = +inf, hi = -inf
        bad = good.copy()
        bad[1, col] = val
        refused(bad)
    assert len(ctx.sets) == 0
    sid = ctx.factors_add(3, 3, start, api.PSI_HINGE_BOX, good)                # sigma = 0, eps < 0 and eps = 0 are legal
    six = ctx.factors_add(6, 3, np.zeros(1, dtype=np.int32), api.PSI_HINGE_BOX, syn.box_params(1.0, 0.1, np.full(6, -1.0), np.full(6, 1.0)))
    field = syn.circle_sdf((-1.0, -1.0), 0.1, 21, 21, [(0.0, 0.0)], [0.5])
    with pytest.raises(api.GviError) as e:                                     # needs no grid, takes none
        ctx.factors_set_sdf2d(sid, (-1.0, -1.0), 0.1, field)
    assert e.value.status == 1
    with pytest.raises(api.GviError) as e:
        ctx.factors_set_sdf3d(sid, (-1.0, -1.0, -1.0), 0.1, np.zeros((3, 3, 3)))
    assert e.value.status == 1
    with pytest.raises(api.GviError) as e:
        ctx.factors_set_arm(sid, syn.wam_like_arm())
    assert e.value.status == 1
    mu, Sigma = syn.random_marginals(np.random.default_rng(1), 2, 3, 0.05)
    assert np.isfinite(ctx.moments(sid, mu, Sigma)[0]).all()                   # works without any of them
    for on in (0, 1, 1, 0, 1):                                                 # both routes can be selected on a box set
        ctx.factors_set_closed_form(sid, on)
    ctx.factors_set_closed_form(six, 0)
    hinge = ctx.factors_add(3, 3, start, api.PSI_HINGE_SDF_2D, np.tile([[15.0, 0.5, 0.3]], (2, 1)))
    with pytest.raises(api.GviError) as e:                                     # refused as before
        ctx.factors_set_closed_form(hinge, 1)
    assert e.value.status == 1
    ctx.factors_set_closed_form(hinge, 0)
    ctx.close()


# ---- the iteration ----
def attach_oracle(ch):
    """tests/chains.py's glue for a chain whose last set is a box set: oracle_sets(closed) gives that set the exact moments as
    fast_moments (closed) or leaves it on the Gauss-Hermite sums of psi_batch."""
    from chains import oracle_psi_batch
    for spec in ch["specs"]:
        spec["psi_batch"] = br.psi_batch(spec["params"], spec["d"]) if spec["kind"] == syn.PSI_HINGE_BOX else oracle_psi_batch(spec)

    def oracle_sets(closed):
        out = []
        for spec in ch["specs"]:
            fs = o.FactorSet(spec["start"], spec["d"], spec["p"], spec["psi_batch"])
            fs.temperature = np.asarray(spec["temperature"], dtype=np.float64)
            if closed and spec["kind"] == syn.PSI_HINGE_BOX:
                fs.fast_moments = br.closed_form(spec["params"], spec["d"])
                fs.box_params = spec["params"]                      # ClosedProx
            out.append(fs)
        return out
    ch["oracle_sets"] = oracle_sets
    return ch


@functools.lru_cache(maxsize=None)
def limited_graph(name):
    """planar: make_planar_chain(T = 9) (speeds (3, 0.4)) with velocity limits BELOW them, |vx| <= 2.9 and |vy| <= 0.35, positions
    free.  arm7: make_obstacle_chain("arm7", T = 5) (n = 14) with limits on the seven joint angles placed so that the first and
    the last joints of the start trajectory are in their hinges, rates free; the obstacle set at the temperature the arm
    benchmark uses."""
    if name == "planar":
        ch = syn.add_box_set(syn.make_planar_chain(T=9), [-INF, -INF, -2.9, -0.35], [INF, INF, 2.9, 0.35], sigma=8.0, eps=0.05, p=3)
    else:
        base = syn.make_obstacle_chain("arm7", T=5)
        base["specs"][1]["temperature"] = np.full(5, 30.0)
        q = base["mu0"][:, :7]
        lo = np.concatenate([q.min(axis=0) - 0.5, np.full(7, -INF)])
        hi = np.concatenate([q.max(axis=0) + 0.5, np.full(7, INF)])
        lo[0], hi[6] = q[:, 0].min() + 0.02, q[:, 6].max() - 0.02
        ch = syn.add_box_set(base, lo, hi, sigma=8.0, eps=0.05, p=3)
    return attach_oracle(ch)


def initial_near_share(ch):
    """Share of the box factors with a coordinate whose nearest hinge is within 3 standard deviations at the initial marginals."""
    box = ch["specs"][-1]
    SigD, SigU = o.inverse_gbp(ch["D0"], ch["U0"])
    mk, Sk = o.gather_marginals(ch["mu0"], SigD, SigU, box["start"], box["d"])
    t = br.t_values(box["params"], box["d"], mk, Sk)
    return float((np.nanmin(np.abs(np.where(np.isnan(t), INF, t)), axis=(1, 2)) < 3).mean())


def check_state(ctx, chain, tag):
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D), rel(st["SigD"], chain.SigD)]
    print(f"{tag}: mu {errs[0]:.2e}, D {errs[1]:.2e}, SigD {errs[2]:.2e}")
    assert max(errs) < RTOL / 10, (tag, errs)


@pytest.mark.parametrize("name,iters", [("planar", 5), ("arm7", 2)])
def test_iterations_vs_oracle(name, iters):
    ch = limited_graph(name)
    share = initial_near_share(ch)
    print(f"{name}: share of box factors with a hinge within 3 sd at the start: {share:.2f}")
    assert share >= 0.25
    ctol = 1e-8 if name == "arm7" else 1e-9
    for closed in (True, False):
        ctx, ids = api.context_for_chain(ch)
        ctx.factors_set_closed_form(ids[-1], int(closed))
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](closed), ch["mu0"], ch["D0"], ch["U0"])
        log = []
        for it in range(iters):
            r = ctx.ngd_step(0.55, 10)
            ok, cost, ntr = chain.step()
            print(f"{name} closed {closed} iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
            assert r["accepted"] == ok and r["ntrials"] == ntr
            assert np.isclose(r["new_cost"], cost, rtol=ctol, atol=0)
            check_state(ctx, chain, f"{name} closed {closed} iteration {it}")
            log.append(r)
        geo = ctx.profile_geometry(ids[-1])
        assert geo["variant"] == (0 if closed else (2 if ch["n"] in REG else 1)), geo
        assert ctx.ngd_factor_costs(ids[-1]).max() > 0              # the limits are active on this path
        state = ctx.ngd_get_state()
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])                 # the same iterations in one call
        assert ctx.ngd_run(iters, 0.55, 10) == log
        st = ctx.ngd_get_state()
        assert all(np.array_equal(st[k], state[k]) for k in state)
        ctx.close()


class ClosedProx(o.ChainProx):
    """o.ChainProx integrates every set by Gauss-Hermite sums (no fast_moments hook).  This wrapper changes ONE thing: the raw
    integrals E[psi], E[(x - mu) psi], E[(x - mu)(x - mu)^T psi] of a box set come from box_ref's closed form; the factor-level
    JKO map (o.bw_jko), the assembly and the line search are the oracle's own."""

    def raw(self, fs, mk, Sk):
        if getattr(fs, "box_params", None) is not None:
            return br.closed_moments(fs.box_params, fs.d, mk, Sk, 1.0)
        return o.batched_moments(fs.Z, fs.w, mk, Sk, fs.psi_batch, 1.0)

    def factor_costs(self, mu, SigD, SigU):
        return [self.raw(fs, *o.gather_marginals(mu, SigD, SigU, fs.start, fs.d))["E_phi"] for fs in self.sets]

    def gradients(self, h):
        parts = []
        for fs in self.sets:
            mk, Sk = o.gather_marginals(self.mu, self.SigD, self.SigU, fs.start, fs.d)
            r = self.raw(fs, mk, Sk)
            jko = [o.bw_jko(mk[k], Sk[k], np.linalg.inv(Sk[k]), r["E_phi"][k], r["E_xmuphi"][k], r["E_xxphi"][k], h) for k in range(len(mk))]
            parts.append((fs.start, np.array([v[0] for v in jko]), np.array([v[1] for v in jko])))
        return o.bt_assemble(self.T, self.n, parts)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("name", ["planar", "arm7"])
def test_prox_step_vs_oracle(name, closed):
    """One step under GVI_RULE_PROX_JKO with the box set on its default closed-form route (against ClosedProx) and on the
    quadrature route (against o.ChainProx as it is)."""
    ch = limited_graph(name)
    ctx, ids = api.context_for_chain(ch)
    ctx.factors_set_closed_form(ids[-1], int(closed))
    ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    cls = ClosedProx if closed else o.ChainProx
    chain = cls(ch["T"], ch["n"], ch["oracle_sets"](closed), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.3)
    r = ctx.prox_step(0.3, 10)
    ok, cost, ntr = chain.step()
    print(f"{name} closed {closed}: device {r}, oracle {(ok, cost, ntr)}")
    assert ctx.profile_geometry(ids[-1])["variant"] == (0 if closed else (2 if ch["n"] in REG else 1))
    assert r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-8 if name == "arm7" else 1e-9, atol=0)
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D)]
    print(f"{name} closed {closed}: mu {errs[0]:.2e}, D {errs[1]:.2e}")
    assert max(errs) < RTOL / 10
    ctx.close()


# ---- posterior queries ----
def test_samples():
    ch = limited_graph("planar")
    T, n, S = ch["T"], ch["n"], 33
    box = ch["specs"][-1]
    ctx, ids = api.context_for_chain(ch)
    sid = ids[-1]
    X = ctx.bt_sample(ch["D0"], ch["U0"], ch["mu0"], S, seed=4100)
    Xk = factor_slices(X, box, n)
    ref_cost = (box["psi_batch"](Xk) / np.asarray(box["temperature"])[:, None]).T
    ref_mg = br.margin(box["params"], box["d"], Xk).T
    share = float((ref_cost > 0).mean())
    print(f"share of (sample, factor) pairs with psi > 0: {share:.3f}; margin min {ref_mg.min():.3f} max {ref_mg.max():.3f}")
    assert 0.03 <= share <= 0.97 and ref_mg.min() < 0 < ref_mg.max()
    cost, mg = ctx.sample_factor_costs(sid, X), ctx.sample_clearance(sid, X)
    err = rel(cost, ref_cost)
    print(f"cost {err:.2e}; margin bit-equal: {np.array_equal(mg, ref_mg)}")
    assert cost.shape == (S, T) and err <= 1e-11 and np.array_equal(mg, ref_mg)
    rows = [ctx.sample_factor_costs(s, X) for s in ids]
    Jrows = np.sum([r.sum(axis=1) for r in rows], axis=0)
    J = ctx.sample_costs(X)
    assert np.abs(J - Jrows).max() <= 1e-11 * np.abs(Jrows).max()
    # a NaN and a +inf in the slices of factors 4 and 6 of samples 2 and 5: those entries are NaN, every other one is untouched
    Xb = X.copy()
    Xb[2, 4, 0], Xb[5, 6, 3] = np.nan, INF                                   # a position (no limit on it) and a velocity
    bad = np.zeros((S, T), dtype=bool)
    bad[2, 4] = bad[5, 6] = True
    for got, clean in ((ctx.sample_factor_costs(sid, Xb), cost), (ctx.sample_clearance(sid, Xb), mg)):
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean[~bad]) and np.isfinite(got[~bad]).all()
    Jb = ctx.sample_costs(Xb)
    assert np.isnan(Jb[[2, 5]]).all() and np.array_equal(np.delete(Jb, [2, 5]), np.delete(J, [2, 5]))
    # the resident call: clearance_set = the box set; the resident state is not touched
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    ctx.ngd_step(0.55, 10)
    before = ctx.ngd_get_state()
    r = ctx.ngd_sample_costs(S, seed=5, clearance_set=sid)
    after = ctx.ngd_get_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert np.array_equal(r["clr_min"], ctx.sample_clearance(sid, r["X"]).min(axis=1))
    assert np.array_equal(r["clr_min"], br.margin(box["params"], box["d"], factor_slices(r["X"], box, n)).min(axis=0))
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    ctx.close()
    # a set without a finite limit: +inf margin, zero cost
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    free = ctx.factors_add(n, 3, np.arange(T, dtype=np.int32), api.PSI_HINGE_BOX, np.tile(syn.box_params(1.0, 0.1, np.full(n, -INF), np.full(n, INF)), (T, 1)))
    assert (ctx.sample_clearance(free, X) == INF).all() and (ctx.sample_factor_costs(free, X) == 0).all()
    ctx.close()


def test_shim_box_callsite(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "box_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "box_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
