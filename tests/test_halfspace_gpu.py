"""Half-space and corridor limit factors (GVI_PSI_HINGE_HALFSPACE) on the device, against
tests/halfspace_ref.py: the closed-form route (moments_halfspace_closed_kernel: several factors per wave) against the exact
moments, the quadrature route against the oracle's Gauss-Hermite sums of the same psi (o.batched_moments), axis rows against a
GVI_PSI_HINGE_BOX set of the same limits, both routes inside the iteration (o.ChainNGD, o.ChainProx and the ClosedProx wrapper),
and the posterior queries.

Bounds, max-norm relative (rel of tests/test_gpu_parity.py), the ones of tests/test_box_gpu.py: operators TIGHT = 1e-9 (Vddmu,
E_xxphi 1e-8); chain iterates RTOL / 10 and costs 1e-9; sample costs 1e-11, margins 1e-13 (a d-long inner product and a division).

Shapes: the packing of (factor, row) pairs into a wave goes wrong, if at all, where J is no power of two (3, 5: padding lanes),
at the cap (16: four factors per wave), at J = 1 (64 factors per wave, one lane walks every output), where K leaves a wave
part-filled (1, 5, 67) or needs a second wave (J = 1, K = 67), and at the largest slice (d = 32).

The two routes compute DIFFERENT numbers on purpose -- the sparse rule is poor on a kink -- so each is held to its own
reference, and to each other only where psi is a plain quadratic over the whole grid (test_edges)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o
import halfspace_ref as hr
import test_box_gpu as box_gpu
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import RTOL, TIGHT, rel
from test_sample_cost_host import factor_slices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
# (d, J, K): every d of {1, 2, 3, 4, 7, 8, 12, 14, 32}, every J of {1, 2, 3, 5, 8, 16}, every K of {1, 5, 67}
CASES = [(1, 1, 67), (2, 2, 5), (3, 3, 1), (4, 5, 67), (4, 2, 67), (7, 8, 5), (8, 16, 5), (12, 3, 67), (14, 16, 1), (32, 16, 5), (32, 1, 67)]


@functools.lru_cache(maxsize=None)
def operator_case(d, J, K, seed=0):
    """K factors of J rows: normals N(0, I), sigma in (1, 5), eps in (0, 0.2), about a quarter of the rows off (half of those with a
    zero normal; row 0 of factor 0 stays on), b_j = a_j^T mu + eps_j + t_j sd_j with t_j from U[-2.5, 2.5]: every active hinge is
    within 3 standard deviations of the mean."""
    rng = np.random.default_rng(16000 + 1000 * d + 10 * J + K + seed)
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.05)
    A = rng.normal(size=(K, J, d))
    sig, eps = rng.uniform(1.0, 5.0, (K, J)), rng.uniform(0.0, 0.2, (K, J))
    off = rng.random((K, J)) < 0.25
    off[0, 0] = False
    sig[off] = 0.0
    A[off & (rng.random((K, J)) < 0.5)] = 0.0
    sd = np.sqrt(np.einsum("kja,kab,kjb->kj", A, Sigma, A))
    t = rng.uniform(-2.5, 2.5, (K, J))
    b = np.einsum("kjd,kd->kj", A, mu) + eps + t * sd
    params = syn.halfspace_params(sig, eps, b, A)
    tv = hr.t_values(params, d, mu, Sigma)
    assert np.array_equal(np.isnan(tv), off) and np.nanmax(np.abs(tv)) <= 3.0          # every active hinge within 3 sd
    temperature = rng.uniform(0.5, 5.0, K)
    assert (temperature != 1).all()
    return dict(d=d, J=J, K=K, params=params, mu=mu, Sigma=Sigma, temperature=temperature, off=off)


def half_ctx(case, p=3):
    ctx = api.Context(0)
    ctx.chain_set(1, case["d"])
    sid = ctx.factors_add(case["d"], p, np.zeros(case["K"], dtype=np.int32), api.PSI_HINGE_HALFSPACE, case["params"], case["temperature"])
    return ctx, sid


operators, check_operators = box_gpu.operators, box_gpu.check_operators


# K = 4100 at J = 16: 1025 waves, the first launch with four waves per block (plan_moments); at d = 32 its dynamic LDS passes 64 KB
@pytest.mark.parametrize("d,J,K", CASES + [(2, 16, 4100), (32, 16, 4100)])
def test_closed_route_vs_closed_form(d, J, K):
    case = operator_case(d, J, K)
    ref = hr.closed_moments(case["params"], d, case["mu"], case["Sigma"], case["temperature"])
    assert ref["E_phi"].max() > 0
    ctx, sid = half_ctx(case)
    got = operators(ctx, sid, case)
    assert ctx.profile_geometry(sid)["variant"] == 0          # no sigma points
    check_operators(got, ref, f"closed d {d} J {J} K {K} (rows off: {case['off'].mean():.2f})")
    again = operators(ctx, sid, case)                          # the same input: the same bits
    assert all(np.array_equal(got[k], again[k]) for k in got)
    ctx.close()


# p = 4 up to d = 14: the (32, 4) rule has 45889 points, ten seconds of table generation on the host before anything is tested
@pytest.mark.parametrize("d,J,K,p", [c + (3,) for c in CASES] + [c + (4,) for c in CASES if c[0] <= 14])
def test_quadrature_route_vs_oracle(d, J, K, p):
    case = operator_case(d, J, K)
    Z, w = o.nwspgr_cached(d, p)
    ref = o.batched_moments(Z, w, case["mu"], case["Sigma"], hr.psi_batch(case["params"], d), case["temperature"])
    ctx, sid = half_ctx(case, p)
    ctx.factors_set_closed_form(sid, 0)
    got = operators(ctx, sid, case)
    assert ctx.profile_geometry(sid)["variant"] == 1          # the generic kernel: no register instance for this kind
    check_operators(got, ref, f"quadrature d {d} J {J} K {K} p {p}")
    ctx.close()


@pytest.mark.parametrize("d", [2, 4, 8])
def test_axis_rows_vs_box_set_on_the_device(d):
    """Rows +e_i / -e_i with b = hi_i / -lo_i against a HINGE_BOX set of the same limits, each route against the same route."""
    rng = np.random.default_rng(1600 + d)
    K = 5
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.05)
    sig, eps = rng.uniform(1.0, 5.0, (K, d)), rng.uniform(0.0, 0.1, (K, d))
    sd = np.sqrt(np.einsum("kii->ki", Sigma))
    hi, lo = mu + rng.uniform(-1.0, 2.5, (K, d)) * sd, mu - rng.uniform(-1.0, 2.5, (K, d)) * sd
    lo = np.minimum(lo, hi - 0.5 * sd)
    temperature = rng.uniform(0.5, 5.0, K)
    half = syn.halfspace_params(np.tile(sig, 2), np.tile(eps, 2), np.concatenate([hi, -lo], axis=1), np.concatenate([np.eye(d), -np.eye(d)]))
    case = dict(d=d, K=K, mu=mu, Sigma=Sigma)
    ctx = api.Context(0)
    ctx.chain_set(1, d)
    start = np.zeros(K, dtype=np.int32)
    hs = ctx.factors_add(d, 3, start, api.PSI_HINGE_HALFSPACE, half, temperature)
    bx = ctx.factors_add(d, 3, start, api.PSI_HINGE_BOX, syn.box_params(sig, eps, lo, hi), temperature)
    ctx.set_variant(1)                                         # the box set on the generic kernel too: the same sums
    for on in (1, 0):
        ctx.factors_set_closed_form(hs, on)
        ctx.factors_set_closed_form(bx, on)
        a, b = operators(ctx, hs, case), operators(ctx, bx, case)
        assert a["E_phi"].max() > 0
        errs = {k: rel(a[k], b[k]) for k in a}
        print(f"axis rows against the box set, d {d}, closed {on}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < (TIGHT * 10 if k in ("Vddmu", "E_xxphi") else TIGHT), (d, on, k, v)
    ctx.close()


def single_row_case(d, K, t, seed):
    """One active row per factor whose mean sits t standard deviations INSIDE the hinge (t = +40: psi is a plain quadratic over
    the whole grid; t = -6: the far tail)."""
    rng = np.random.default_rng(seed)
    mu, Sigma = syn.random_marginals(rng, K, d, scale=0.05)
    A = rng.normal(size=(K, 1, d))
    sd = np.sqrt(np.einsum("kja,kab,kjb->kj", A, Sigma, A))
    b = np.einsum("kjd,kd->kj", A, mu) + 0.1 - t * sd
    return dict(d=d, K=K, mu=mu, Sigma=Sigma, temperature=rng.uniform(0.5, 5.0, K),
                params=syn.halfspace_params(rng.uniform(1.0, 5.0, (K, 1)), 0.1, b, A))


def test_edges():
    # every row off (one of them with a zero normal): exact zeros on both routes, +inf margin
    case = dict(operator_case(4, 5, 67))
    sig0 = case["params"].copy()
    sig0[:, :5] = 0.0
    sig0[:, 15 + 4:15 + 8] = 0.0
    case["params"] = sig0
    ctx, sid = half_ctx(case)
    for on in (1, 0):
        ctx.factors_set_closed_form(sid, on)
        assert all((v == 0).all() for v in operators(ctx, sid, case).values()), on
    ctx.close()
    # t = -6 and t = +40 single rows: finite on both routes; at t = +40 the rule is exact and the routes agree
    for d, t in ((3, -6.0), (6, -6.0), (3, 40.0), (6, 40.0), (12, 40.0)):
        case = single_row_case(d, 5, t, 1700 + d)
        ref = hr.closed_moments(case["params"], d, case["mu"], case["Sigma"], case["temperature"])
        ctx, sid = half_ctx(case, 3)
        a = operators(ctx, sid, case)
        ctx.factors_set_closed_form(sid, 0)
        b = operators(ctx, sid, case)
        assert all(np.isfinite(v).all() for v in a.values()) and all(np.isfinite(v).all() for v in b.values()), (d, t)
        check_operators(a, ref, f"t = {t:+.0f}, d {d}, closed against the reference")
        if t > 0:
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
    # the toggle on the standard inputs, where the routes differ by the rule's error on the kink, not by rounding
    case = operator_case(4, 5, 67)
    ctx, sid = half_ctx(case)
    runs = []
    for on in (1, 0, 1, 0):
        ctx.factors_set_closed_form(sid, on)
        runs.append(operators(ctx, sid, case))
        assert ctx.profile_geometry(sid)["variant"] == (0 if on else 1)
    assert all(np.array_equal(runs[0][k], runs[2][k]) and np.array_equal(runs[1][k], runs[3][k]) for k in runs[0])
    assert rel(runs[1]["E_phi"], runs[0]["E_phi"]) > 1e-6
    ctx.close()
    # K = 0 (the shard of a rank that holds none of the set's factors) on either route: the iteration is, bit for bit, the one
    # of the graph without the set.  The graph already holds a corridor set, so both take prep -> moments -> epilogue per set.
    base = corridor_graph(False)
    empty = dict(kind=api.PSI_HINGE_HALFSPACE, d=4, p=3, start=np.zeros(0, dtype=np.int32), params=np.zeros((0, 28)), temperature=np.ones(0))
    res = []
    for specs, on in ((base["specs"], None), (base["specs"] + [empty], 1), (base["specs"] + [empty], 0)):
        ctx, ids = api.context_for_chain(base, specs=specs)
        if on is not None:
            ctx.factors_set_closed_form(ids[-1], on)
        ctx.ngd_init(base["mu0"], base["D0"], base["U0"])
        res.append(([ctx.ngd_step(0.55, 10) for _ in range(2)], ctx.ngd_get_state()))
        ctx.close()
    (r0, st0), (r1, st1), (r2, st2) = res
    assert r0 == r1 == r2
    assert all(np.array_equal(st0[k], st1[k]) and np.array_equal(st0[k], st2[k]) for k in st0)


def test_argument_rules():
    ctx = api.Context(0)
    ctx.chain_set(2, 3)
    start = np.zeros(2, dtype=np.int32)
    # J = 3 on d = 3: [sigma 0..2 | eps 3..5 | b 6..8 | A 9..17]; row 2 is off and carries a zero normal
    good = syn.halfspace_params([1.0, 2.0, 0.0], [0.1, 0.0, -0.1], [1.0, -1.0, 0.0], [[1.0, 0.0, 0.5], [0.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
    good = np.tile(good, (2, 1))

    def refused(params, text, d=3):
        with pytest.raises(api.GviError) as e:
            ctx.factors_add(d, 3, start, api.PSI_HINGE_HALFSPACE, params)
        assert e.value.status == 1 and text in str(e.value), str(e.value)

    for width in (5, 7, 17, 19, 6 * 17):                                       # no multiple of d + 3 = 6, or J = 17
        refused(np.ones((2, width)), "params_per_factor = J (d + 3)")
    refused(None, "params_per_factor")
    for col in (0, 4, 7, 10, 17):                                              # a NaN in sigma, eps, b, A, and in the row that is off
        bad = good.copy()
        bad[1, col] = np.nan
        refused(bad, "NaN")
    for col, val, text in ((1, -1.0, "sigma must be finite and >= 0"), (1, INF, "sigma must be finite and >= 0"), (2, -INF, "sigma must be finite and >= 0"),
                           (3, INF, "eps must be finite"), (5, -INF, "eps must be finite"),
                           (6, INF, "b must be finite"), (8, -INF, "b must be finite"),
                           (9, INF, "A must be finite"), (16, -INF, "A must be finite")):
        bad = good.copy()
        bad[1, col] = val
        refused(bad, text)
    bad = good.copy()
    bad[1, 13] = 0.0                                                           # row 1 (sigma = 2): its only non-zero entry
    refused(bad, "non-zero normal")
    bad = good.copy()
    bad[0, 2] = 1.0                                                            # switching the zero row on
    refused(bad, "non-zero normal")
    assert len(ctx.sets) == 0
    sid = ctx.factors_add(3, 3, start, api.PSI_HINGE_HALFSPACE, good)          # sigma = 0 with a zero normal, eps < 0 and eps = 0 are legal
    cap = ctx.factors_add(3, 3, start, api.PSI_HINGE_HALFSPACE, np.tile(syn.halfspace_params(1.0, 0.1, 1.0, np.eye(3)[[0]], J=16), (2, 1)))
    six = ctx.factors_add(6, 3, np.zeros(1, dtype=np.int32), api.PSI_HINGE_HALFSPACE, syn.halfspace_params(1.0, 0.1, 1.0, np.ones((2, 6))))
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
    assert np.isfinite(ctx.moments(sid, mu, Sigma)[0]).all() and np.isfinite(ctx.moments(cap, mu, Sigma)[0]).all()
    assert ctx.profile_geometry(sid)["variant"] == 0
    for on in (0, 1, 1, 0, 1):                                                 # both routes can be selected
        ctx.factors_set_closed_form(sid, on)
        ctx.moments(sid, mu, Sigma)
        assert ctx.profile_geometry(sid)["variant"] == (0 if on else 1)
    ctx.factors_set_closed_form(six, 0)
    hinge = ctx.factors_add(3, 3, start, api.PSI_HINGE_SDF_2D, np.tile([[15.0, 0.5, 0.3]], (2, 1)))
    with pytest.raises(api.GviError) as e:                                     # refused as before, and the message names the kind
        ctx.factors_set_closed_form(hinge, 1)
    assert e.value.status == 1 and "HINGE_HALFSPACE" in str(e.value)
    ctx.factors_set_closed_form(hinge, 0)
    ctx.close()


# ---- the iteration ----
NORMALS = np.array([[-0.4, 2.0], [0.2, -1.0], [1.5, 0.0], [-1.0, 0.0]])      # oblique and not normalised
OFFSETS = np.array([0.3, 0.15, 4.2, 2.8])


def attach_oracle(ch):
    """tests/chains.py's glue for a chain whose last set is a half-space set: oracle_sets(closed) gives that set the exact moments
    as fast_moments (closed) or leaves it on the Gauss-Hermite sums of psi_batch."""
    from chains import oracle_psi_batch
    for spec in ch["specs"]:
        spec["psi_batch"] = hr.psi_batch(spec["params"], spec["d"]) if spec["kind"] == syn.PSI_HINGE_HALFSPACE else oracle_psi_batch(spec)

    def oracle_sets(closed):
        out = []
        for spec in ch["specs"]:
            fs = o.FactorSet(spec["start"], spec["d"], spec["p"], spec["psi_batch"])
            fs.temperature = np.asarray(spec["temperature"], dtype=np.float64)
            if closed and spec["kind"] == syn.PSI_HINGE_HALFSPACE:
                fs.fast_moments = hr.closed_form(spec["params"], spec["d"])
                fs.halfspace_params = spec["params"]                # ClosedProx
            out.append(fs)
        return out
    ch["oracle_sets"] = oracle_sets
    return ch


@functools.lru_cache(maxsize=None)
def corridor_graph(pair):
    """make_planar_chain(T = 9) -- the start path runs from (-3, -0.4) to (3, 0.4) -- with a corridor of four faces around the
    line y = 0.2 x, |x| bounded at 2.8: the start path leaves it at both ends.  pair: the corridor on the interpolated position
    at two times inside every segment instead (d = 8, J = 8)."""
    base = syn.make_planar_chain(T=9)
    if pair:
        ch = syn.add_corridor_set(base, NORMALS, OFFSETS, sigma=8.0, eps=0.05, p=3, pair=True, taus=[0.08, 0.17], dt=0.25)
    else:
        ch = syn.add_corridor_set(base, NORMALS, OFFSETS, sigma=8.0, eps=0.05, p=3)
    cor = ch["specs"][-1]
    Xk = np.stack([np.concatenate([base["mu0"][s:s + cor["d"] // 4].reshape(-1)]) for s in cor["start"]])[:, None, :]
    psi0, mg0 = hr.psi_batch(cor["params"], cor["d"])(Xk)[:, 0], hr.margin(cor["params"], cor["d"], Xk)[:, 0]
    assert (psi0 > 0).sum() >= 2 and mg0.min() < 0 < mg0.max()       # the start path violates the corridor, and not everywhere
    return attach_oracle(ch)


check_state = box_gpu.check_state


@pytest.mark.parametrize("pair,iters", [(False, 5), (True, 2)])
def test_iterations_vs_oracle(pair, iters):
    ch = corridor_graph(pair)
    for closed in (True, False):
        ctx, ids = api.context_for_chain(ch)
        ctx.factors_set_closed_form(ids[-1], int(closed))
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        chain = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](closed), ch["mu0"], ch["D0"], ch["U0"])
        log = []
        for it in range(iters):
            r = ctx.ngd_step(0.55, 10)
            ok, cost, ntr = chain.step()
            print(f"pair {pair} closed {closed} iteration {it}: device {r}, oracle {(ok, cost, ntr)}")
            assert r["accepted"] == ok and r["ntrials"] == ntr
            assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
            check_state(ctx, chain, f"pair {pair} closed {closed} iteration {it}")
            log.append(r)
        assert ctx.profile_geometry(ids[-1])["variant"] == (0 if closed else 1)
        assert ctx.ngd_factor_costs(ids[-1]).max() > 0              # the corridor is active on this path
        state = ctx.ngd_get_state()
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])                 # the same iterations in one call
        assert ctx.ngd_run(iters, 0.55, 10) == log
        st = ctx.ngd_get_state()
        assert all(np.array_equal(st[k], state[k]) for k in state)
        ctx.close()


class ClosedProx(box_gpu.ClosedProx):
    """The wrapper of tests/test_box_gpu.py with the raw integrals of a half-space set from halfspace_ref's closed form."""

    def raw(self, fs, mk, Sk):
        if getattr(fs, "halfspace_params", None) is not None:
            return hr.closed_moments(fs.halfspace_params, fs.d, mk, Sk, 1.0)
        return super().raw(fs, mk, Sk)


@pytest.mark.parametrize("closed", [True, False])
def test_prox_step_vs_oracle(closed):
    """One step under GVI_RULE_PROX_JKO with the corridor set on its default closed-form route (against ClosedProx) and on the
    quadrature route (against o.ChainProx as it is)."""
    ch = corridor_graph(False)
    ctx, ids = api.context_for_chain(ch)
    ctx.factors_set_closed_form(ids[-1], int(closed))
    ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    cls = ClosedProx if closed else o.ChainProx
    chain = cls(ch["T"], ch["n"], ch["oracle_sets"](closed), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.3)
    r = ctx.prox_step(0.3, 10)
    ok, cost, ntr = chain.step()
    print(f"closed {closed}: device {r}, oracle {(ok, cost, ntr)}")
    assert ctx.profile_geometry(ids[-1])["variant"] == (0 if closed else 1)
    assert r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9, atol=0)
    st = ctx.ngd_get_state()
    errs = [rel(st["mu"], chain.mu), rel(st["D"], chain.D)]
    print(f"closed {closed}: mu {errs[0]:.2e}, D {errs[1]:.2e}")
    assert max(errs) < RTOL / 10
    ctx.close()


# ---- posterior queries ----
def test_samples():
    ch = corridor_graph(False)
    T, n, S = ch["T"], ch["n"], 33
    cor = ch["specs"][-1]
    ctx, ids = api.context_for_chain(ch)
    sid = ids[-1]
    X = ctx.bt_sample(ch["D0"], ch["U0"], ch["mu0"], S, seed=4100)
    Xk = factor_slices(X, cor, n)
    ref_cost = (cor["psi_batch"](Xk) / np.asarray(cor["temperature"])[:, None]).T
    ref_mg = hr.margin(cor["params"], cor["d"], Xk).T
    share = float((ref_cost > 0).mean())
    print(f"share of (sample, factor) pairs with psi > 0: {share:.3f}; margin min {ref_mg.min():.3f} max {ref_mg.max():.3f}")
    assert 0.03 <= share <= 0.97 and ref_mg.min() < 0 < ref_mg.max()
    cost, mg = ctx.sample_factor_costs(sid, X), ctx.sample_clearance(sid, X)
    print(f"cost {rel(cost, ref_cost):.2e}; margin {rel(mg, ref_mg):.2e}")
    assert cost.shape == (S, T) and rel(cost, ref_cost) <= 1e-11 and rel(mg, ref_mg) <= 1e-13
    rows = [ctx.sample_factor_costs(s, X) for s in ids]
    Jrows = np.sum([r.sum(axis=1) for r in rows], axis=0)
    J = ctx.sample_costs(X)
    assert np.abs(J - Jrows).max() <= 1e-11 * np.abs(Jrows).max()
    assert (J - np.sum([r.sum(axis=1) for r in rows[:-1]], axis=0)).max() > 0          # the corridor set is part of J
    # a NaN and a +inf in the slices of factors 4 and 6 of samples 2 and 5: those entries are NaN, every other one is untouched
    Xb = X.copy()
    Xb[2, 4, 0], Xb[5, 6, 3] = np.nan, INF                                   # a position and a velocity (no row reads it)
    bad = np.zeros((S, T), dtype=bool)
    bad[2, 4] = bad[5, 6] = True
    for got, clean in ((ctx.sample_factor_costs(sid, Xb), cost), (ctx.sample_clearance(sid, Xb), mg)):
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean[~bad]) and np.isfinite(got[~bad]).all()
    Jb = ctx.sample_costs(Xb)
    assert np.isnan(Jb[[2, 5]]).all() and np.array_equal(np.delete(Jb, [2, 5]), np.delete(J, [2, 5]))
    # the resident call: clearance_set = the corridor set; the resident state is not touched
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    ctx.ngd_step(0.55, 10)
    before = ctx.ngd_get_state()
    r = ctx.ngd_sample_costs(S, seed=5, clearance_set=sid)
    after = ctx.ngd_get_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert np.array_equal(r["clr_min"], ctx.sample_clearance(sid, r["X"]).min(axis=1))
    assert rel(r["clr_min"], hr.margin(cor["params"], cor["d"], factor_slices(r["X"], cor, n)).min(axis=0)) <= 1e-13
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    ctx.close()
    # a set whose rows are all off: +inf margin, zero cost
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    free = ctx.factors_add(n, 3, np.arange(T, dtype=np.int32), api.PSI_HINGE_HALFSPACE, np.tile(syn.halfspace_params(0.0, 0.1, 1.0, np.eye(n)[:2]), (T, 1)))
    assert (ctx.sample_clearance(free, X) == INF).all() and (ctx.sample_factor_costs(free, X) == 0).all()
    ctx.close()


def test_shim_halfspace_callsite(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "halfspace_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "halfspace_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
