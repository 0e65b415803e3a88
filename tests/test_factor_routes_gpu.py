"""Route selection of the factor stage (routes.hpp decides, gvi_hip.hip binds and launches: plan_moments -> fuse -> launch_plan),
one row per compiled kernel instance and one leg per way the resident iteration fuses or does not fuse the sets' launches
(-m gpu).  The route model (_route, _chunks, the instance constants) is tests/route_model.py, which tests/test_routes_host.py
holds the header to on the CPU.

test_every_instance: single-set contexts through gvi_moments / gvi_costs.  A row is a (kind, d, p) that has an instance in one
of the lists of routes.hpp (with_reg_instance 24, with_sreg_instance 5, with_split_instance 6, with_orbit_instance one per
(m, support class), with_orbit_psi_instance 5); for every row the variants of {0, 1, 2, 5, 6, 7} that take different routes are
run, and each is held to (a) the kernel gvi_profile_geometry reports, (b) the chunking rule of that route, restated here in
Python (_chunks), for the full pass and for the cost pass, (c) the oracle's quadrature on the same table at the tolerance
tests/test_gpu_parity.py uses for the kind.  A pairing slip inside one list (d = 6 mapped to an instance of d = 8, say) changes
the numbers of exactly one row.  The route model (_route) restates plan_moments: closed form aside, sign-orbit kernel (variants
0, 6, 7; sum-of-squares kinds on a table of complete sign orbits, m in {2, 6, 12, 14}), its non-polynomial sibling (7),
lane-per-point kernels (SGPR operands under 0, 5, 7 where instantiated, the two-factor cost kernel for QUAD d = 12 / FIXED
d = 6), split kernel (d in {16, 20, 24} on a coded table), generic kernel.

test_refusals pins status and message of the four ways a pass is refused before anything is launched.

test_resident_fusing: two accepted gvi_ngd_step per leg on chains of T <= 5 (pr3d: its default 9), against the oracle chain at
the chain tests' bounds (cost 1e-9, state 1e-7; the arm-sized n = 14 chain 1e-8), with the kernel every set reports after a
cost pass and after a full pass, the pass counters, and the launch counters of factor_fused_kernel / factor_block3_kernel.
pair_fuse 0 / 1 end in the same bits (n = 6 chain with the sign-orbit kernel off, planning graph under fused 0).  The header's
switch table says the same of sreg_pipe and no_scost; on the n = 6, p = 3 chain they do NOT (measured on the library before
this module's refactor: new_cost 79.3604872386473 against ...728 and ...731) -- the hand-pipelined body sums mirror pairs of the
table and the two-factor cost kernel cuts eight times as many chunks, so the sums associate differently -- and they are held
to the bounds test_gpu_parity.py has for its switches (costs 1e-12, state 1e-10).  Two legs
hold the pair launch of two sign-orbit sets to what moments_orbit_pair_kernel is compiled for: n = 14 (no pair instance: the
m = 12 one ran on m = 14 data) and a unary factor with an indefinite weight (the pair kernel has no signed form: sgn was
ignored); both go out as two launches of the single kernel and agree with the oracle.
"""
import functools

import numpy as np
import pytest

import gvi_oracle as o
import segment_ref as sr
from chains import oracle_psi_batch, oracle_table
from gaussianvi_amd import api, synthetic as syn
from route_model import (ARM, BODY, CODE, FIXED, H2D, H3D, OPSI_ROWS, QUAD, RANGE, REG, SCOST, SEG2, SEG3, SPLIT_D, SREG, _chunks, _orbit_shape,
                         _route)
from test_gpu_parity import RTOL, TIGHT, quad_params, rel
from test_segment_gpu import field_of, operator_case, set_field

pytestmark = pytest.mark.gpu


# ---- single-set problems ----
F2 = dict(origin=(-5.0, -4.0), cell=0.1, field=syn.circle_sdf((-5.0, -4.0), 0.1, 81, 101, [(0.0, 1.6), (-1.0, -2.2)], [1.2, 0.9]))
FB = dict(origin=(-6.0, -5.0), cell=0.1, field=syn.circle_sdf((-6.0, -5.0), 0.1, 101, 121, [(0.0, 2.2), (-1.0, -3.0)], [1.2, 0.9]))
F3 = dict(origin=(-4.0, -3.0, -2.0), cell=0.2,
          field=syn.sphere_sdf3d((-4.0, -3.0, -2.0), 0.2, 31, 41, 21, [(0.0, 1.4, 0.3), (-0.5, -1.8, 0.0)], [1.0, 0.8]))
FA = dict(origin=(-1.5, -1.5, -0.5), cell=0.05,
          field=syn.sphere_sdf3d((-1.5, -1.5, -0.5), 0.05, 61, 61, 41, [(0.4, 0.2, 0.5), (-0.3, -0.4, 0.3)], [0.25, 0.2]))
POSES2 = [(0.0, 1.5), (0.1, 0.2), (-1.0, -1.2), (3.0, 3.0)]
POSESB = [(0.0, 1.9, 0.3), (0.1, 0.2, 1.2), (-1.0, -2.0, -0.7), (3.0, 3.0, 2.5)]
POSES3 = [(0.0, 1.3, 0.3), (0.1, 0.2, 0.1), (-0.5, -1.0, 0.2), (3.0, 2.0, 1.5)]
# tolerances of tests/test_gpu_parity.py per kind: (E[psi], Vdmu and cost, Vddmu)
TOL_TIGHT, TOL_WIDE, TOL_RANGE = (TIGHT, TIGHT, 10 * TIGHT), (1e-8, 1e-8, 1e-7), (1e-12, 1e-11, 1e-11)
D_GT_32 = (3, "factor dimension > 32")


@functools.lru_cache(maxsize=None)
def _problem(kind, d, p, K=4):
    """Operands, marginals, the oracle's moments (computed once, read-only) and how to finish the set (grid, arm)"""
    rng = np.random.default_rng(9000 + 100 * kind + 10 * d + p)
    finish, temp, n, tol = (lambda ctx, sid: None), np.ones(K), d, TOL_TIGHT
    mu, Sigma = syn.random_marginals(rng, K, d, 0.3 if kind in (QUAD, FIXED) else 0.2)
    if kind == QUAD:
        n = d // 2
        Phi, Qinv = quad_params(rng, K, n)
        params, psi, temp = np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1), o.psi_batch_quad_prior(Phi, Qinv), rng.uniform(0.5, 2.0, K)
    elif kind == FIXED:
        mu0, Kh = rng.normal(size=(K, d)), rng.normal(size=(K, d, d))
        Kinv = Kh @ np.transpose(Kh, (0, 2, 1)) / d + 0.3 * np.eye(d)
        params, psi = np.concatenate([mu0, Kinv.reshape(K, -1)], axis=1), o.psi_batch_fixed_prior(mu0, Kinv)
    elif kind == RANGE:                                                  # the K3 integrand of test_moments_range_1d_nonlinear
        y = 40.0 / 20.0 + 0.05
        params, psi, tol = np.tile([[y, 20.0, 40.0, 0.09, 9.0]], (K, 1)), o.psi_batch_range_1d(y), TOL_RANGE
        mu, Sigma = np.full((K, 1), 20.0) + np.arange(K)[:, None] * 0.25, np.full((K, 1, 1), 9.0)
    elif kind in (H2D, H3D, BODY):
        F, poses = {H2D: (F2, POSES2), BODY: (FB, POSESB), H3D: (F3, POSES3)}[kind]
        cols = [rng.uniform(5, 20, K), rng.uniform(0.2, 0.8, K), rng.uniform(0.1, 0.5, K)]
        if kind == BODY:
            cols += [np.full(K, 5.0), np.full(K, 5.0), rng.uniform(0.8, 2.0, K)]
        params = np.column_stack(cols)
        psi = {H2D: o.psi_batch_hinge_sdf2d, BODY: o.psi_batch_hinge_sdf2d_body, H3D: o.psi_batch_hinge_sdf3d}[kind](params, F["origin"], F["cell"], F["field"])
        mu[:, :len(poses[0])] = poses[:K]
        finish = lambda ctx, sid: (ctx.factors_set_sdf3d if kind == H3D else ctx.factors_set_sdf2d)(sid, F["origin"], F["cell"], F["field"])
    elif kind == ARM:
        arm = syn.wam_like_arm()
        params = np.column_stack([rng.uniform(5, 20, K), rng.uniform(0.05, 0.2, K)])
        psi, tol = o.psi_batch_hinge_sdf3d_arm(params, arm, FA["origin"], FA["cell"], FA["field"]), TOL_WIDE
        mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
        mu[:, :7] = rng.uniform(-1.2, 1.2, (K, 7))
        finish = lambda ctx, sid: (ctx.factors_set_sdf3d(sid, FA["origin"], FA["cell"], FA["field"]), ctx.factors_set_arm(sid, arm))
    else:
        P = 2 if kind == SEG2 else 3
        case = operator_case(P, d, 3, K)
        F = field_of(P)
        params, n, mu, Sigma, temp = case["params"], case["n"], case["mu"], case["Sigma"], case["temperature"]
        psi = sr.psi_batch_hinge_seg(params, P, d, F["origin"], F["cell"], F["field"])
        finish = lambda ctx, sid: set_field(ctx, sid, P)
    if kind in (QUAD, FIXED) and (d >= 16 or p > 5):                     # |w|_1 grows with d and p: the sums carry more rounding
        tol = TOL_WIDE
    Z, w = oracle_table(d, p)
    ref = o.batched_moments(Z, w, mu, Sigma, psi, temp)
    for a in (mu, Sigma, params, temp) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return dict(kind=kind, d=d, m=(n if kind == QUAD else d), p=p, K=K, n=n, params=params, temp=temp, mu=mu, Sigma=Sigma, Z=Z, ref=ref,
                finish=finish, tol=tol)


def _context(P):
    ctx = api.Context(0)
    ctx.chain_set(2 if P["d"] == 2 * P["n"] else 1, P["n"])
    sid = ctx.factors_add(P["d"], P["p"], np.zeros(P["K"], dtype=np.int32), P["kind"], P["params"], P["temp"])
    return ctx, sid


# one row per compiled instance: (kind, d, p), then the list it stands for.  p = 3 unless the instance needs another table
# (supports of 5, 6 nodes need degree >= 6; p = 2 has no Cholesky route)
ROWS = ([("reg", k, d, 3) for k in (RANGE, H2D, BODY, H3D, SEG2, SEG3, QUAD, FIXED) for d in REG[k]] +
        [("split", QUAD, d, 3) for d in SPLIT_D] + [("split", FIXED, d, 3) for d in SPLIT_D] +
        [("orbit", QUAD, 4, 5), ("orbit", FIXED, 6, 5), ("orbit", FIXED, 6, 6), ("orbit", FIXED, 12, 5), ("orbit", FIXED, 12, 6),
         ("orbit", QUAD, 28, 3)] +
        [("opsi", RANGE, 1, 5), ("opsi", H2D, 4, 4), ("opsi", BODY, 3, 4), ("opsi", H3D, 3, 4), ("opsi", ARM, 7, 3)])
KNAME = {QUAD: "quad", FIXED: "fixed", RANGE: "range", H2D: "sdf2d", BODY: "body", H3D: "sdf3d", ARM: "arm", SEG2: "seg2", SEG3: "seg3"}


def test_the_rows_cover_every_list():
    assert sum(r[0] == "reg" for r in ROWS) == 24 == sum(len(v) for v in REG.values())
    assert sum(r[0] == "reg" and r[2] in SREG.get(r[1], ()) for r in ROWS) == 5        # the sreg instances ride on their reg rows
    assert sum(r[0] == "split" for r in ROWS) == 6
    shapes = {((r[2] // 2 if r[1] == QUAD else r[2]), _orbit_shape(oracle_table(r[2], r[3])[0])[0] > 4) for r in ROWS if r[0] == "orbit"}
    assert shapes == {(2, False), (6, False), (6, True), (12, False), (12, True), (14, False)}
    assert {r[1] for r in ROWS if r[0] == "opsi"} == set(OPSI_ROWS)


@pytest.mark.parametrize("family,kind,d,p", ROWS, ids=[f"{r[0]}-{KNAME[r[1]]}-d{r[2]}-p{r[3]}" for r in ROWS])
def test_every_instance(family, kind, d, p):
    P = _problem(kind, d, p)
    K, Z, ref, (tolE, tol, tolV) = P["K"], P["Z"], P["ref"], P["tol"]
    ctx, sid = _context(P)
    try:
        P["finish"](ctx, sid)
        seen = set()
        for variant, orbit_on in [(0, True), (0, False), (1, True), (2, True), (5, True), (6, True), (7, True)]:
            route = _route(kind, d, P["m"], Z, variant, orbit_on)
            cost_route = _route(kind, d, P["m"], Z, variant, orbit_on, full=False)
            if route is None or (route, cost_route) in seen:
                continue
            seen.add((route, cost_route))
            ctx.set_variant(variant)
            ctx.set_option("orbit", int(orbit_on))
            Ephi, Vdmu, Vddmu = ctx.moments(sid, P["mu"], P["Sigma"])
            geo = ctx.profile_geometry(sid)
            cost = ctx.costs(sid, P["mu"], P["Sigma"])
            geo_cost = ctx.profile_geometry(sid)
            want = _chunks(route, K, Z)
            want_cost = _chunks(cost_route, K, Z, want[0])
            errs = (rel(Ephi, ref["E_phi"]), rel(Vdmu, ref["Vdmu"]), rel(Vddmu, ref["Vddmu"]), rel(cost, ref["cost"]))
            print(f"    variant {variant} orbit {int(orbit_on)}: {route} / {cost_route}, geometry {geo} / {geo_cost}, errors " +
                  " ".join(f"{e:.1e}" for e in errs))
            assert geo == dict(variant=CODE[route], nchunk=want[0], chunk=want[1]), (variant, route, geo, want)
            assert geo_cost == dict(variant=CODE[cost_route], nchunk=want_cost[0], chunk=want_cost[1]), (variant, cost_route, geo_cost, want_cost)
            assert errs[0] < tolE and errs[1] < tol and errs[2] < tolV and errs[3] < tol, (variant, route, errs)
            assert np.array_equal(Vddmu, np.transpose(Vddmu, (0, 2, 1)))
        routes = {r for pair in seen for r in pair}
        assert family in routes, seen                                    # the instance the row stands for ran
        if family == "reg" and d in SREG.get(kind, ()):
            assert "sreg" in routes, seen                                # and the SGPR-operand instance of the same (kind, d)
        if family == "reg" and d in SCOST.get(kind, ()):
            assert "scost" in routes, seen
    finally:
        ctx.close()


def test_a_fresh_set_reports_the_default_record():
    """Before any pass gvi_profile_geometry reports the default PassRecord: generic kernel (closed form: 0), one chunk, chunk 0"""
    P = _problem(FIXED, 2, 3, K=2)
    for closed, want in [(False, dict(variant=1, nchunk=1, chunk=0)), (True, dict(variant=0, nchunk=1, chunk=0))]:
        ctx, sid = _context(P)
        try:
            ctx.factors_set_closed_form(sid, closed)
            assert ctx.profile_geometry(sid) == want, (closed, ctx.profile_geometry(sid))
        finally:
            ctx.close()


def _refused(ctx, call):
    with pytest.raises(api.GviError) as e:
        call()
    print(f"    refused: {e.value}")
    return e.value.status, str(e.value).split(": ", 1)[1]


def test_refusals():
    """Status and message of a pass that is refused before anything is launched"""
    P = _problem(H2D, 8, 3)                                              # a hinge set without a grid; with one, no register instance at d = 8
    ctx, sid = _context(P)
    try:
        assert _refused(ctx, lambda: ctx.moments(sid, P["mu"], P["Sigma"])) == \
            (5, "HINGE_SDF set without a grid: call gvi_factors_set_sdf2d / gvi_factors_set_sdf3d")
        P["finish"](ctx, sid)
        ctx.set_variant(2)
        for call in (lambda: ctx.moments(sid, P["mu"], P["Sigma"]), lambda: ctx.costs(sid, P["mu"], P["Sigma"])):
            assert _refused(ctx, call) == (3, "register kernel not instantiated for this (kind, d)")
        ctx.set_variant(0)
        assert rel(ctx.costs(sid, P["mu"], P["Sigma"]), P["ref"]["cost"]) < TIGHT          # and the context goes on working
    finally:
        ctx.close()
    P = _problem(ARM, 7, 3)
    ctx, sid = _context(P)
    try:
        ctx.factors_set_sdf3d(sid, FA["origin"], FA["cell"], FA["field"])
        assert _refused(ctx, lambda: ctx.moments(sid, P["mu"], P["Sigma"])) == \
            (5, "HINGE_SDF_3D_ARM set without an arm model: call gvi_factors_set_arm")
    finally:
        ctx.close()
    ctx = api.Context(0)                                                 # d > 32
    try:
        ctx.chain_set(1, 34)
        rng = np.random.default_rng(34)
        status, msg = _refused(ctx, lambda: ctx.moments(ctx.factors_add(34, 2, np.zeros(2, dtype=np.int32), FIXED, np.concatenate(
            [rng.normal(size=(2, 34)), np.stack([np.eye(34)] * 2).reshape(2, -1)], axis=1)), *syn.random_marginals(rng, 2, 34, 0.3)))
        assert (status, msg) == D_GT_32, (status, msg)
    finally:
        ctx.close()


# ---- the resident iteration ----
def _chain(name, T=None, n=None, p=None, kind="ltv"):
    """gaussianvi_amd.synthetic chain with the oracle's closures; (T, n, p): a CONFIGS entry made here, as make_chain does for c3x*"""
    if name == "planar":
        ch = syn.make_planar_chain(T=5)
    elif name == "pr3d":
        ch = syn.make_obstacle_chain("pr3d")
    else:
        if name not in syn.CONFIGS:
            syn.CONFIGS[name] = (700 + 10 * n + T, T, n, p, kind)
        ch = syn.make_chain(name)
    return ch


def _oracle_sets(ch, tables=None):
    out = []
    for i, spec in enumerate(ch["specs"]):
        fs = o.FactorSet(spec["start"], spec["d"], spec["p"], oracle_psi_batch(spec))
        fs.temperature = np.asarray(spec["temperature"], dtype=np.float64)
        if tables and i in tables:
            fs.Z, fs.w = tables[i]
        out.append(fs)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_run(name, steps=2):
    """The oracle's two steps on the leg's chain, computed once and shared by the legs of that chain"""
    ch, tables = CHAINS[name]()
    chain = o.ChainNGD(ch["T"], ch["n"], _oracle_sets(ch, tables), ch["mu0"], ch["D0"], ch["U0"])
    log = [chain.step() for _ in range(steps)]
    eig = np.linalg.eigvalsh(o.bt_to_dense(chain.D, chain.U)).min()
    state = dict(mu=chain.mu.copy(), D=chain.D.copy(), U=chain.U.copy(), SigD=chain.SigD.copy())
    for a in state.values():
        a.setflags(write=False)
    return ch, tables, log, state, eig


def _indefinite_unary():
    """n = 6, T = 3: the unary factor on the middle state has a weight with ONE small negative eigenvalue (sgn = -1 for that
    residual row, so the set is not all_pos); the chain's precision stays positive definite (asserted on the oracle's iterates)"""
    ch = _chain("r6t3", 3, 6, 3)
    spec = ch["specs"][1]
    Q = np.linalg.qr(np.random.default_rng(63).normal(size=(6, 6)))[0]
    Kinv = spec["Kinv"].copy()
    Kinv[1] = Q @ np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -0.05]) @ Q.T
    Kinv[1] = 0.5 * (Kinv[1] + Kinv[1].T)
    spec["Kinv"] = Kinv
    spec["params"] = np.concatenate([spec["mu0"], Kinv.reshape(3, -1)], axis=1)
    return ch, None


def _caller_table():
    """n = 6, T = 5: the unary set on a caller's table whose row 3 carries another weight than the rest of its sign orbit"""
    ch = _chain("r6t5", 5, 6, 3)
    Z, w = oracle_table(6, 3)
    w = w.copy()
    w[3] *= 1.0 + 1e-3
    return ch, {1: (Z, w)}


CHAINS = {
    "n6": lambda: (_chain("r6t5", 5, 6, 3), None),
    "n2": lambda: (_chain("tiny"), None),
    "n4": lambda: (_chain("r4t5", 5, 4, 3, "minacc"), None),
    "n6table": _caller_table,
    "planar": lambda: (_chain("planar"), None),
    "pr3d": lambda: (_chain("pr3d"), None),
    "n14": lambda: (_chain("r14t3", 3, 14, 3), None),
    "n6signed": _indefinite_unary,
}

# leg: (chain, options, kernel per set after a cost pass, after a full pass, launches of (fused [0], [1], [2], block3) per full pass)
ORBIT0 = dict(orbit=0, fuse_trial=0)
LEGS = {
    "n6": ("n6", {}, (6, 6), (6, 6), (1, 0, 0, 0)),
    "n6-fused0": ("n6", dict(fused=0), (6, 6), (6, 6), (0, 0, 0, 0)),
    "n6-orbit0": ("n6", ORBIT0, (5, 5), (5, 5), (0, 0, 0, 0)),
    "n6-orbit0-pipe0": ("n6", dict(ORBIT0, sreg_pipe=0), (5, 5), (5, 5), (0, 0, 0, 0)),
    "n6-orbit0-noscost": ("n6", dict(ORBIT0, no_scost=1), (2, 2), (5, 5), (0, 0, 0, 0)),
    "n6-orbit0-nopair": ("n6", dict(ORBIT0, pair_fuse=0), (2, 2), (2, 2), (0, 0, 0, 0)),
    "n2": ("n2", {}, (6, 6), (6, 6), (0, 0, 1, 0)),
    "n2-orbit0": ("n2", dict(orbit=0), (2, 2), (2, 2), (0, 0, 0, 0)),
    "n4": ("n4", {}, (2, 2), (2, 2), (0, 0, 0, 0)),
    "n6table": ("n6table", {}, (6, 2), (6, 2), (0, 0, 0, 0)),
    "planar": ("planar", {}, (2, 2, 2), (2, 2, 2), (0, 0, 0, 1)),
    "planar-fused0": ("planar", dict(fused=0), (2, 2, 2), (2, 2, 2), (0, 0, 0, 0)),
    "planar-variant7": ("planar", dict(set_variant=7), (2, 7, 2), (2, 7, 2), (0, 0, 0, 0)),
    "planar-nopair": ("planar", dict(pair_fuse=0), (2, 2, 2), (2, 2, 2), (0, 0, 0, 0)),
    "pr3d": ("pr3d", {}, (6, 2, 6), (6, 2, 6), (0, 0, 0, 0)),
    "n14": ("n14", {}, (6, 6), (6, 6), (0, 0, 0, 0)),
    "n6signed": ("n6signed", {}, (6, 6), (6, 6), (0, 0, 0, 0)),
}
PAIR_BUGS = ("n14", "n6signed")                                          # the two corrected pair conditions
SAME_BITS = [("n6-orbit0", "n6-orbit0-nopair"), ("planar-fused0", "planar-nopair")]
SAME_TO_ROUNDING = [("n6-orbit0", "n6-orbit0-pipe0"), ("n6-orbit0", "n6-orbit0-noscost")]


def _launches():
    return tuple(api.fused_launches()) + (api.block3_launches(),)


@functools.lru_cache(maxsize=None)
def _device_run(leg):
    name, options, _, _, _ = LEGS[leg]
    ch, tables, _, _, _ = _oracle_run(name)
    options = dict(options)
    ctx, ids = api.context_for_chain(ch)
    try:
        if tables:
            for sid, (Z, w) in tables.items():
                ctx.factors_set_table(ids[sid], Z, w)
        if "set_variant" in options:
            ctx.set_variant(options.pop("set_variant"))
        if "fuse_trial" in options:
            ctx.ngd_set_mode(True, options.pop("fuse_trial"))
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        ctx.ngd_counters(reset=True)
        out = dict(cost0=ctx.ngd_cost())
        out["after_cost"] = [ctx.profile_geometry(s)["variant"] for s in ids]
        # (a full pass at a state whose products a cost pass left resident skips the one-launch kernels: start afresh)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        c0 = _launches()
        ctx.ngd_gradients()
        out["per_full_pass"] = tuple(b - a for a, b in zip(c0, _launches()))
        out["after_full"] = [ctx.profile_geometry(s)["variant"] for s in ids]
        out["counters_1"] = tuple(ctx.ngd_counters())
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        c0 = _launches()
        out["log"] = [ctx.ngd_step(0.55, 10) for _ in range(2)]
        out["launches"] = tuple(b - a for a, b in zip(c0, _launches()))
        out["counters"] = tuple(ctx.ngd_counters())
        out["state"] = ctx.ngd_get_state()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("leg", list(LEGS))
def test_resident_fusing(leg):
    name, options, after_cost, after_full, per_pass = LEGS[leg]
    ch, _, log, state, eig = _oracle_run(name)
    assert eig > 0 and all(ok for ok, _, _ in log), (eig, log)           # two accepted steps, precision positive definite
    R = _device_run(leg)
    nfull, ncost = R["counters"]
    print(f"    {leg}: kernels after a cost pass {R['after_cost']}, after a full pass {R['after_full']}, passes (full, cost) {R['counters_1']} "
          f"-> {R['counters']}, launches per full pass {R['per_full_pass']}, over the steps {R['launches']}, trials {[r['ntrials'] for r in R['log']]}")
    assert tuple(R["after_cost"]) == after_cost and tuple(R["after_full"]) == after_full
    assert R["counters_1"] == (1, 1) and R["per_full_pass"] == per_pass
    # the two steps: a one-launch leg went through its kernel in each (the trial's full pass), no other leg touched one
    assert nfull - 1 >= 2 and all((c >= 2) if one else (c == 0) for c, one in zip(R["launches"], per_pass)), (R["launches"], nfull)
    if options.get("fuse_trial") == 0:
        assert ncost - 1 >= sum(r["ntrials"] for r in R["log"])           # reference pass order: one cost pass per trial
    ctol, stol = (1e-8, RTOL / 10) if ch["n"] == 14 else (1e-9, RTOL / 10)
    for r, (ok, cost, ntr) in zip(R["log"], log):
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=ctol), (r["new_cost"], cost)
    errs = {k: rel(R["state"][k], state[k]) for k in ("mu", "D", "U", "SigD")}
    print("    state against the oracle: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < stol, errs


@pytest.mark.parametrize("a,b", SAME_BITS, ids=[f"{a}={b}" for a, b in SAME_BITS])
def test_pair_fuse_legs_end_in_the_same_bits(a, b):
    Ra, Rb = _device_run(a), _device_run(b)
    assert Ra["log"] == Rb["log"] and Ra["cost0"] == Rb["cost0"]
    assert all(np.array_equal(Ra["state"][k], Rb["state"][k]) for k in Ra["state"])


@pytest.mark.parametrize("a,b", SAME_TO_ROUNDING, ids=[f"{a}~{b}" for a, b in SAME_TO_ROUNDING])
def test_body_and_cost_kernel_switches_agree_to_rounding(a, b):
    Ra, Rb = _device_run(a), _device_run(b)
    assert np.isclose(Ra["cost0"], Rb["cost0"], rtol=1e-12)
    for ra, rb in zip(Ra["log"], Rb["log"]):
        assert (ra["accepted"], ra["ntrials"]) == (rb["accepted"], rb["ntrials"])
        assert np.isclose(ra["new_cost"], rb["new_cost"], rtol=1e-12) and np.isclose(ra["cost_iter"], rb["cost_iter"], rtol=1e-12)
    errs = {k: rel(Ra["state"][k], Rb["state"][k]) for k in Ra["state"]}
    print("    " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < 1e-10, errs
