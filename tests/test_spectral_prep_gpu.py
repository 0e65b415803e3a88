"""The per-factor spectral stage (kernels_prep.hpp: prep_body<EPLP, DT>, the one-wave cyclic Jacobi; jko_half_kernel /
jko_finish_kernel around it) at every block size class and on the inputs where an eigen-solver goes wrong (-m gpu).

Sizes D_ALL = 1..17, 20, 24, 28, 31, 32: every unrolled instance (2, 4, 6, 12), odd d -- the phantom rotation partner dp = d + 1
-- in all three element layouts (EPLP = 1 for d <= 8, 4 for d <= 16, 16 for d <= 32), the full-lane sizes 8 / 16 / 32 and the
first size of each layout (9, 17).  Inputs (tests/spectral_ref.py): well- and ill-conditioned (1e4, 1e8), two clusters of equal
eigenvalues, 0.7 I and a diagonal matrix (the sweep-0 exit), diagonal + 1e-9 (rotations with |theta| ~ 1e9; the identity
branch |theta| >= 1e150 needs |a_pq| < 1e-150 |a_qq - a_pp|, and the stopping rule off^2 <= 1e-34 diag^2 ends the sweeps long
before an off-diagonal entry is that small: no input here reaches it, and none that is not denormal-sized could),
Sigma scaled by 1e-12 and 1e+12 (the relative stopping rule, the rcp / rsq + Newton ranges).

A row's bound is max(floor, 32 * ref_err): floor is the tolerance the suite already used for the quantity, ref_err the error of
the float64 restatement the device is compared with (oracle/gvi_oracle.py) against a 50-digit mpmath reference, recorded in
tests/golden/spectral_ref_err.json and re-derived by tests/test_spectral_host.py; the margin 32 covers the different, equally
legitimate summation and rotation orders of a Jacobi solve against LAPACK.  Every row prints `ROW <key> dev <device error> ref
<ref_err> bound <bound>` before anything is asserted; the figures measured on the MI355X are in profiles/spectral_stage_tests.txt.

test_nodes            gvi_expand of a HOST_CALLBACK set at p = 2 (2 d + 1 points; 2 at d = 1) against mu + Z sym_sqrt(Sigma), relative to
                      max |X - mu|, floor 1e-12; a second call and a call with the strict upper triangle of Sigma overwritten
                      (the kernel reads the lower triangle only) return the same bits.
test_inverse_outputs  Sinv and Lam through gvi_moments_from_psi on psi = log(1 + |x - c|^2) + sin(a . x), evaluated on the
                      host at the device's own nodes (at p = 2 the rule does not integrate it exactly, so S matters), against
                      o.batched_moments; floors TIGHT, TIGHT, 10 TIGHT (cond1e4: 1e-7); Vddmu exactly symmetric.  d = 1: the
                      rule's nodes are +-1, Vddmu vanishes identically and is measured against |Lam E_phi|.
test_indefinite_input one negated eigenvalue gives NaN nodes for that factor (the reference's operatorSqrt), GVI_OK, the factor
                      beside it and the next call are untouched.
test_resident_*       T = 3 chains (QUAD_PRIOR d = 2 n, FIXED_PRIOR d = n, p = 3) at n = 3, 6, 9, 10, 16: ngd_prep_all picks the
                      layout from the LARGEST d, so d = 6 beside d = 12 runs <4, 6> and d = 16 beside d = 32 runs <16, 0>.  Three
                      accepted ngd_step on the Cholesky route (a), under chol_sqrt = 0 with the warm start from the second pass on
                      (b) and without it (c): each against o.ChainNGD at the chain tests' bounds, (b) and (c) against (a) at the
                      bounds of test_cholesky_route_ngd_iterations_match_symmetric_root, (b) again from ngd_init: same bits.
test_jko_map          a chain with ONE factor makes the assembled prox increments that factor's own outputs (T = 1 FIXED_PRIOR,
                      d = n: g = Vdmu, VD[0] = Vddmu; T = 2 QUAD_PRIOR, d = 2 n: VD[0], VU[0], VD[1] its blocks; the chain
                      kernels stop at n = 16, hence unary d <= 16 and binary d <= 32).  (D, U) are the blocks of the inverse of a
                      `well` / `cond1e4` Sigma, the factor carries temperature 3.7, which the rule must ignore; h = 0.55, 1e-2,
                      1e-4 (where (Lam_new - Lam) / h cancels) against o.bw_jko on the oracle's unit-temperature moments: g to
                      TIGHT, VD and VU to max(1e-8, 32 ref_err); diagonal blocks symmetric to the last bit; second call same bits.
                      No row has a singular I - h S: there l (l + 4h) can round negative and both restatements give NaN.
test_prox_step_wide   one gvi_prox_step on the d = 18 and d = 32 binary chains with a unary set, against o.ChainProx.
test_rule_is_a_property_of_the_context
                      the same graph (n = 2, 6; every factor at temperature 3.7) built with the rule selected after the sets,
                      before them, and before a second gvi_chain_set: prox increments, gvi_ngd_factor_costs and
                      gvi_sample_factor_costs agree bit for bit and with the unit-temperature oracle; back under GVI_RULE_NGD the
                      sets divide by 3.7 again.  Before this module the second and third order kept the sets' own temperatures
                      (FactorSet::unit_temperature was only written by gvi_ngd_set_update_rule, for the sets that existed).

Measured on the MI355X (profiles/spectral_stage_tests.txt): no row exceeds its bound.  Nodes stay under 8e-13 (the cond1e8 rows,
whose reference itself carries 8e-13; every other class under 2e-14), the moment rows under 1.3e-10 (cond1e4) and 2e-13 (the
rest).  The JKO rows closest to their bound are cond1e4 at h = 1e-4 (8.9e-9 at unary d = 16, 8.4e-9 at binary d = 32, floor 1e-8).
That is not the spectral stage: device and oracle each invert (D, U) for the marginal (relative error eps cond = 1e-12 each, by
different eliminations), and for small h Vddmu ~ Lam S + S Lam - 2 Lam^2 moves by 2 cond times the relative change of Sigma, 2e-8
in the worst direction; the `well` rows stay under 1.5e-11 at every size and h.  A second call gives the same bits (asserted row by
row) and two separate runs printed the same figures, so the margin is not a matter of luck.

On the library of the commit before this module, the four rule-before-sets rows of test_rule_is_a_property_of_the_context
fail (n = 2, 6; "rule-sets", "rule-chain_set-sets") and everything else passes.

Sensitivity: four arithmetic-only edits to a scratch copy of the prep source (kernels_prep.hpp today), each run once on this module (124 tests):
  l + 2h for l + 4h in the JKO spectral function   all 117 JKO rows exceed (39 test_jko_map), test_prox_step_wide [9, 16], the six
                                                   test_rule_is_a_property_of_the_context (their prox half); nothing else
  jko_half_kernel forming I + h S                  the same 47 tests, all 117 JKO rows
  cold start reading Sg[j d + i] for i >= j        the triangle assertion of test_nodes at every d >= 2 (21 tests; d = 1 has no
                                                   triangle); all 194 node rows, run-to-run and everything else pass
  1 / l for 1 / sqrt(l) (second spectral output)   all 86 moment rows (test_inverse_outputs at all 22 sizes) and the symmetric-root
                                                   legs b, c of the resident rows (20 tests); all 194 node rows and the JKO rows pass
"""
import functools

import numpy as np
import pytest

import gvi_oracle as o
import spectral_ref as sp
from chains import oracle_psi_batch, oracle_table
from gaussianvi_amd import api
from test_gpu_parity import RTOL, TIGHT, quad_params, rel

pytestmark = pytest.mark.gpu

NODE_ROWS, MOMENT_ROWS, JKO_ROWS = sp.node_rows(), sp.moment_rows(), sp.jko_rows()
JKO_CASES = sorted({r[1:4] for r in JKO_ROWS}, key=lambda c: (c[0], c[1], c[2]))
RESIDENT_N = (3, 6, 9, 10, 16)
KIND = {"u": api.PSI_FIXED_PRIOR, "b": api.PSI_QUAD_PRIOR}


def _row(row, dev, floor):
    """Print the row's figures; return what is wrong with it (None: inside its bound)"""
    ref, b = sp.recorded()[sp.key(row)], sp.bound(row, floor)
    print(f"    ROW {sp.key(row)} dev {dev:.2e} ref {ref:.2e} bound {b:.2e}")
    return None if dev < b else (sp.key(row), dev, b)


def _none(problems):
    problems = [p for p in problems if p is not None]
    assert not problems, problems


# ---- operator rows: one context per d, factor k carries class k ----
@functools.lru_cache(maxsize=None)
def _operator_run(d):
    C = sp.operator_case(d)
    K = len(C["names"])
    Z, w = oracle_table(d, 2)
    psi = sp.psi_smooth(C["a"], C["c"])
    ref = o.batched_moments(Z, w, C["mu"], C["Sigma"], psi, np.ones(K))
    upper = C["Sigma"].copy()
    iu = np.triu_indices(d, 1)
    upper[:, iu[0], iu[1]] = np.random.default_rng(d).uniform(-3.0, 3.0, (K, len(iu[0])))
    ctx = api.Context(0)
    try:
        ctx.chain_set(1, d)
        sid = ctx.factors_add(d, 2, np.zeros(K, dtype=np.int32), api.PSI_HOST_CALLBACK)
        X = ctx.expand(sid, C["mu"], C["Sigma"])
        X2 = ctx.expand(sid, C["mu"], C["Sigma"])
        X3 = ctx.expand(sid, C["mu"], upper)
        got = ctx.moments_from_psi(sid, C["mu"], C["Sigma"], psi(np.transpose(X, (0, 2, 1))))
    finally:
        ctx.close()
    Xref = C["mu"][:, :, None] + np.stack([o.sym_sqrt(S) for S in C["Sigma"]]) @ Z.T
    return dict(C=C, X=X, X2=X2, X3=X3, Xref=Xref, got=got, ref=ref, N=len(w))


@pytest.mark.parametrize("d", sp.D_ALL)
def test_nodes(d):
    R = _operator_run(d)
    C, X, Xref = R["C"], R["X"], R["Xref"]
    assert X.shape == Xref.shape == (len(C["names"]), d, R["N"]) and R["N"] == (2 * d + 1 if d > 1 else 2)
    problems = []
    for k, cls in enumerate(C["names"]):
        err = np.abs(X[k] - Xref[k]).max() / np.abs(Xref[k] - C["mu"][k][:, None]).max()
        problems.append(_row(("nodes", d, cls), err, 1e-12))
    _none(problems)
    assert np.array_equal(X, R["X2"]), "a second call gives other bits"
    assert np.array_equal(X, R["X3"]), "the strict upper triangle of Sigma was read"


@pytest.mark.parametrize("d", sp.D_ALL)
def test_inverse_outputs(d):
    R = _operator_run(d)
    C, (Ephi, Vdmu, Vddmu), ref = R["C"], R["got"], R["ref"]
    problems = []
    for k, cls in enumerate(C["names"]):
        if cls not in sp.MOMENT_CLASSES:
            continue
        row = ("moments", d, cls)
        fE, fV, fVV = (1e-7, 1e-7, 1e-7) if cls == "cond1e4" else (TIGHT, TIGHT, 10 * TIGHT)
        eVV = rel(Vddmu[k], ref["Vddmu"][k])
        if d == 1:
            eVV = abs(Vddmu[k, 0, 0] - ref["Vddmu"][k, 0, 0]) / sp.vddmu_scale_1d(C["Sigma"][k], ref["E_phi"][k])
        errs = (rel(Ephi[k], ref["E_phi"][k]), rel(Vdmu[k], ref["Vdmu"][k]), eVV)
        print(f"    {sp.key(row)}: E_phi {errs[0]:.2e} Vdmu {errs[1]:.2e} Vddmu {errs[2]:.2e}")
        problems.append(_row(row, max(errs), fVV))
        problems += [None if e < sp.bound(row, f) else (sp.key(row), q, e) for q, e, f in zip(("E_phi", "Vdmu"), errs, (fE, fV))]
    _none(problems)
    assert np.array_equal(Vddmu, np.transpose(Vddmu, (0, 2, 1)))


@pytest.mark.parametrize("d", [5, 12, 24])
def test_indefinite_input(d):
    C = sp.operator_case(d)
    good = C["Sigma"][C["names"].index("well")]
    lam, V = np.linalg.eigh(good)
    lam[d // 2] = -lam[d // 2]
    bad = (V * lam) @ V.T
    bad = 0.5 * (bad + bad.T)
    mu = np.stack([C["mu"][0], C["mu"][0]])
    Z = oracle_table(d, 2)[0]
    ctx = api.Context(0)
    try:
        ctx.chain_set(1, d)
        sid = ctx.factors_add(d, 2, np.zeros(2, dtype=np.int32), api.PSI_HOST_CALLBACK)
        X = ctx.expand(sid, mu, np.stack([bad, good]))                   # returns GVI_OK: no exception
        Xn = ctx.expand(sid, mu, np.stack([good, good]))
    finally:
        ctx.close()
    Xref = mu[0][:, None] + o.sym_sqrt(good) @ Z.T
    assert np.isnan(X[0]).all(), "a negative eigenvalue must give NaN nodes, as the reference's operatorSqrt"
    scale = np.abs(Xref - mu[0][:, None]).max()
    for got in (X[1], Xn[0], Xn[1]):
        assert np.isfinite(got).all() and np.abs(got - Xref).max() < 1e-12 * scale
    assert np.array_equal(X[1], Xn[1]) and np.array_equal(Xn[0], Xn[1])


# ---- small graphs: T states, one QUAD_PRIOR set (d = 2 n) and one FIXED_PRIOR set on every state (d = n), p = 3 ----
@functools.lru_cache(maxsize=None)
def _graph(T, n, seed, temp=None):
    """Seeded well-conditioned data; every factor its own temperature in [0.5, 2] (temp: that value for all); the start is
    0.7 x the sum of the factors' Hessians, positive definite"""
    rng = np.random.default_rng(seed)
    K = T - 1
    Phi, Qinv = quad_params(rng, K, n)
    mu_u, G = rng.normal(size=(T, n)), rng.normal(size=(T, n, n))
    Kinv = G @ G.transpose(0, 2, 1) / n + 1.5 * np.eye(n)
    tb, tu = (rng.uniform(0.5, 2.0, K), rng.uniform(0.5, 2.0, T)) if temp is None else (np.full(K, temp), np.full(T, temp))
    D0, U0 = 2.0 * Kinv / tu[:, None, None], np.zeros((K, n, n))
    for k in range(K):
        J = np.concatenate([Phi[k], -np.eye(n)], axis=1)
        M = J.T @ Qinv[k] @ J / tb[k]
        D0[k] += M[:n, :n]
        D0[k + 1] += M[n:, n:]
        U0[k] += M[:n, n:]
    specs = [dict(kind=api.PSI_QUAD_PRIOR, d=2 * n, p=3, start=np.arange(K, dtype=np.int32), temperature=tb, Phi=Phi, Qinv=Qinv,
                  params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1)),
             dict(kind=api.PSI_FIXED_PRIOR, d=n, p=3, start=np.arange(T, dtype=np.int32), temperature=tu, mu0=mu_u, Kinv=Kinv,
                  params=np.concatenate([mu_u, Kinv.reshape(T, -1)], axis=1))]
    ch = dict(T=T, n=n, specs=specs, mu0=0.3 * rng.normal(size=(T, n)), D0=0.7 * D0, U0=0.7 * U0)
    for a in (ch["mu0"], ch["D0"], ch["U0"]):
        a.setflags(write=False)
    return ch


def _oracle_sets(ch, temp=None):
    out = []
    for spec in ch["specs"]:
        fs = o.FactorSet(spec["start"], spec["d"], spec["p"], oracle_psi_batch(spec))
        fs.temperature = np.asarray(spec["temperature"], dtype=np.float64) if temp is None else np.full(len(spec["start"]), temp)
        out.append(fs)
    return out


def _add_sets(ctx, ch):
    return [ctx.factors_add(s["d"], s["p"], s["start"], s["kind"], s["params"], s["temperature"]) for s in ch["specs"]]


# ---- resident rows ----
STEPS = 3
LEG_OPTIONS = {"a": {}, "b": dict(chol_sqrt=0), "c": dict(chol_sqrt=0, warm_start=0)}


@functools.lru_cache(maxsize=None)
def _resident_oracle(n):
    ch = _graph(3, n, 7300 + n)
    chain = o.ChainNGD(ch["T"], ch["n"], _oracle_sets(ch), ch["mu0"], ch["D0"], ch["U0"])
    log = [chain.step() for _ in range(STEPS)]
    state = dict(mu=chain.mu.copy(), D=chain.D.copy(), U=chain.U.copy(), SigD=chain.SigD.copy())
    for a in state.values():
        a.setflags(write=False)
    return ch, log, state


@functools.lru_cache(maxsize=None)
def _resident_run(n, leg):
    ch = _resident_oracle(n)[0]
    ctx, _ = api.context_for_chain(ch)
    try:
        for k, v in LEG_OPTIONS[leg].items():
            ctx.set_option(k, v)
        runs = []
        for _ in range(2 if leg == "b" else 1):
            ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
            log = [ctx.ngd_step(0.55, 10) for _ in range(STEPS)]
            runs.append((log, ctx.ngd_get_state()))
    finally:
        ctx.close()
    return runs


@pytest.mark.parametrize("leg", list(LEG_OPTIONS))
@pytest.mark.parametrize("n", RESIDENT_N)
def test_resident_legs_vs_oracle(n, leg):
    ch, ref_log, ref_state = _resident_oracle(n)
    assert all(ok for ok, _, _ in ref_log), ref_log                      # three ACCEPTED steps
    log, state = _resident_run(n, leg)[0]
    for r, (ok, cost, ntr) in zip(log, ref_log):
        assert r["accepted"] == ok and r["ntrials"] == ntr
        assert np.isclose(r["new_cost"], cost, rtol=1e-9), (r["new_cost"], cost)
    errs = {k: rel(state[k], ref_state[k]) for k in ("mu", "D", "U", "SigD")}
    print(f"    n {n} leg {leg}: trials {[r['ntrials'] for r in log]}, state against the oracle " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL / 10, errs


@pytest.mark.parametrize("leg", ["b", "c"])
@pytest.mark.parametrize("n", RESIDENT_N)
def test_resident_symmetric_root_legs_match_the_cholesky_route(n, leg):
    (la, sa), (lb, sb) = _resident_run(n, "a")[0], _resident_run(n, leg)[0]
    for a, b in zip(la, lb):
        assert a["accepted"] == b["accepted"] and a["ntrials"] == b["ntrials"]
        assert abs(a["new_cost"] - b["new_cost"]) < 1e-11 * abs(a["new_cost"]), (a["new_cost"], b["new_cost"])
    print(f"    n {n} leg {leg} against the Cholesky route: " + " ".join(f"{k} {rel(sb[k], sa[k]):.1e}" for k in ("mu", "D", "SigD")) +
          f"; bits equal: {all(np.array_equal(sa[k], sb[k]) for k in sa)}")


@pytest.mark.parametrize("n", RESIDENT_N)
def test_resident_warm_started_leg_repeats_bit_for_bit(n):
    (l1, s1), (l2, s2) = _resident_run(n, "b")
    assert l1 == l2
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)


# ---- the JKO map at operator level ----
@functools.lru_cache(maxsize=None)
def _jko_run(kind, d, cls):
    case = sp.jko_case(kind, d, cls)
    ctx = api.Context(0)
    try:
        ctx.chain_set(case["T"], case["n"])
        ctx.factors_add(d, 3, np.zeros(1, dtype=np.int32), KIND[kind], case["params"], np.array([3.7]))
        ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
        ctx.ngd_init(case["mu0"], case["D"], case["U"])
        out = {}
        for h in sp.H_ALL:
            pair = []
            for _ in range(2):
                ctx.prox_gradients(h)
                pair.append(ctx.ngd_get_gradients())
            out[h] = pair
    finally:
        ctx.close()
    return out


def _blocks(V, n, T):
    """(VD [T, n, n], VU [T - 1, n, n]) of the factor's dense Vddmu"""
    VD = np.stack([V[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    return VD, (np.stack([V[:n, n:]]) if T == 2 else np.zeros((0, n, n)))


@pytest.mark.parametrize("kind,d,cls", JKO_CASES, ids=[f"{k}-d{d}-{c}" for k, d, c in JKO_CASES])
def test_jko_map(kind, d, cls):
    case = sp.jko_case(kind, d, cls)
    n, T = case["n"], case["T"]
    R = _jko_run(kind, d, cls)
    problems = []
    for h in sp.H_ALL:
        first, second = R[h]
        ref = sp.jko_oracle(case, h)
        VD, VU = _blocks(ref["V"], n, T)
        eg, eD = rel(first["g"], ref["g"]), rel(first["VD"], VD)
        eU = rel(first["VU"], VU) if T == 2 else 0.0
        print(f"    h {h:g}: g {eg:.2e} VD {eD:.2e} VU {eU:.2e}")
        problems.append(_row(("jko", kind, d, cls, h), max(eD, eU), 1e-8))
        problems.append(None if eg < TIGHT else ("g", h, eg))
        sym = all(np.array_equal(first["VD"][t], first["VD"][t].T) for t in range(T))
        problems.append(None if sym else ("a diagonal block is not symmetric to the last bit", h))
        same = all(np.array_equal(first[k], second[k]) for k in ("g", "VD", "VU"))
        problems.append(None if same else ("a second call gives other bits", h))
    _none(problems)


@pytest.mark.parametrize("n", [9, 16])
def test_prox_step_wide(n):
    """d = 18 and d = 32 binary factors (EPLP = 16 inside the JKO map) with a unary set beside them"""
    ch = _graph(2, n, 8100 + n)
    chain = o.ChainProx(2, n, _oracle_sets(ch), ch["mu0"], ch["D0"], ch["U0"], step_size_base=0.55)
    ctx = api.Context(0)
    try:
        ctx.chain_set(2, n)
        _add_sets(ctx, ch)
        ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        r = ctx.prox_step(0.55, 10)
        st = ctx.ngd_get_state()
    finally:
        ctx.close()
    ok, cost, ntr = chain.step()
    print(f"    n {n}: decreased {ok}, trials {ntr}, cost {cost!r} / {r['new_cost']!r}, mu {rel(st['mu'], chain.mu):.1e} D {rel(st['D'], chain.D):.1e}")
    assert r["decreased"] == ok and r["ntrials"] == ntr
    assert np.isclose(r["new_cost"], cost, rtol=1e-9)
    assert rel(st["mu"], chain.mu) < RTOL / 10 and rel(st["D"], chain.D) < RTOL / 10


# ---- the rule is a property of the context ----
ORDERS = ("sets-rule", "rule-sets", "rule-chain_set-sets")


@functools.lru_cache(maxsize=None)
def _contract_run(n, order):
    ch = _graph(3, n, 9100 + n, temp=3.7)
    X = np.random.default_rng(n).normal(size=(3, 3, n))
    ctx = api.Context(0)
    try:
        ctx.chain_set(3, n)
        if order == "sets-rule":
            ids = _add_sets(ctx, ch)
            ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
        else:
            ctx.ngd_set_update_rule(api.RULE_PROX_JKO)
            if order == "rule-chain_set-sets":
                ctx.chain_set(3, n)
            ids = _add_sets(ctx, ch)
        out = {}
        for rule in ("prox", "ngd"):
            if rule == "ngd":
                ctx.ngd_set_update_rule(api.RULE_NGD)
            ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
            if rule == "prox":
                ctx.prox_gradients(0.55)
            else:
                ctx.ngd_gradients()
            gr = ctx.ngd_get_gradients()
            out[rule] = dict(g=gr["g"], VD=gr["VD"], VU=gr["VU"], costs=[ctx.ngd_factor_costs(s) for s in ids],
                             sample=[ctx.sample_factor_costs(s, X) for s in ids])
    finally:
        ctx.close()
    return ch, X, out


@functools.lru_cache(maxsize=None)
def _contract_oracle(n):
    ch, X, _ = _contract_run(n, ORDERS[0])
    out = {}
    for rule, temp in (("prox", 1.0), ("ngd", 3.7)):
        sets = _oracle_sets(ch, temp)
        if rule == "prox":
            chain = o.ChainProx(3, n, sets, ch["mu0"], ch["D0"], ch["U0"])
            g, VD, VU = chain.gradients(0.55)
            costs = chain.factor_costs(chain.mu, chain.SigD, chain.SigU)
        else:
            chain = o.ChainNGD(3, n, sets, ch["mu0"], ch["D0"], ch["U0"])
            g, VD, VU = chain.gradients()[3]
            costs = [fs.moments(*o.gather_marginals(chain.mu, chain.SigD, chain.SigU, fs.start, fs.d))["cost"] for fs in sets]
        sample = []
        for fs in sets:                                                  # psi_k(x[start_k n : start_k n + d]) / temperature_k
            Xk = np.stack([X.reshape(len(X), -1)[:, s * n:s * n + fs.d] for s in fs.start])         # [K, S, d]
            sample.append(fs.psi_batch(Xk).T / temp)
        out[rule] = dict(g=g, VD=VD, VU=VU, costs=costs, sample=sample)
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", [2, 6])
def test_rule_is_a_property_of_the_context(n, order):
    got, ref, first = _contract_run(n, order)[2], _contract_oracle(n), _contract_run(n, ORDERS[0])[2]
    for rule in ("prox", "ngd"):
        G, Rf = got[rule], ref[rule]
        errs = dict(g=rel(G["g"], Rf["g"]), VD=rel(G["VD"], Rf["VD"]), VU=rel(G["VU"], Rf["VU"]),
                    costs=max(rel(a, b) for a, b in zip(G["costs"], Rf["costs"])),
                    sample=max(rel(a, b) for a, b in zip(G["sample"], Rf["sample"])))
        print(f"    n {n} {order} under {rule}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert errs["g"] < TIGHT and errs["VD"] < 1e-8 and errs["VU"] < 1e-8 and errs["costs"] < TIGHT and errs["sample"] < TIGHT, (rule, errs)
        for k in ("g", "VD", "VU"):
            assert np.array_equal(G[k], first[rule][k]), (rule, k)
        for k in ("costs", "sample"):
            assert all(np.array_equal(a, b) for a, b in zip(G[k], first[rule][k])), (rule, k)
    assert not np.allclose(ref["prox"]["costs"][0], ref["ngd"]["costs"][0], rtol=0.5)       # (3.7 is visible in the reference)
