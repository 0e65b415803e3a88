"""factor_fused_kernel (the whole factor pass of the resident iteration in one launch, kernels_fused.hpp) against two float64
references, at the block and set shapes its hand-made item bookkeeping depends on and no chain of the suite reaches (-m gpu).

A block of the kernel owns 1 to 4 items (factors): item b of every set plus b + nblk, b + 2 nblk, ... where the second set is
longer than the grid; min(4 - nitems, nitems) idle waves help in phase 1, idle waves run the cost tail where nitems <= 2 and the
item's own wave does otherwise, start[k] is read only for sets that are not chain-structured, and there are three
instantiations.  Every other chain of the suite has K0 = T - 1 binary and K1 = T unary factors with start[k] = k and temperature
1 (block 0: 3 items, every other block: 2).  The rows here (ROWS: T, n, GH degree, starts; items per block in the comments)
are small random quadratic chains -- QUAD_PRIOR with Phi = I + 0.05 N, Q = G G^T / n + 2 I; FIXED_PRIOR with Kinv = G G^T / n +
1.5 I; EVERY FACTOR ITS OWN TEMPERATURE from [0.5, 2], so that a factor reading another's temperature, cost slot or start shows
-- with 4 items on every block, 3 items on more than one, several unary factors on one state, binary sets with gaps, one set
only, the degree 6 / 7 instantiation <6,6,2,12,6> and the m = 2 one off the standard pattern, plus the project's own c3litmini.

References.  (1) Closed form, no quadrature: psi_k is quadratic with Hessian H_k, so Vddmu_k = H_k / T_k, Vdmu_k = grad psi_k
(mu_k) / T_k, cost_k = (psi_k(mu_k) + tr(H_k Sigma_k) / 2) / T_k with Sigma_k the marginal block of the dense inverse of the
precision; g, V_D, V_U the sums over start, dmu = solve(dense V, -g), total cost = sum cost_k + log det(precision) / 2.  (2) The
oracle (gvi_oracle.FactorSet / ChainNGD) on every row but I, whose (12, 7) table costs 18 s of numpy.  Bounds (DESIGN section
6): TIGHT = 1e-9 for g, dmu, mu and costs; V_D, V_U and the trial D / U / SigD / SigU 1e-9 at degree 3 and 1e-8 at degree >= 5.
The two references against each other on these rows, state B (CPU; V: the worst of V_D, V_U and the trial's D, U, SigD, SigU;
tight: the worst of g, per-factor costs, dmu, trial mu, trial cost), and cond(V):
    row        cond(V)   V        tight             row        cond(V)   V        tight
    A          10        3.8e-11  2.6e-11           J          14        1.2e-14  2.5e-14
    B          40        5.1e-11  7.8e-11           K          76        1.4e-14  3.9e-14
    C          4.2       3.5e-13  4.5e-13           L          singular  5.2e-14  9.3e-15
    D          99        8.9e-11  5.3e-10 (dmu)     O          6.3       1.8e-14  2.7e-14
    E          singular  5.2e-11  2.1e-12           c3litmini  1847      1.0e-11  1.9e-11
    F          9.0       3.4e-11  5.2e-11           M          13        2.9e-13  5.2e-13
    G          7.1       3.5e-11  3.6e-11           N          11        8.9e-13  3.3e-12
    H          9.7       1.1e-10  1.5e-10           P          6.4       1.1e-13  2.2e-13
    I          5.4       (closed form only)
so the references alone sit 90x inside the V bound and, but for row D, 6x inside TIGHT.  Row D (two anchors on a chain of nine
states: the weakest V of the module) leaves them 5.3e-10 apart in dmu, 1.9x inside: the degree-5 quadrature error of V (7e-11)
times cond(V).  The device measured against the references on these rows: g 2.3e-12, per-factor costs 6.8e-12, V_D 1.0e-10,
trial SigU 1.2e-10, dmu 3.9e-10 (row D, closed form; 1.4e-10 against the oracle), trial mu 2.0e-10, trial cost 7.8e-11.
Rows E and L have no unary set: a chain of relative priors has a null space, V is singular; they compare g, V_D, V_U, the
per-factor costs and the trial D / U / SigD / SigU, and neither dmu, mu, the total cost nor the accept decision.

Sequences, per row in ONE context, on state A first and then (ngd_init) on state B, B checked against B's references and g_B
far from g_A at every node, the launch counter read round B's sequence:
  S1  ngd_gradients, ngd_get_gradients, ngd_factor_costs of every set (the costs pass reads the mu_k / Sigma_k the fused
      gather wrote); again under fuse_gather 0 (the kernel's entry without the gather): equal bits;
  S2  ngd_gradients, ngd_trial, ngd_get_gradients, ngd_accept under ngd_set_mode(1, 1) -- the fused pass at the trial point:
      gather with gdmu, the extra mean-writing blocks, tail on -- and (1, 0);
  S3  one ngd_step(0.55, 10); both references accept the first trial on every row (asserted);
  S4  rows A, C, G, I, J: ngd_run(5) + ngd_run(1) + ngd_run(6) against the same ngd_step sequence, bit for bit, pipeline 1 and
      0, bases 0.55 and 3.5 -- at 3.5 every row backtracks (ntrials 2 to 3 in every iteration; no row needed a larger base):
      the queued-ahead pass of a rejected iteration leaves through pred_fail with 3 and 4 items per block.
Which kernel ran is read from api.fused_launches(): on the fused rows the row's instantiation counts >= 1 in every one of
S1 - S3 and the other two do not move, else every row could pass on the three-launch route.  Classifier rows (M: unary set
first, d0 = 6; N: five items per block; P: n = 4; row A under fused 0 and under pair_fuse 0): no counter moves, same references.
Row O (T = 4, n = 2, degree 6) was expected to be one of them ("m = 2 is instantiated to degree 5 only", orbit_supported): it is
not.  That condition is smax <= 4, smax the largest SUPPORT of a grid point, which cannot exceed d = 4: every n = 2 chain takes
<2,4,4,4,2> at every degree, correctly (the instance's SMAX = 4 covers all of its tables).  O stays, as a fused row.

Legs.  Every fused row again under fused 0 (prep -> stacked pair kernel at K0 != K1 -> epilogue) and fused 0 + pair_fuse 0, to
the same references.  kernels_fused.hpp promises the three-launch route's bits "with four chunks per factor": the fused pass
sums four chunks (one per wave), the other route nchunk = min(tiles, ceil(orbit_waves / K), tiles / orbit_min_tiles) per set.
The legs run under orbit_min_tiles 1 and an orbit_waves that gives four where one value can (profile_geometry reads it back),
and bits are asserted only then: rows D, E, F, L and c3litmini.  A, B, G, I, J (K1 >= 2 K0: no orbit_waves gives both sets
four; they get 4 + 2), C (3 + 2), H (4 + 3), K (2 + 2) and O (4 + 2: the tables of d = 2, and of d = 4 at degree 3, have two tiles)
leave it out.

What the module sees, tried once each on libraries built with one line of kernels_fused.hpp broken (selected NGD tests of
test_gpu_parity.py beside it: iterations vs oracle, golden steps, scheduling modes, run vs steps, the literal chain):
  the phase-3 helper wave divides by temperature[b] instead of [k]      no change at all: helper waves exist only on blocks of at
                                                                        most two items, where k == b;
  ... by the FIRST set's temperature[k] for both sets                   rows D, F, H, K, O fail (S3's new_cost, by 2e-2 to 2e-1:
                                                                        that tail runs where the step publishes); the others
                                                                        have no block of <= 2 items with a unary one, or T_k = 1;
                                                                        test_gpu_parity passes (temperature 1 everywhere);
  fused_gather ignores S.start (s = k)                                  rows D, G, K, c3litmini fail, and the bit comparison of
                                                                        the legs on D and c3litmini; test_gpu_parity passes;
  phase 1 forms set 1's products with k = b (no "* nblk" wrap)          A, B, C, F, G, H, I, J, O fail (g off by 1);
                                                                        test_gpu_parity fails too (block 0 of every chain wraps)."""
import functools

import numpy as np
import pytest

import gvi_oracle as o
from chains import make_chain
from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import _state
from test_gpu_parity import TIGHT, rel
from test_handover_fresh_gpu import far_at_every_node

pytestmark = pytest.mark.gpu

STEP = 0.55 * 0.75                                                   # the first trial of ngd_step(0.55, .)
I0, I1, I2 = 0, 1, 2                                                 # <6,4,4,12,6>, <6,6,2,12,6>, <2,4,4,4,2>
_r = lambda a, b=None: list(range(a)) if b is None else list(range(a, b))
_C_UNARY = [int(v) for v in np.random.default_rng(5).permutation([0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4])]

# name: (T, n, p, binary starts, unary starts, registration order, instantiation or None = not fused)
ROWS = {
    "A": (6, 6, 5, [1, 3], _r(6), "bu", I0),                  # items per block 4, 4
    "B": (6, 6, 5, [0, 4], [0, 1, 2, 3, 5], "bu", I0),        # 4, 3
    "C": (5, 6, 3, _r(4), _C_UNARY, "bu", I0),                # 4 on every block, K1 = 3 K0, degree 3
    "D": (9, 6, 5, _r(8), [0, 8], "bu", I0),                  # 2, 2, then 1 x 6; unary start non-null
    "E": (9, 6, 5, _r(8), [], "b", I0),                       # single set; V singular
    "F": (9, 6, 5, _r(8), _r(9), "bu", I0),                   # 3, 2, ...: the standard pattern, with temperatures
    "G": (7, 6, 5, [0, 2, 5], _r(7), "bu", I0),               # 4, 3, 3; binary start non-null: d = 12 gather with s != k
    "H": (4, 6, 6, _r(3), _r(4), "bu", I1),                   # 3, 2, 2
    "I": (3, 6, 7, [0, 1], [0, 1, 2, 0, 2], "bu", I1),        # 4, 3; closed form only
    "J": (6, 2, 5, [1, 3], _r(6), "bu", I2),                  # 4, 4
    "K": (9, 2, 3, _r(8), [0, 8], "bu", I2),
    "L": (9, 2, 5, _r(8), [], "b", I2),                       # single set; V singular
    "O": (4, 2, 6, _r(3), _r(4), "bu", I2),                   # 3, 2, 2 at degree 6 (module docstring: not a classifier row)
    "c3litmini": (17, 6, 5, _r(16), [0, 16], "bu", I0),       # the project's own literal chain (chains.make_chain)
    # classifier rows: the three-launch route
    "M": (5, 6, 3, _r(4), _r(5), "ub", None),                 # unary set first: d0 = 6
    "N": (7, 6, 3, [0, 3], _r(7), "bu", None),                # 5 items per block
    "P": (4, 4, 3, _r(3), _r(4), "bu", None),                 # n = 4: no instantiation
}
FUSED_ROWS = [r for r, v in ROWS.items() if v[6] is not None]
CLASSIFIER_ROWS = [r for r, v in ROWS.items() if v[6] is None]
SINGULAR = ("E", "L")                                                # no unary set: dmu, mu, total cost, accept not compared
NO_ORACLE = ("I",)                                                   # the (12, 7) table costs 18 s of numpy
S4_ROWS = {"A": 3.5, "C": 3.5, "G": 3.5, "I": 3.5, "J": 3.5}         # second step base of the run-vs-steps sequence
MUST_MATCH_BITS = ("E", "F", "L")                                    # rows that can always be steered to four chunks
SEEDS = {}                                                           # row -> seed offset, where the default's cond(V) was too large


@functools.lru_cache(maxsize=None)
def _problem(row):
    """The factor sets (registration order) and the two states of a row"""
    T, n, p, bs, us, layout, _ = ROWS[row]
    if row == "c3litmini":
        ch = make_chain(row)
        sets = []
        for spec, kind in zip(ch["specs"], "bu"):
            s = dict(kind=kind, d=spec["d"], p=spec["p"], start=np.asarray(spec["start"], dtype=np.int32),
                     temp=np.asarray(spec["temperature"], dtype=np.float64))
            if kind == "b":
                s["Phi"], s["Q"] = spec["Phi"], spec["Qinv"]
            else:
                s["mu_u"], s["Kinv"] = spec["mu0"], spec["Kinv"]
            sets.append(s)
        rng = np.random.default_rng(37)
        A = (ch["mu0"] + 0.1 * rng.normal(size=ch["mu0"].shape), 1.3 * ch["D0"], 1.3 * ch["U0"])
        return dict(row=row, T=T, n=n, sets=sets, A=A, B=(ch["mu0"], ch["D0"], ch["U0"]))
    rng = np.random.default_rng(1000 * T + 10 * n + p + 7 * len(bs) + 3 * len(us) + SEEDS.get(row, 0))
    temps = rng.uniform(0.5, 2.0, len(bs) + len(us))                 # every factor its own temperature
    assert len(np.unique(temps)) == len(temps)
    by = {}
    if bs:
        K = len(bs)
        G = rng.normal(size=(K, n, n))
        by["b"] = dict(kind="b", d=2 * n, p=p, start=np.asarray(bs, dtype=np.int32), temp=temps[:K],
                       Phi=np.eye(n)[None] + 0.05 * rng.normal(size=(K, n, n)), Q=G @ G.transpose(0, 2, 1) / n + 2.0 * np.eye(n))
    if us:
        K = len(us)
        G = rng.normal(size=(K, n, n))
        by["u"] = dict(kind="u", d=n, p=p, start=np.asarray(us, dtype=np.int32), temp=temps[len(bs):],
                       mu_u=rng.normal(size=(K, n)), Kinv=G @ G.transpose(0, 2, 1) / n + 1.5 * np.eye(n))
    return dict(row=row, T=T, n=n, sets=[by[c] for c in layout],
                A=_state(T, n, np.random.default_rng(7 * T + n + 1)), B=_state(T, n, np.random.default_rng(11 * T + n + 2)))


def _hessians(s, n):
    if s["kind"] == "b":                                          # psi = (J x)^T Q (J x) / 2, J = [Phi, -I]
        J = np.concatenate([s["Phi"], np.broadcast_to(-np.eye(n), s["Phi"].shape)], axis=2)
        return J.transpose(0, 2, 1) @ s["Q"] @ J
    return 2.0 * s["Kinv"]                                        # psi = (x - mu_k)^T Kinv (x - mu_k)


def _closed_form_at(P, mu, D, U):
    """Without quadrature: psi_k is quadratic with Hessian H_k, so Vddmu_k = H_k / T_k, Vdmu_k = grad psi_k(mu_k) / T_k and
    cost_k = (psi_k(mu_k) + tr(H_k Sigma_k) / 2) / T_k, Sigma_k the marginal block of the dense inverse of the precision"""
    T, n = P["T"], P["n"]
    Lam = o.bt_to_dense(D, U)
    Sig = np.linalg.inv(Lam)
    g, VD, VU, costs = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((T - 1, n, n)), []
    for s in P["sets"]:
        H, d = _hessians(s, n), s["d"]
        c = np.zeros(len(s["start"]))
        for k, st in enumerate(s["start"]):
            x = mu[st:st + d // n].reshape(-1) - (s["mu_u"][k] if s["kind"] == "u" else 0.0)
            gr = H[k] @ x
            c[k] = (0.5 * x @ gr + 0.5 * np.trace(H[k] @ Sig[st * n:st * n + d, st * n:st * n + d])) / s["temp"][k]
            g[st] += gr[:n] / s["temp"][k]
            VD[st] += H[k][:n, :n] / s["temp"][k]
            if d == 2 * n:
                g[st + 1] += gr[n:] / s["temp"][k]
                VD[st + 1] += H[k][n:, n:] / s["temp"][k]
                VU[st] += H[k][:n, n:] / s["temp"][k]
        costs.append(c)
    total = sum(c.sum() for c in costs) + 0.5 * np.linalg.slogdet(Lam)[1]
    return dict(g=g, VD=VD, VU=VU, costs=costs, total=total)


def _oracle_sets(P):
    out = []
    for s in P["sets"]:
        psi = o.psi_batch_quad_prior(s["Phi"], s["Q"]) if s["kind"] == "b" else o.psi_batch_fixed_prior(s["mu_u"], s["Kinv"])
        fs = o.FactorSet(s["start"], s["d"], s["p"], psi)
        fs.temperature = np.asarray(s["temp"], dtype=np.float64)
        out.append(fs)
    return out


def _freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _references(row):
    """(closed form, oracle or None) of state B, computed once per row and shared (read-only) by the tests.  Both carry
    g, VD, VU, costs (per set), the trial D / U / SigD / SigU and -- where V is regular -- dmu, the trial mu, the trial's
    total cost, cost0 (state B's) and whether the first trial is accepted"""
    P = _problem(row)
    T, n = P["T"], P["n"]
    mu, D, U = P["B"]
    regular = row not in SINGULAR
    cf = _closed_form_at(P, mu, D, U)
    cf["cost0"] = cf.pop("total")
    cf["D"], cf["U"] = D + STEP * (cf["VD"] - D), U + STEP * (cf["VU"] - U)
    SigT = np.linalg.inv(o.bt_to_dense(cf["D"], cf["U"]))
    cf["SigD"], cf["SigU"] = o.dense_to_bt(SigT, n)
    if regular:
        V = o.bt_to_dense(cf["VD"], cf["VU"])
        cf["cond"] = np.linalg.cond(V)
        cf["dmu"] = np.linalg.solve(V, -cf["g"].reshape(-1)).reshape(T, n)
        cf["mu"] = mu + STEP * cf["dmu"]
        cf["cost"] = _closed_form_at(P, cf["mu"], cf["D"], cf["U"])["total"]
        cf["accepted"], cf["ntrials"] = bool(cf["cost"] < cf["cost0"]), 1
    ora = None
    if row not in NO_ORACLE:
        sets = _oracle_sets(P)
        chain = o.ChainNGD(T, n, sets, mu, D, U)
        with np.errstate(all="ignore"):
            dmu, _, _, (g, VD, VU) = chain.gradients()
        ora = dict(g=g, VD=VD, VU=VU)
        ora["costs"] = [fs.moments(*o.gather_marginals(mu, chain.SigD, chain.SigU, fs.start, fs.d))["cost"] for fs in sets]
        ora["D"], ora["U"] = D + STEP * (VD - D), U + STEP * (VU - U)
        ora["SigD"], ora["SigU"] = o.inverse_gbp(ora["D"], ora["U"])
        if regular:
            ora["dmu"], ora["mu"] = dmu, mu + STEP * dmu
            ora["accepted"], ora["cost"], ora["ntrials"] = chain.step()
        _freeze(ora)
    return _freeze(cf), ora


def _refs(row):
    cf, ora = _references(row)
    return [("closed form", cf)] + ([("oracle", ora)] if ora is not None else [])


def _context(P, options=None):
    ctx = api.Context(0)
    for name, value in (options or {}).items():
        ctx.set_option(name, value)
    ctx.chain_set(P["T"], P["n"])
    for s in P["sets"]:
        K = len(s["start"])
        params = (np.concatenate([s["Phi"].reshape(K, -1), s["Q"].reshape(K, -1)], 1) if s["kind"] == "b" else
                  np.concatenate([s["mu_u"], s["Kinv"].reshape(K, -1)], 1))
        kind = api.PSI_QUAD_PRIOR if s["kind"] == "b" else api.PSI_FIXED_PRIOR
        ctx.factors_add(s["d"], s["p"], s["start"], kind, params, s["temp"])
    return ctx


def _s1(ctx):
    ctx.ngd_gradients()
    gr = ctx.ngd_get_gradients()
    gr["costs"] = [ctx.ngd_factor_costs(sid) for sid in range(len(ctx.sets))]
    return gr


def _s2(ctx):
    ctx.ngd_gradients()
    cost = ctx.ngd_trial(STEP)
    gr = ctx.ngd_get_gradients()
    ctx.ngd_accept()
    return gr, ctx.ngd_get_state(), cost


def _counted(fn, *args):
    """fn's result and how many launches of the fused pass it issued, per instantiation"""
    c0 = api.fused_launches()
    out = fn(*args)
    c1 = api.fused_launches()
    return out, tuple(b - a for a, b in zip(c0, c1))


def _a_then_b(ctx, P, counted, fn, *args):
    """fn on state A and then on state B of the same context: B's result, the launch counts of B's sequence (counted: a
    module's own counter), A's result"""
    ctx.ngd_init(*P["A"])
    outA = fn(*args)
    ctx.ngd_init(*P["B"])
    out, counts = counted(fn, *args)
    return out, counts, outA


def _geometry(ctx, P):
    return [ctx.profile_geometry(sid)["nchunk"] for sid in range(len(ctx.sets))]


def _run_sequences(P, options=None, context=None, counted=_counted, geometry=_geometry):
    """S1, S1 without the fused gather, S2 with the full pass at the trial point and with the cost pass, S3: everything of
    state B, after the same sequence on state A in the same context.  context, counted, geometry: how a module builds its
    context, counts its kernel's launches and reads the chunking back (after S1: nchunk_s1, at the end: nchunk)"""
    ctx = (context or _context)(P, options)
    R = {}
    try:
        R["s1"], R["n1"], a = _a_then_b(ctx, P, counted, _s1, ctx)
        R["g1A"] = a["g"]
        R["nchunk_s1"] = geometry(ctx, P)
        ctx.set_option("fuse_gather", 0)
        R["s1ng"], R["n1ng"], _ = _a_then_b(ctx, P, counted, _s1, ctx)
        ctx.set_option("fuse_gather", 1)
        for mode in (1, 0):
            ctx.ngd_set_mode(1, mode)
            R["s2", mode], R["n2", mode], a = _a_then_b(ctx, P, counted, _s2, ctx)
            R["g2A", mode] = a[0]["g"]
        ctx.ngd_set_mode(1, 2)
        R["s3"], R["n3"], _ = _a_then_b(ctx, P, counted, ctx.ngd_step, 0.55, 10)
        R["nchunk"] = geometry(ctx, P)
    finally:
        ctx.close()
    return R


def _hold(what, value, bound):
    print(f"    {what}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, (what, value, bound)


def _vtol(P):
    return TIGHT if max(s["p"] for s in P["sets"]) <= 3 else 1e-8      # V at GH degree >= 5


def _cost_err(c, cr):
    """Per-factor relative error of the costs; a factor whose reference cost is 0 exactly (a hinge factor with every sigma point
    outside the hinge) has no relative error: there the absolute one, relative to the set's largest cost"""
    c, cr = np.asarray(c), np.asarray(cr)
    zero = cr == 0.0
    return np.where(zero, np.abs(c) / np.abs(cr).max(), np.abs(c / np.where(zero, 1.0, cr) - 1.0)).max()


def _check_gradients(tag, P, refs, regular, gr, gA):
    """g, V_D, V_U, dmu (and the per-factor costs, where the sequence read them) of state B against the references
    (refs: [(name, reference)]; regular: V is not singular by construction)"""
    for rname, ref in refs:
        _hold(f"{tag} g vs {rname}", rel(gr["g"], ref["g"]), TIGHT)
        _hold(f"{tag} VD vs {rname}", rel(gr["VD"], ref["VD"]), _vtol(P))
        if any(s["kind"] == "b" for s in P["sets"]):
            _hold(f"{tag} VU vs {rname}", rel(gr["VU"], ref["VU"]), _vtol(P))
        if regular:
            _hold(f"{tag} dmu vs {rname}", rel(gr["dmu"], ref["dmu"]), TIGHT)
        if "costs" in gr:
            for sid, (c, cr) in enumerate(zip(gr["costs"], ref["costs"])):
                _hold(f"{tag} costs of set {sid} vs {rname}, per factor", _cost_err(c, cr), TIGHT)
    free = np.ones(P["T"] - 1, dtype=bool)
    for s in P["sets"]:
        if s["kind"] == "b":
            free[s["start"]] = False
    assert (gr["VU"][free] == 0.0).all()                          # no binary factor couples these neighbours
    assert far_at_every_node(gr["g"], gA, P["T"]) > 1e-3


def _check_trial(tag, P, refs, regular, gr, st, cost):
    muB, DB, UB = P["B"]
    # formed from the device's own V by the factorisation's first pass (one fused against two rounded operations)
    _hold(f"{tag} D vs D_B + step (V_dev - D_B)", rel(st["D"], DB + STEP * (gr["VD"] - DB)), 1e-14)
    _hold(f"{tag} U vs U_B + step (V_dev - U_B)", rel(st["U"], UB + STEP * (gr["VU"] - UB)), 1e-14)
    for rname, ref in refs:
        for k in ("D", "U", "SigD", "SigU"):
            _hold(f"{tag} trial {k} vs {rname}", rel(st[k], ref[k]), _vtol(P))
        if regular:
            _hold(f"{tag} mu vs {rname}", rel(st["mu"], ref["mu"]), TIGHT)
            _hold(f"{tag} trial cost vs {rname}", abs(cost / ref["cost"] - 1.0), TIGHT)


def _check_step(tag, row, r3):
    if row in SINGULAR:
        return
    for rname, ref in _refs(row):
        assert ref["accepted"] and ref["ntrials"] == 1, (rname, ref["accepted"], ref["ntrials"])
        assert r3["accepted"] and r3["ntrials"] == 1, r3
        _hold(f"{tag} new_cost vs {rname}", abs(r3["new_cost"] / ref["cost"] - 1.0), TIGHT)


def _check_sequences(tag, P, refs, regular, R, check_step):
    """S1 (and its bits without the gather), S2 under both trial modes and, by check_step(tag, r3), S3"""
    _check_gradients(f"{tag} S1", P, refs, regular, R["s1"], R["g1A"])
    for k in ("g", "VD", "VU", "dmu"):                             # the no-gather entry: same numbers, bit for bit
        assert np.array_equal(R["s1"][k], R["s1ng"][k], equal_nan=True), (tag, "fuse_gather 0", k)
    for c, cng in zip(R["s1"]["costs"], R["s1ng"]["costs"]):
        assert np.array_equal(c, cng), (tag, "fuse_gather 0", "costs")
    for mode in (1, 0):
        gr, st, cost = R["s2", mode]
        _check_gradients(f"{tag} S2 mode (1, {mode})", P, refs, regular, gr, R["g2A", mode])
        _check_trial(f"{tag} S2 mode (1, {mode})", P, refs, regular, gr, st, cost)
    check_step(f"{tag} S3", R["s3"])


def _check_all(tag, row, R):
    _check_sequences(tag, _problem(row), _refs(row), row not in SINGULAR, R, lambda t, r3: _check_step(t, row, r3))


def _bits_equal(R, R0, what, whole_s1=False):
    """whole_s1: S1's per-factor costs and the run without the gather as well (routes that share their chunking)"""
    for s1 in ("s1", "s1ng") if whole_s1 else ("s1",):
        for k in ("g", "VD", "VU", "dmu"):
            assert np.array_equal(R[s1][k], R0[s1][k], equal_nan=True), (what, s1, k)
        for sid, (c, c0) in enumerate(zip(R[s1]["costs"], R0[s1]["costs"]) if whole_s1 else ()):
            assert np.array_equal(c, c0, equal_nan=True), (what, s1, "costs", sid)
    for mode in (1, 0):
        (gr, st, cost), (gr0, st0, cost0) = R["s2", mode], R0["s2", mode]
        for k in ("g", "VD", "VU", "dmu"):
            assert np.array_equal(gr[k], gr0[k], equal_nan=True), (what, mode, k)
        for k in st0:
            assert np.array_equal(st[k], st0[k], equal_nan=True), (what, mode, k)
        assert cost == cost0 or (np.isnan(cost) and np.isnan(cost0)), (what, mode, cost, cost0)
    for k, v in R0["s3"].items():
        assert R["s3"][k] == v or (np.isnan(R["s3"][k]) and np.isnan(v)), (what, "S3", k, R["s3"], R0["s3"])


def _four_chunk_options(P):
    """orbit_waves / orbit_min_tiles under which the three-launch route sums four chunks per factor in every set, where
    such a value exists: nchunk = min(tiles, ceil(orbit_waves / K), tiles / orbit_min_tiles)"""
    lo = max(3 * len(s["start"]) for s in P["sets"]) + 1
    hi = min(4 * len(s["start"]) for s in P["sets"])
    return dict(orbit_min_tiles=1, orbit_waves=hi if lo <= hi else 4 * len(P["sets"][0]["start"]))


@pytest.mark.parametrize("row", FUSED_ROWS)
def test_fused_pass_vs_closed_form_and_oracle(row):
    """S1 (with and without the fused gather), S2 under both trial modes and S3 go through the row's instantiation of the
    fused kernel and no other, and state B's results agree with the references."""
    P = _problem(row)
    R = _run_sequences(P)
    want = ROWS[row][6]
    for tag in ("n1", "n1ng", ("n2", 1), ("n2", 0), "n3"):
        cnt = R[tag]
        assert cnt[want] >= 1 and sum(cnt) == cnt[want], (tag, cnt)
    _check_all("fused", row, R)


@pytest.mark.parametrize("row", FUSED_ROWS)
def test_three_launch_legs_vs_the_same_references(row):
    """The same sequences under fused 0 and under fused 0 + pair_fuse 0 (the stacked pair kernel at K0 != K1, then one launch
    per set): no fused launch, the same references; bit for bit the fused leg's numbers where the leg summed four chunks
    per factor in every set (rows E, F, L must)."""
    P = _problem(row)
    steer = _four_chunk_options(P)
    R0 = _run_sequences(P, steer)
    for leg in (dict(fused=0), dict(fused=0, pair_fuse=0)):
        R = _run_sequences(P, {**steer, **leg})
        for tag in ("n1", "n1ng", ("n2", 1), ("n2", 0), "n3"):
            assert R[tag] == (0, 0, 0), (leg, tag, R[tag])
        _check_all(str(leg), row, R)
        four = all(c == 4 for c in R["nchunk"])
        print(f"    {leg}: chunks per factor {R['nchunk']}")
        if row in MUST_MATCH_BITS:
            assert four, (leg, R["nchunk"])
        if four:
            _bits_equal(R, R0, leg)


@pytest.mark.parametrize("row,options", [(r, {}) for r in CLASSIFIER_ROWS] + [("A", dict(fused=0)), ("A", dict(pair_fuse=0))],
                         ids=CLASSIFIER_ROWS + ["A-fused0", "A-pair_fuse0"])
def test_the_host_classifier_keeps_other_shapes_off_the_fused_pass(row, options):
    """Unary set first, five items per block, m = 2 at degree 6, n = 4, and row A with the fused pass or the pair launch
    switched off: the three-launch route, the same references."""
    R = _run_sequences(_problem(row), options)
    for tag in ("n1", "n1ng", ("n2", 1), ("n2", 0), "n3"):
        assert R[tag] == (0, 0, 0), (tag, R[tag])
    _check_all("classifier", row, R)


@pytest.mark.parametrize("row", list(S4_ROWS))
def test_ngd_run_equals_the_same_sequence_of_steps_at_3_and_4_items(row):
    """The pattern of test_gpu_parity.test_ngd_run_equals_the_same_sequence_of_steps on blocks of 3 and 4 items: the
    pipelined run queues the next iteration's fused pass behind a device-side accept word, and a rejected first trial
    (base 3.5) turns it into a no-op through pred_fail in every item wave."""
    P = _problem(row)
    ctx = _context(P)
    want = ROWS[row][6]
    try:
        for base in (0.55, S4_ROWS[row]):
            ctx.ngd_init(*P["B"])
            ref = []
            for nrun in (5, 1, 6):                                # gvi_ngd_run returns after an iteration that was not accepted
                for _ in range(nrun):
                    ref.append(ctx.ngd_step(base, 10))
                    if not ref[-1]["accepted"]:
                        break
            st_ref = ctx.ngd_get_state()
            print(f"    base {base}: ntrials {[r['ntrials'] for r in ref]}")
            for pipeline in (1, 0):
                ctx.set_option("pipeline", pipeline)
                ctx.ngd_init(*P["B"])
                got, cnt = _counted(lambda: ctx.ngd_run(5, base, 10) + ctx.ngd_run(1, base, 10) + ctx.ngd_run(6, base, 10))
                st = ctx.ngd_get_state()
                assert cnt[want] >= 1 and sum(cnt) == cnt[want], (base, pipeline, cnt)
                assert got == ref, (base, pipeline)
                assert all(np.array_equal(st[k], st_ref[k]) for k in st_ref), (base, pipeline)
            if base > 3.0:
                assert max(r["ntrials"] for r in ref) > 1           # the backtracking path was exercised
    finally:
        ctx.set_option("pipeline", 1)
        ctx.close()
