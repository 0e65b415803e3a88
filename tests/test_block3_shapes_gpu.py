"""factor_block3_kernel (the factor stage of the planning graph in one launch, kernels_block.hpp) against float64 references,
at the chunk counts, set sizes and starts its hand-made bookkeeping depends on and no graph of the suite reaches (-m gpu).

A workgroup of the kernel owns G = 4 / nch consecutive factors of one set, nch = block3_nch(nchunk) (3 chunks run as 4 with an
idle wave), wave w takes chunk w % nch of factor w / nch, arrivals at the tail are numbered k, K0 + k, K0 + K1 + k, start[k] is
read for every set, the workgroups behind the sets' write the chain-level trial mean, and a set with more than four chunks
sends the whole pass to the three launches.  The two graphs of the suite that reach the kernel (planar, planar1k) have the
chunk triples (priors, obstacle, anchors) = (1, 1, 1) and (1, 2, 1), start = arange, two anchors at the ends, K0 = T - 1,
K1 = T and one temperature per set.  The rows here (ROWS: T, GH degrees, target_waves, starts, registration order, expected
chunk triple) are small n = 4 planning graphs built directly: QUAD_PRIOR d = 8 with the minimum-acceleration Phi, Q^-1
(dt = 1) perturbed per factor (Phi + 0.05 N, Q^-1 + 0.3 G G^T / n); HINGE_SDF_2D d = 4 on make_planar_chain's field with sigma
and eps varied within +-30 % per factor, the states along y = 0.3 under the upper disc so that the hinge is active (asserted on
the CPU: at least half of the obstacle factors have a non-zero oracle Vddmu; it is 0.8 to 1.0); FIXED_PRIOR d = 4 anchors with
Kinv = G G^T / n + 1.5 I; EVERY FACTOR ITS OWN TEMPERATURE from [0.5, 2].  The states' precision is 8 x that of the fused
module's _state: with the weaker one the hinge's negative curvature makes the first trial precision indefinite on half of the
rows and the trial cost a NaN on both sides.  Chunking is steered by the GH degrees and target_waves (plan_chunks: nch =
min(max(1, ceil(target_waves / K)), Np / 256), nchunk = ceil(iters / ceil(iters / nch))) and read back with profile_geometry; a
row that misses its triple fails.  Between them the one-launch rows have (test_the_rows_between_them_reach_every_path):
    A (4, 4, 1)   B (1, 3, 1): the idle wave   C (3, 2, 4)   D (2, 2, 3)   E, H (1, 1, 1)   F (1, 2, 1)   G (1, 1, 2)
every set at 1, 2, 3 and 4 chunks; for every set an odd K at two chunks and K % 4 = 1, 2 and 3 at one chunk (idle factor slots
in the set's last workgroup); obstacle factors on a subset of the states with several on one (B, F, G, H), priors with gaps
(E: the d = 8 gather with s != k), three anchors away from the ends (B, G), one anchor only (E), K1 > K0 + 1 (D), K1 < K0 (E),
and T = 70 (H: nmu = 280, two trial-mean workgroups, the second partly filled; 175 arrivals in three groups of the tail's
two-level count, every other row has one group).

References.  (1) The oracle (gvi_oracle.FactorSet / ChainNGD with the closures of tests/chains.py) on every row.  (2) For the two
quadratic sets the closed form of test_fused_pass_shapes_gpu (imported: Vddmu_k = H_k / T_k, Vdmu_k = grad psi_k(mu_k) / T_k,
cost_k = (psi_k(mu_k) + tr(H_k Sigma_k) / 2) / T_k, marginals of the dense inverse), to which the hinge set's part is added by
the oracle's quadrature -- the hinge has no closed form.  The hinge set therefore also has an operator-level check
(test_hinge_moments_of_the_obstacle_set_alone_vs_oracle: gvi_moments / gvi_costs of the obstacle set alone at the marginals the
oracle computes).  Bounds: TIGHT = 1e-9 for g, per-factor costs, dmu, mu and the total cost; V_D, V_U and the
trial D / U / SigD / SigU 1e-9 at degree 3 and 1e-8 at degree >= 5.  Conditions, checked on the CPU at the top of every test
of a row (_check_conditions, on the cached references): the references agree 5x inside the bound, cond(V) of the oracle's
assembled V is <= 1e3 (the hinge makes V indefinite on every row; near-singular it must not be), every compared accept
decision has its cost difference >= 1e-6 relative from zero.  Per row, state B: cond(V) of the oracle's assembled V; the two
REFERENCES AGAINST EACH OTHER on the CPU (ref V: the worst of V_D, V_U and the trial's D, U, SigD, SigU; ref tight: the worst
of g, per-factor costs, dmu, trial mu, trial cost, cost of B); the relative distance of the accept decision's cost difference
from zero (margin; every row accepts its first trial at base 0.55); and the DEVICE AGAINST THE REFERENCES, measured, the worse
of the two references over every leg the row runs (dev V, dev tight: the same groups, with S3's cost_iter and new_cost in
tight):
    row  cond(V)   ref V    ref tight  margin  dev V    dev tight
    A    111       1.2e-12  3.4e-12    0.35    1.0e-12  3.6e-12 (dmu)
    B    193       1.5e-13  4.6e-12    0.28    2.5e-13  2.9e-12 (dmu)
    C    89        5.7e-12  5.1e-11    0.29    8.0e-12  8.3e-11 (dmu)
    D    156       1.1e-12  2.2e-11    0.40    1.4e-12  3.4e-11 (dmu)
    E    singular  6.5e-14  1.6e-14    --      6.3e-14  1.3e-14 (costs)
    F    153       2.2e-13  1.8e-12    0.32    2.4e-13  1.5e-12 (dmu)
    G    165       1.6e-12  3.5e-13    0.34    1.1e-12  9.6e-13 (dmu)
    H    404       2.0e-13  4.5e-12    0.27    1.6e-13  5.9e-12 (dmu)
    X    49        3.3e-13  4.2e-12    0.31    1.9e-13  2.2e-12 (dmu)
    Y    87        1.2e-13  6.2e-13    0.29    6.6e-14  4.2e-13 (dmu)
Rows C, G and H took another seed (SEEDS): the default's cond(V) was 231 with the references 5.9e-10 apart in dmu (C), 4370 (G)
and 1035 (H).  Row E is singular by construction (priors with gaps; states 4 and 7 carry an obstacle factor only, which says
nothing about the velocities): it compares g, V_D, V_U, the per-factor costs and the trial D / U / SigD / SigU, and neither dmu,
mu, the total cost nor the accept decision.
The obstacle set alone, worst row: E[psi] 3.6e-14, Vdmu 7.1e-14, Vddmu 2.7e-13, cost 3.1e-14.  One obstacle factor of rows G,
H and Y has all its sigma points outside the hinge: its cost is 0 exactly in both references, so it has no relative error and
is held absolutely, relative to the set's largest cost (_cost_err).  The whole module takes 4 s on the device.

Sequences, per row in ONE context, on state A first and then (ngd_init) on state B, B checked against B's references and g_B
far from g_A at every node, the launch counter (api.block3_launches) read round B's sequence:
  S1  ngd_gradients, ngd_get_gradients, ngd_factor_costs of every set (the costs pass reuses the products and the mu_k / Sigma_k
      the one launch left in memory); again under fuse_gather 0 (the kernel's entry without the gather): equal bits;
  S2  ngd_gradients, ngd_trial, ngd_get_gradients, ngd_accept under ngd_set_mode(1, 1) -- gather with gdmu, the trial-mean
      workgroups, tail on -- and (1, 0);
  S3  one ngd_step(0.55, 10): accepted, ntrials, cost_iter and new_cost against the oracle;
  S4  rows A, B, C, D: ngd_run(5) + ngd_run(1) + ngd_run(6) against the same ngd_step sequence, bit for bit, pipeline 1 and 0,
      bases 0.55 and 3.5 -- at 3.5 every iteration backtracks (asserted on the device's log and on the oracle's first step;
      the oracle needs 4 to 10 trials per iteration there): the queued-ahead pass of a rejected iteration leaves through
      pred_skip.  (At temperatures near 1 the hinge ends rows A and B after one accepted iteration at base 0.55, as it does
      planar; C and D accept nine.)
The counter moves in every one of S1 - S3 on the one-launch rows, else every row could pass on the three launches, and on no
classifier row: X (nine chunks per obstacle factor), Y (anchors registered before the obstacle set), row A under fused 0,
pair_fuse 0, set_variant 2 and chol_sqrt 0 (ngd_block3_full asks for the Cholesky products of the two quadratic sets: with
the symmetric root the pass takes the three launches).  Same references, same bounds.

Legs.  Every one-launch row again under fused 0 (prep_all_kernel -> moments_planar3_kernel -> epilogue_all_kernel): the same
references, and the one-launch run's bits in S1 - S3 on every row and in S4 on its rows -- the one launch captures the sets'
own chunking, so no row is exempt.  Rows B and C (priors at three chunks) also under sreg_pipe 0 / 1, mirror 0 / 1 and
warm_start 0 / 1, to the same references.  sreg_pipe 0 and 1 were measured NOT to give equal bits on these rows: the
hand-pipelined body sums mirror pairs of the table, the compiler-scheduled one single points; both hold the bounds.  Two things
these legs cannot observe, so the module asserts neither: whether the kernel's pipe flag was 1 (it is sreg_pipe && the d = 8
table has its tile-major copy, which upload_table makes for every d <= 12 at every degree; no entry point reports it), and
whether a pass was warm-started (warm_count % 32 != 0 holds from a context's second pass on, and state B's passes follow state
A's in the same context; no entry point reports it either).

Mutations of kernels_block.hpp, each tried once on a library built with that one line changed (GVI_LIB_PATH), this module beside
the existing planar tests (test_planar_obstacle_chain_vs_oracle, test_planning_graph_one_launch_factor_stage_is_bit_identical_
to_three_launches[planar, planar1k], test_ngd_reinit_on_a_perturbed_state_vs_oracle[planar, planar1k]):
  block_epilogue receives arrival k instead of K0 + k for the obstacle set    row H fails, in the one-launch test and in the
      fused 0 leg: "cost publish did not arrive".  The arrival number only selects the group of the tail's two-level count (64
      arrivals per group); H's 175 arrivals make three groups, 128 arrive in group 0 and the top count never completes.  Rows
      A - G have one group and pass.  Of the planar tests the two on planar1k fail, the three on planar (35 arrivals) pass.
  block3_nch returns nchunk unchanged for 3                                   judged from the code first: wave 3 becomes a
      second lead wave (chunk 0) of factor b + 1, guarded by k < K, so every index stays in bounds and nothing waits on the
      device: no fault, no hang.  Run: rows B, C and D (the rows with a set at three chunks) fail in every test they are in
      (one launch: g off by 0.1 to 0.8; fused 0 leg; all twelve option legs; S4 of B, C, D); A, E - H pass.  All planar tests
      pass (no set at three chunks).
  block_products gathers with s = k                                           every one-launch row fails: A - D, F, G, H in the
      one-launch test, all eight in the fused 0 leg's bit comparison, all option legs, S4 of A - D.  Row E passes the one-launch
      test -- singular, so the trial mean and cost, where its gather shows, are not compared -- and is caught by the bits of the
      three launches.  All five planar tests fail too (their anchors sit at [0, T - 1]).
  a set's k is computed with 4 / nchunk in place of 4 / nch                   no mutant, not built: nchunk and nch differ only
      at nchunk = 3, and 4 / 3 == 4 / 4 == 1 in integer arithmetic.
  the obstacle set's phase 3 divides by temperature[b]                        rows C, D, E, F, G, H fail (one launch: g off by
      0.04 to 0.7; fused 0 leg; C's option legs; S4 of C, D): the rows with two or four obstacle factors per workgroup.  A and B
      pass, as they must: four waves per obstacle factor, k == b.  All planar tests pass (one temperature per set).
"""
import functools

import numpy as np
import pytest

import gvi_oracle as o
from gaussianvi_amd import api
from gaussianvi_amd import synthetic as syn
from test_asm_dense_vs_reference_gpu import _state
from test_fused_pass_shapes_gpu import (STEP, _bits_equal, _check_sequences, _closed_form_at, _cost_err, _freeze, _hold,
                                         _vtol)
from test_fused_pass_shapes_gpu import _run_sequences as _sequences
from test_gpu_parity import TIGHT, rel

pytestmark = pytest.mark.gpu

N = 4                                                                # [x, y, vx, vy]
DT = 1.0                                                             # time step of the minimum-acceleration prior
SDF_ORIGIN, SDF_CELL = (-5.0, -4.0), 0.1                             # make_planar_chain's field and hinge parameters
SDF_FIELD = syn.circle_sdf(SDF_ORIGIN, SDF_CELL, 81, 101, [(0.0, 1.6), (-1.0, -2.2)], [1.2, 0.9])
SDF_FIELD.setflags(write=False)
PREC = 8.0                                                           # the states' precision: 8 x _state's (marginal sigma ~ 0.18)
HINGE = (15.5, 0.5, 0.3)                                             # (sigma, eps, r)
_r = lambda a, b=None: list(range(a)) if b is None else list(range(a, b))

# name: (T, GH degrees (priors, obstacle, anchors), target_waves or None = default, starts of the priors, of the obstacle
#        factors, of the anchors, registration order, chunks per factor (priors, obstacle, anchors))
ROWS = {
    "A": (6, (4, 6, 3), None, _r(5), _r(6), [0, 5], "bhu", (4, 4, 1)),                  # K = 5, 6, 2
    "B": (7, (3, 7, 3), 21, _r(6), [0, 0, 2, 5, 5, 5, 3], [1, 3, 5], "bhu", (1, 3, 1)),  # the idle wave; K = 6, 7, 3
    "C": (5, (5, 5, 6), 12, _r(4), _r(5), [0, 4], "bhu", (3, 2, 4)),                    # K = 4, 5, 2
    "D": (4, (4, 5, 7), 6, _r(3), [0, 1, 1, 2, 3], [0, 3], "bhu", (2, 2, 3)),           # K = 3, 5, 2: K1 > K0 + 1
    "E": (9, (3, 3, 3), None, [0, 2, 5], [4, 7], [8], "bhu", (1, 1, 1)),                # K = 3, 2, 1: K1 < K0; V singular
    "F": (8, (3, 5, 3), None, _r(7), [1, 1, 3, 4, 6, 6, 7], [0, 7], "bhu", (1, 2, 1)),  # K = 7, 7, 2
    "G": (6, (3, 3, 5), None, _r(5), [0, 1, 3, 3, 5], [1, 2, 4], "bhu", (1, 1, 2)),     # K = 5, 5, 3
    "H": (70, (3, 3, 3), None, _r(69), _r(70) + [33], list(range(0, 70, 2)), "bhu", (1, 1, 1)),   # K = 69, 71, 35; nmu = 280
    # classifier rows: the three launches
    "X": (4, (3, 7, 3), None, _r(3), _r(4), [0, 3], "bhu", (1, 9, 1)),                  # nine chunks per obstacle factor
    "Y": (6, (3, 3, 3), None, _r(5), _r(6), [0, 5], "buh", (1, 1, 1)),                  # anchors registered before the obstacle set
}
ONE_LAUNCH_ROWS = ["A", "B", "C", "D", "E", "F", "G", "H"]
SINGULAR = ("E",)                                                    # priors with gaps, states 4 and 7 without a velocity term
S4_ROWS = {"A": 3.5, "B": 3.5, "C": 3.5, "D": 3.5}                   # second step base of the run-vs-steps sequence
LEG_ROWS = ("B", "C")                                                # sreg_pipe / mirror / warm_start legs (C: priors at 3 chunks)
SEEDS = {"C": 3, "G": 1, "H": 3}                                     # row -> seed offset, where the default missed a condition
SEQS = ("n1", "n1ng", ("n2", 1), ("n2", 0), "n3")


def _mean(T, rng):
    """States along y = 0.3 under the disc of radius 1.2 at (0, 1.6): the signed distance stays below eps + r on most of them"""
    x = np.linspace(-1.6, 1.6, T) + 0.1 * rng.normal(size=T)
    return np.column_stack([x, 0.3 + 0.15 * rng.normal(size=T), 0.5 * rng.normal(size=(T, 2))])


@functools.lru_cache(maxsize=None)
def _problem(row):
    """The factor sets (registration order) and the two states of a row; no two factors share an operand"""
    T, (p0, p1, p2), tw, bs, hs, us, order, _ = ROWS[row]
    rng = np.random.default_rng(4000 + 100 * T + 10 * p0 + p1 + 7 * len(hs) + SEEDS.get(row, 0))
    K0, K1, K2 = len(bs), len(hs), len(us)
    temps = rng.uniform(0.5, 2.0, K0 + K1 + K2)                      # every factor its own temperature
    assert len(np.unique(temps)) == len(temps)
    Phi1, Q1 = syn._minacc(N // 2, syn.QC, DT)
    G = rng.normal(size=(K0, N, N))
    b = dict(kind="b", d=2 * N, p=p0, start=np.asarray(bs, dtype=np.int32), temp=temps[:K0],
             Phi=Phi1[None] + 0.05 * rng.normal(size=(K0, N, N)), Q=Q1[None] + 0.3 * G @ G.transpose(0, 2, 1) / N)
    params = np.asarray(HINGE)[None] * np.column_stack([rng.uniform(0.7, 1.3, K1), rng.uniform(0.7, 1.3, K1), np.ones(K1)])
    h = dict(kind="h", d=N, p=p1, start=np.asarray(hs, dtype=np.int32), temp=temps[K0:K0 + K1], params=params)
    A = (_mean(T, np.random.default_rng(7 * T + 1)),) + tuple(PREC * a for a in _state(T, N, np.random.default_rng(7 * T + N + 1))[1:])
    B = (_mean(T, np.random.default_rng(11 * T + 2)),) + tuple(PREC * a for a in _state(T, N, np.random.default_rng(11 * T + N + 2))[1:])
    G = rng.normal(size=(K2, N, N))
    u = dict(kind="u", d=N, p=p2, start=np.asarray(us, dtype=np.int32), temp=temps[K0 + K1:],
             mu_u=B[0][us] + 0.3 * rng.normal(size=(K2, N)), Kinv=G @ G.transpose(0, 2, 1) / N + 1.5 * np.eye(N))
    by = dict(b=b, h=h, u=u)
    return dict(row=row, T=T, n=N, sets=[by[c] for c in order], A=A, B=B, target_waves=tw)


def _hinge_set(s):
    fs = o.FactorSet(s["start"], s["d"], s["p"], o.psi_batch_hinge_sdf2d(s["params"], SDF_ORIGIN, SDF_CELL, SDF_FIELD))
    fs.temperature = np.asarray(s["temp"], dtype=np.float64)
    return fs


def _oracle_sets(P):
    out = []
    for s in P["sets"]:
        if s["kind"] == "h":
            out.append(_hinge_set(s))
            continue
        psi = o.psi_batch_quad_prior(s["Phi"], s["Q"]) if s["kind"] == "b" else o.psi_batch_fixed_prior(s["mu_u"], s["Kinv"])
        fs = o.FactorSet(s["start"], s["d"], s["p"], psi)
        fs.temperature = np.asarray(s["temp"], dtype=np.float64)
        out.append(fs)
    return out


def _hybrid_at(P, mu, D, U):
    """The priors and the anchors in closed form (no quadrature), the hinge factors by the oracle's quadrature at the
    marginals of the dense inverse"""
    T, n = P["T"], P["n"]
    quad = [s for s in P["sets"] if s["kind"] != "h"]
    cf = _closed_form_at(dict(P, sets=quad), mu, D, U)
    hset = next(s for s in P["sets"] if s["kind"] == "h")
    SigD, SigU = o.dense_to_bt(np.linalg.inv(o.bt_to_dense(D, U)), n)
    r = _hinge_set(hset).moments(*o.gather_marginals(mu, SigD, SigU, hset["start"].astype(np.int64), hset["d"]))
    g, VD, VU = o.bt_assemble(T, n, [(hset["start"].astype(np.int64), r["Vdmu"], r["Vddmu"])])
    qc = iter(cf["costs"])
    costs = [r["cost"] if s["kind"] == "h" else next(qc) for s in P["sets"]]
    return dict(g=cf["g"] + g, VD=cf["VD"] + VD, VU=cf["VU"] + VU, costs=costs, total=cf["total"] + r["cost"].sum())


@functools.lru_cache(maxsize=None)
def _references(row):
    """(closed form + hinge by quadrature, oracle) of state B, computed once per row and shared (read-only) by the tests.
    Both carry g, VD, VU, costs (per set), the trial D / U / SigD / SigU and -- where V is regular -- dmu, the trial mu, the
    trial's total cost and cost0 (state B's); the oracle also its step (accepted, cost, ntrials) and the smallest relative
    distance of a compared cost difference from zero (margin).  cond: of the oracle's assembled V."""
    P = _problem(row)
    T, n = P["T"], P["n"]
    mu, D, U = P["B"]
    regular = row not in SINGULAR
    cf = _hybrid_at(P, mu, D, U)
    cf["cost0"] = cf.pop("total")
    sets = _oracle_sets(P)
    chain = o.ChainNGD(T, n, sets, mu, D, U)
    with np.errstate(all="ignore"):
        dmu, _, _, (g, VD, VU) = chain.gradients()
    ora = dict(g=g, VD=VD, VU=VU)
    marg = [o.gather_marginals(mu, chain.SigD, chain.SigU, fs.start, fs.d) for fs in sets]
    ora["costs"] = [fs.moments(*m)["cost"] for fs, m in zip(sets, marg)]
    hi = [s["kind"] for s in P["sets"]].index("h")
    ora["hinge"] = dict(marg=marg[hi], **{k: v for k, v in sets[hi].moments(*marg[hi]).items() if k in ("E_phi", "Vdmu", "Vddmu", "cost")})
    ora["cond"] = np.linalg.cond(o.bt_to_dense(VD, VU))
    for ref in (cf, ora):
        ref["D"], ref["U"] = D + STEP * (ref["VD"] - D), U + STEP * (ref["VU"] - U)
        ref["SigD"], ref["SigU"] = o.dense_to_bt(np.linalg.inv(o.bt_to_dense(ref["D"], ref["U"])), n)
    if regular:
        V = o.bt_to_dense(cf["VD"], cf["VU"])
        cf["dmu"] = np.linalg.solve(V, -cf["g"].reshape(-1)).reshape(T, n)
        cf["mu"] = mu + STEP * cf["dmu"]
        cf["cost"] = _hybrid_at(P, cf["mu"], cf["D"], cf["U"])["total"]
        ora["dmu"], ora["mu"] = dmu, mu + STEP * dmu
        ora["cost0"] = chain.cost_value(mu, D, U, chain.SigD, chain.SigU)
        ora["cost"] = chain.cost_value(ora["mu"], ora["D"], ora["U"])
        ora["accepted"], ora["new_cost"], ora["ntrials"] = chain.step()
        margins = []
        for t in range(1, ora["ntrials"] + 1):                        # every trial the step compared with cost0
            s = 0.55 * 0.75 ** t
            margins.append(abs(chain.cost_value(mu + s * dmu, D + s * (VD - D), U + s * (VU - U)) / ora["cost0"] - 1.0))
        ora["margin"] = np.nanmin(margins)                           # (NaN: a trial precision that is not positive definite)
    return _freeze(cf), _freeze(ora)


def _refs(row):
    cf, ora = _references(row)
    return [("closed form + hinge", cf), ("oracle", ora)]


def _context(P, options=None, sets=None):
    options = dict(options or {})
    variant = options.pop("set_variant", None)
    ctx = api.Context(0)
    if P["target_waves"] is not None:
        ctx.set_option("target_waves", P["target_waves"])
    for name, value in options.items():
        ctx.set_option(name, value)
    if variant is not None:
        ctx.set_variant(variant)
    ctx.chain_set(P["T"], P["n"])
    for s in (P["sets"] if sets is None else sets):
        K = len(s["start"])
        if s["kind"] == "h":
            sid = ctx.factors_add(s["d"], s["p"], s["start"], api.PSI_HINGE_SDF_2D, s["params"], s["temp"])
            ctx.factors_set_sdf2d(sid, SDF_ORIGIN, SDF_CELL, SDF_FIELD)
            continue
        params = (np.concatenate([s["Phi"].reshape(K, -1), s["Q"].reshape(K, -1)], 1) if s["kind"] == "b" else
                  np.concatenate([s["mu_u"], s["Kinv"].reshape(K, -1)], 1))
        ctx.factors_add(s["d"], s["p"], s["start"], api.PSI_QUAD_PRIOR if s["kind"] == "b" else api.PSI_FIXED_PRIOR, params, s["temp"])
    return ctx


def _counted(fn, *args):
    """fn's result and how many launches of the one-launch factor stage it issued"""
    c0 = api.block3_launches()
    out = fn(*args)
    return out, api.block3_launches() - c0


def _geometry(ctx, P):
    """chunks per factor (priors, obstacle, anchors) of the sets' last launch"""
    by = {s["kind"]: ctx.profile_geometry(sid)["nchunk"] for sid, s in enumerate(P["sets"])}
    return by["b"], by["h"], by["u"]


@functools.lru_cache(maxsize=None)
def _run_sequences(row, options=()):
    """The fused module's S1 - S3 (state A, then state B in the same context) with this module's context, counter and
    geometry.  Cached: the legs compare bits with the plain run."""
    return _sequences(_problem(row), dict(options), context=_context, counted=_counted, geometry=_geometry)


def _check_conditions(row):
    """What the row must satisfy on the CPU before its device numbers mean anything"""
    P = _problem(row)
    cf, ora = _references(row)
    active = (np.abs(ora["hinge"]["Vddmu"]).max(axis=(1, 2)) > 0).mean()
    print(f"    row {row}: obstacle factors with a non-zero Vddmu {active:.2f}")
    assert active >= 0.5
    vkeys, tkeys = ("VD", "VU", "D", "U", "SigD", "SigU"), ["g"]
    _hold("references: V", max(rel(cf[k], ora[k]) for k in vkeys), _vtol(P) / 5)
    worst = [rel(cf["g"], ora["g"])] + [_cost_err(c, cr) for c, cr in zip(cf["costs"], ora["costs"])]
    if row not in SINGULAR:
        worst += [rel(cf["dmu"], ora["dmu"]), rel(cf["mu"], ora["mu"]), abs(cf["cost"] / ora["cost"] - 1.0), abs(cf["cost0"] / ora["cost0"] - 1.0)]
        _hold("cond(V)", ora["cond"], 1e3 * (1 + 1e-12))
        print(f"    accept margin {ora['margin']:.3e}, oracle step {ora['accepted'], ora['ntrials']}")
        assert ora["margin"] >= 1e-6
    _hold("references: tight", max(worst), TIGHT / 5)


def _check_step(tag, row, r3):
    if row in SINGULAR:
        return
    cf, ora = _references(row)
    assert (r3["accepted"], r3["ntrials"]) == (ora["accepted"], ora["ntrials"]), (r3, ora["accepted"], ora["ntrials"])
    _hold(f"{tag} cost_iter vs oracle", abs(r3["cost_iter"] / ora["cost0"] - 1.0), TIGHT)
    _hold(f"{tag} new_cost vs oracle", abs(r3["new_cost"] / ora["new_cost"] - 1.0), TIGHT)
    if ora["ntrials"] == 1:
        _hold(f"{tag} new_cost vs closed form + hinge", abs(r3["new_cost"] / cf["cost"] - 1.0), TIGHT)


def _check_all(tag, row, R):
    _check_sequences(tag, _problem(row), _refs(row), row not in SINGULAR, R, lambda t, r3: _check_step(t, row, r3))


def _check_route(row, R, one_launch):
    print(f"    row {row}: chunks per factor (priors, obstacle, anchors) {R['nchunk_s1']}, launches {[R[t] for t in SEQS]}")
    assert R["nchunk_s1"] == R["nchunk"] == ROWS[row][7], (R["nchunk_s1"], R["nchunk"], ROWS[row][7])
    for tag in SEQS:
        assert (R[tag] >= 1) if one_launch else (R[tag] == 0), (tag, R[tag])


def test_the_rows_between_them_reach_every_path():
    """All six chunk triples; every set at 1, 2, 3 and 4 chunks; at two chunks an odd K and at one chunk K % 4 = 1, 2 and 3
    for each set (idle factor slots in the set's last workgroup); K1 > K0 + 1 and K1 < K0; two trial-mean workgroups, the
    second partly filled.  (The chunking itself is read back from the device in the tests below.)"""
    rows = [ROWS[r] for r in ONE_LAUNCH_ROWS]
    triples = {r[7] for r in rows}
    assert {(4, 4, 1), (1, 3, 1), (3, 2, 4), (2, 2, 3), (1, 1, 1), (1, 2, 1)} <= triples
    for q in range(3):
        assert {t[q] for t in triples} >= {1, 2, 3, 4}, q
        K = lambda r: len(r[3 + q])
        assert any(r[7][q] == 2 and K(r) % 2 == 1 for r in rows), q
        assert {K(r) % 4 for r in rows if r[7][q] == 1} >= {1, 2, 3}, q
    assert any(len(r[4]) > len(r[3]) + 1 for r in rows) and any(len(r[4]) < len(r[3]) for r in rows)
    assert any(256 < r[0] * N < 512 for r in rows)
    assert len(SINGULAR) <= 2 and all(r[0] <= 9 or r[0] == 70 for r in rows)


@pytest.mark.parametrize("row", ONE_LAUNCH_ROWS + ["X", "Y"])
def test_hinge_moments_of_the_obstacle_set_alone_vs_oracle(row):
    """The hinge has no closed form: the obstacle set alone, gvi_moments / gvi_costs at the marginals the oracle computes at
    state B, against the oracle's quadrature with its psi closure."""
    P = _problem(row)
    _check_conditions(row)
    ref = _references(row)[1]["hinge"]
    hset = next(s for s in P["sets"] if s["kind"] == "h")
    ctx = _context(P, sets=[hset])
    try:
        Ephi, Vdmu, Vddmu = ctx.moments(0, *ref["marg"])
        cost = ctx.costs(0, *ref["marg"])
    finally:
        ctx.close()
    _hold("E[psi]", rel(Ephi, ref["E_phi"]), TIGHT)
    _hold("Vdmu", rel(Vdmu, ref["Vdmu"]), TIGHT)
    _hold("Vddmu", rel(Vddmu, ref["Vddmu"]), _vtol(P))
    _hold("cost", rel(cost, ref["cost"]), TIGHT)


@pytest.mark.parametrize("row", ONE_LAUNCH_ROWS)
def test_one_launch_factor_stage_vs_closed_form_and_oracle(row):
    """S1 (with and without the gather), S2 under both trial modes and S3 go through factor_block3_kernel at the row's
    chunk triple, and state B's results agree with the references."""
    _check_conditions(row)
    R = _run_sequences(row)
    _check_route(row, R, True)
    _check_all("one launch", row, R)


@pytest.mark.parametrize("row", ONE_LAUNCH_ROWS)
def test_three_launches_give_the_same_bits_and_hold_to_the_same_references(row):
    """The same sequences under fused 0 (prep_all_kernel -> moments_planar3_kernel -> epilogue_all_kernel): no launch of the
    one-launch stage, the same references, and the one-launch run's numbers bit for bit -- the one launch captures the
    sets' own chunking, so no row is exempt."""
    _check_conditions(row)
    R = _run_sequences(row, (("fused", 0),))
    _check_route(row, R, False)
    _check_all("fused 0", row, R)
    _bits_equal(R, _run_sequences(row), "fused 0", whole_s1=True)


CLASSIFIER = [("X", ()), ("Y", ()), ("A", (("fused", 0),)), ("A", (("pair_fuse", 0),)), ("A", (("set_variant", 2),)),
              ("A", (("chol_sqrt", 0),))]


@pytest.mark.parametrize("row,options", CLASSIFIER, ids=["X", "Y", "A-fused0", "A-pair_fuse0", "A-variant2", "A-chol_sqrt0"])
def test_the_host_classifier_keeps_other_shapes_off_the_one_launch_stage(row, options):
    """Nine chunks per obstacle factor, the anchors registered before the obstacle set, and row A with the one launch or the
    three-set launch switched off, on the LDS-operand register kernels (variant 2) or with symmetric-root products
    (chol_sqrt 0: the kernel is compiled for the Cholesky products of the two quadratic sets): the three launches, the same
    references."""
    _check_conditions(row)
    R = _run_sequences(row, options)
    _check_route(row, R, False)
    _check_all("classifier", row, R)


LEGS = [(r, (leg,)) for r in LEG_ROWS for leg in (("sreg_pipe", 0), ("sreg_pipe", 1), ("mirror", 0), ("mirror", 1),
                                                   ("warm_start", 0), ("warm_start", 1))]


@pytest.mark.parametrize("row,options", LEGS, ids=[f"{r}-{o_[0][0]}{o_[0][1]}" for r, o_ in LEGS])
def test_body_and_product_switches_on_the_one_launch_stage(row, options):
    """sreg_pipe (the priors' phase 2 on the hand-pipelined or on the compiler-scheduled body), mirror and warm_start (state
    B's passes follow state A's in the same context): one launch, the same references.  Neither the kernel's pipe flag nor a
    warm-started pass can be observed from outside (module docstring)."""
    _check_conditions(row)
    R = _run_sequences(row, options)
    _check_route(row, R, True)
    _check_all(str(options), row, R)


def _run_vs_steps(row, fused):
    """(step logs, states) of ngd_run(5) + ngd_run(1) + ngd_run(6) and of the same sequence of ngd_step, per base and pipeline"""
    P = _problem(row)
    ctx = _context(P, dict(fused=fused))
    out = {}
    try:
        for base in (0.55, S4_ROWS[row]):
            ctx.ngd_init(*P["B"])
            ref = []
            for nrun in (5, 1, 6):                                # gvi_ngd_run returns after an iteration that was not accepted
                for _ in range(nrun):
                    ref.append(ctx.ngd_step(base, 10))
                    if not ref[-1]["accepted"]:
                        break
            out[base, "steps"] = (ref, ctx.ngd_get_state())
            print(f"    fused {fused} base {base}: ntrials {[r['ntrials'] for r in ref]}")
            for pipeline in (1, 0):
                ctx.set_option("pipeline", pipeline)
                ctx.ngd_init(*P["B"])
                got, cnt = _counted(lambda: ctx.ngd_run(5, base, 10) + ctx.ngd_run(1, base, 10) + ctx.ngd_run(6, base, 10))
                assert (cnt >= 1) if fused else (cnt == 0), (base, pipeline, cnt)
                out[base, pipeline] = (got, ctx.ngd_get_state())
            ctx.set_option("pipeline", 1)
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("row", list(S4_ROWS))
def test_ngd_run_equals_the_same_sequence_of_steps_on_both_routes(row):
    """S4.  The pipelined run queues the next iteration's one-launch pass behind a device-side accept word; a rejected
    first trial (second base: every iteration backtracks, on the oracle too) turns it into a no-op through pred_skip, and
    the cost-only passes of the backtracking re-plan the sets' chunks between two full passes.  Run and steps agree bit for
    bit, pipeline 1 and 0, and so do the one launch and the three."""
    _check_conditions(row)
    P = _problem(row)
    base = S4_ROWS[row]
    chain = o.ChainNGD(P["T"], P["n"], _oracle_sets(P), *P["B"], step_size_base=base)
    assert chain.step()[2] >= 2                                    # the oracle backtracks at this base
    runs = {fused: _run_vs_steps(row, fused) for fused in (1, 0)}
    for fused, out in runs.items():
        for b in (0.55, base):
            ref, st_ref = out[b, "steps"]
            for pipeline in (1, 0):
                got, st = out[b, pipeline]
                assert got == ref, (fused, b, pipeline)
                assert all(np.array_equal(st[k], st_ref[k]) for k in st_ref), (fused, b, pipeline)
        assert min(r["ntrials"] for r in out[base, "steps"][0]) >= 2   # every iteration backtracked
    for key, (log, st) in runs[1].items():
        log0, st0 = runs[0][key]
        assert log == log0, key
        assert all(np.array_equal(st[k], st0[k]) for k in st0), key
