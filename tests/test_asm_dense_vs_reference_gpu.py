"""The batched assemble-on-load of the chain's first pass against two float64 references, at the shapes where its hand-made
addresses and predicates can go wrong (-m gpu).

kernels_chain.hpp's dense path (ChainArgs::asm_on == ASM_DENSE) forms V_D, V_U and g from the per-factor results of at most
one binary (d = 2n) and one unary (d = n) factor set: both sets' fields in one batch, every address an offset from one product,
skipped loads redirected to index 0 and selected to 0.0, the solve's g entry fetched ahead (gpre).  tests/test_chain_dense_gpu.py
compares NGD runs between switch settings on chains that all have the binary set first, Kb = T - 1, Ku = T and n = 6 = N; the
chains here are small random quadratic ones (QUAD_PRIOR + FIXED_PRIOR, GH degree 3, temperature 1) that cover what those leave
out: the unary set registered first, one set only, sets shorter than the chain, identity-padded blocks (n = 5, 7, 13), N >= 12
(a second load round per thread), the generic kernels at N = 1, 2 (chain_wave 0), segmented first passes with a partial last
workgroup, and the solve-only launch of ngd_join_solve.

References.  (1) The oracle (gvi_oracle.ChainNGD).  (2) A closed form without any quadrature: psi is quadratic, so V is the sum
of the factor Hessians (2 Kinv_k on block k; J^T Q_k J with J = [Phi_k, -I] on blocks k, k + 1), g the sum of the factor
gradients at the mean, dmu = solve(dense(V), -g).  TIGHT = 1e-9 is what the project holds operator-level results to; the two
references differ from each other by at most 5.3e-12 (V), 1.2e-13 (g) and 1.1e-10 (dmu, on the T = 75, n = 5 row, whose V has
condition 1.3e3; 8e-12 on the rows of condition <= 10) on these chains, so the references alone sit 9x inside the bound.

Sequences, per case in ONE context, on state A first and then (ngd_init) on state B, B checked against B's references and
g_B far from g_A at every node, so nothing B reads can be left over from A:
  S1  ngd_gradients, ngd_get_gradients                         -- the solve-only launch with the assemble pending;
  S2  ngd_gradients, ngd_trial, ngd_get_gradients, ngd_accept  -- the dual launch (trial factorisation || gradient solve);
  S3  one ngd_step.
Which load path a launch took is read from api.asm_launches(): every row must count as dense in the all-switches-on leg and
as generic under asm_dense 0, else the whole module could pass on the generic loop.

The binary-only row: a chain of relative priors has a null space, V is singular and dmu means nothing; that row compares g,
V_D, V_U, the trial D / U and its SigD / SigU, and neither dmu, mu, the cost nor the accept decision.  (The trial's log-det
reaches the host only inside the cost, which depends on mu: it is not observable on that row.)

What the module sees, tried once on libraries built with one line of the dense path broken (tests/test_chain_dense_gpu.py
passes on the last two):
  the left neighbour's predicate t - 1 < Kb one short (t < Kb)        32 cases here (and the LTV chains of the other module);
  the g pointers of the two sets swapped when the unary set is first  every unary-first row on the generic kernels;
  r < a.n dropped from val (padding rows loaded instead of identity)  the n = 5, 7, 13 rows, through dmu (the stores are guarded).
Two breaks one might try change nothing and cannot be seen by any test: gpre = gs in every round (the g request does not depend
on the round, so every round's sum is the same number), and the two sets' sums added in the other order (x + y = y + x)."""
import functools
import os

import numpy as np
import pytest

import gvi_oracle as o
from asm_closed_form import closed_form
from chains import make_chain
from gaussianvi_amd import api
from test_gpu_parity import TIGHT, rel
from test_handover_fresh_gpu import far_at_every_node

pytestmark = pytest.mark.gpu

DENSE_DEFAULT = int(os.environ.get("GVI_ASM_DENSE", "1") != "0")     # the switches as a context reads them at creation
WAVE_DEFAULT = int(os.environ.get("GVI_CHAIN_WAVE", "1") != "0")
STEP = 0.55 * 0.75                                                   # the first trial of ngd_step(0.55, .)
ALL_ON = dict(asm_dense=1, assemble_on_load=1, chain_merge=1)

# (T, n, layout, Kb, Ku, chain_wave): layout = registration order of the binary (b) and the unary (u) set
CASES = [
    (2, 1, "bu", 1, 2, 1),           # shortest chain on the lane-per-node kernel (it gets asm_on == 2)
    (2, 1, "bu", 1, 2, 0),           # ... and on the generic kernels, N = 1, TOP instance
    (3, 2, "ub", 2, 3, 1),
    (3, 2, "ub", 2, 3, 0),
    (131, 1, "ub", 130, 131, 1),     # generic N = 1, segmented first pass (cap 128), last workgroup partial
    (131, 2, "bu", 130, 131, 1),     # generic N = 2, same
    (9, 3, "ub", 8, 9, 1),           # unary-first sums
    (70, 3, "bu", 40, 70, 1),        # short binary set: V_U[t] = 0 for t >= 40, V_D[41..] unary only; cap 64: segmented
    (9, 4, "u", 0, 9, 1),            # single unary set
    (9, 4, "b", 8, 0, 1),            # single binary set: V singular (module docstring)
    (75, 5, "ub", 74, 60, 1),        # padded block (N = 6), short unary set, 3 workgroups, merged top + backward launch
    (49, 6, "bu", 48, 49, 1),        # first T above the one-launch cap of N = 6
    (33, 6, "ub", 20, 33, 1),        # TOP instance, short binary set
    (27, 7, "bu", 26, 27, 1),        # padded (N = 8), segmented (cap 24, S = 16)
    (25, 8, "ub", 24, 25, 1),
    (11, 12, "bu", 10, 11, 1),       # two load rounds per thread, S = 8, partial last segment
    (9, 12, "ub", 8, 5, 1),          # two rounds + short unary set
    (10, 13, "ub", 9, 10, 1),        # padded N = 16, d = 26
    (11, 16, "bu", 10, 11, 1),       # N = 16, d = 32 (the factor kernels' limit)
]
IDS = [f"T{T}-n{n}-{lay}-Kb{Kb}-Ku{Ku}-wave{w}" for T, n, lay, Kb, Ku, w in CASES]


def _state(T, n, rng):
    s = rng.uniform(0.8, 1.25, T)
    D = (4.0 * s * s)[:, None, None] * np.eye(n)[None]
    U = (-0.5 * s[:-1] * s[1:])[:, None, None] * np.eye(n)[None] + 0.05 * rng.normal(size=(T - 1, n, n))
    return rng.normal(size=(T, n)), D, U


@functools.lru_cache(maxsize=None)
def _problem(T, n, layout, Kb, Ku):
    """The factor sets and the two states of a case (chain_wave does not enter)"""
    rng = np.random.default_rng(1000 * T + 10 * n + Kb + 3 * Ku + len(layout))
    P = dict(T=T, n=n, layout=layout, Kb=Kb, Ku=Ku)
    if Kb:
        G = rng.normal(size=(Kb, n, n))
        P["Phi"] = np.eye(n)[None] + 0.05 * rng.normal(size=(Kb, n, n))
        P["Q"] = G @ G.transpose(0, 2, 1) / n + 2.0 * np.eye(n)
    if Ku:
        G = rng.normal(size=(Ku, n, n))
        P["mu_u"] = rng.normal(size=(Ku, n))
        P["Kinv"] = G @ G.transpose(0, 2, 1) / n + 1.5 * np.eye(n)
    P["A"] = _state(T, n, np.random.default_rng(7 * T + n + 1))
    P["B"] = _state(T, n, np.random.default_rng(11 * T + n + 2))
    return P


def _closed_form(P, mu):
    """g, V_D, V_U as the sums of the factor gradients at the mean and of the factor Hessians; the binary set's share of
    V_D; dmu from the dense system (None where V is singular: no unary set)"""
    T, n = P["T"], P["n"]
    sets = []                                                     # (binary set first: the order these sums always had)
    if P["Kb"]:
        sets.append(dict(kind="b", start=np.arange(P["Kb"]), Phi=P["Phi"], Q=P["Q"]))
    if P["Ku"]:
        sets.append(dict(kind="u", start=np.arange(P["Ku"]), mu_u=P["mu_u"], Kinv=P["Kinv"]))
    cf = closed_form(T, n, sets, mu, solve=bool(P["Ku"]))
    return dict(g=cf["g"], VD=cf["VD"], VU=cf["VU"], VDb=cf["parts"][0] if P["Kb"] else np.zeros((T, n, n)), dmu=cf["dmu"])


def _oracle_sets(P):
    n = P["n"]
    by = {"b": lambda: o.FactorSet(np.arange(P["Kb"]), 2 * n, 3, o.psi_batch_quad_prior(P["Phi"], P["Q"])),
          "u": lambda: o.FactorSet(np.arange(P["Ku"]), n, 3, o.psi_batch_fixed_prior(P["mu_u"], P["Kinv"]))}
    return [by[c]() for c in P["layout"]]


@functools.lru_cache(maxsize=None)
def _references(T, n, layout, Kb, Ku):
    """Both references of state B, computed once per case and shared (read-only) by the tests"""
    P = _problem(T, n, layout, Kb, Ku)
    mu, D, U = P["B"]
    cf = _closed_form(P, mu)
    chain = o.ChainNGD(T, n, _oracle_sets(P), mu, D, U)
    dmu, _, _, (g, VD, VU) = chain.gradients()
    ora = dict(g=g, VD=VD, VU=VU, dmu=dmu)
    ora["D"], ora["U"] = D + STEP * (VD - D), U + STEP * (VU - U)
    ora["SigD"], ora["SigU"] = o.inverse_gbp(ora["D"], ora["U"])
    if Ku:                                                        # (V singular otherwise: no meaningful step)
        ora["accepted"], ora["cost"], ora["ntrials"] = chain.step()
    for d in (cf, ora):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cf, ora


def _context(P, wave, options):
    T, n = P["T"], P["n"]
    ctx = api.Context(0)
    ctx.set_option("chain_wave", wave)
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.chain_set(T, n)
    for c in P["layout"]:
        if c == "b":
            K = P["Kb"]
            ctx.factors_add(2 * n, 3, np.arange(K, dtype=np.int32), api.PSI_QUAD_PRIOR,
                            np.concatenate([P["Phi"].reshape(K, -1), P["Q"].reshape(K, -1)], 1))
        else:
            K = P["Ku"]
            ctx.factors_add(n, 3, np.arange(K, dtype=np.int32), api.PSI_FIXED_PRIOR,
                            np.concatenate([P["mu_u"], P["Kinv"].reshape(K, -1)], 1))
    return ctx


def _restore(ctx):
    ctx.set_option("asm_dense", DENSE_DEFAULT)                    # (the context closes next: harmless)
    ctx.set_option("chain_wave", WAVE_DEFAULT)
    ctx.close()


def _s1(ctx):
    ctx.ngd_gradients()
    return ctx.ngd_get_gradients()


def _s2(ctx):
    ctx.ngd_gradients()
    cost = ctx.ngd_trial(STEP)
    gr = ctx.ngd_get_gradients()
    ctx.ngd_accept()
    return gr, ctx.ngd_get_state(), cost


def _counted(fn, *args):
    """fn's result and how many of its launches with an assemble list were classified (dense, generic)"""
    d0, g0 = api.asm_launches()
    out = fn(*args)
    d1, g1 = api.asm_launches()
    return out, (d1 - d0, g1 - g0)


def _s2_a_then_b(P, wave, options):
    """S2 on state A and then on state B of one fresh context: (gradients, accepted state, trial cost) of B, g of A and
    the launch counts of B's sequence"""
    ctx = _context(P, wave, options)
    try:
        ctx.ngd_init(*P["A"])
        grA, _, _ = _s2(ctx)
        ctx.ngd_init(*P["B"])
        (gr, st, cost), counts = _counted(_s2, ctx)
    finally:
        _restore(ctx)
    return gr, st, cost, grA["g"], counts


def _hold(what, value, bound):
    print(f"    {what}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, (what, value, bound)


def _check_gradients(tag, P, gr, gA):
    """g, V_D, V_U, dmu of state B against both references, the structural zeros, and far from state A's"""
    T, Kb, Ku = P["T"], P["Kb"], P["Ku"]
    cf, ora = _references(P["T"], P["n"], P["layout"], Kb, Ku)
    for rname, ref in (("oracle", ora), ("closed form", cf)):
        for k in ("g", "VD", "VU") if Kb else ("g", "VD"):        # (V_U of a unary-only chain is zero: held exactly below)
            _hold(f"{tag} {k} vs {rname}", rel(gr[k], ref[k]), TIGHT)
        if Ku:
            _hold(f"{tag} dmu vs {rname}", rel(gr["dmu"], ref["dmu"]), TIGHT)
    assert (gr["VU"][Kb:] == 0.0).all()                          # no binary factor couples t, t + 1 for t >= Kb
    if Kb and Ku < T:
        _hold(f"{tag} VD[t >= Ku] vs the closed form's binary part", rel(gr["VD"][Ku:], cf["VDb"][Ku:]), TIGHT)
    assert far_at_every_node(gr["g"], gA, T) > 1e-3


@pytest.mark.parametrize("T,n,layout,Kb,Ku,wave", CASES, ids=IDS)
def test_dense_assemble_on_load_vs_oracle_and_closed_form(T, n, layout, Kb, Ku, wave):
    """S1, S2 and S3 with every switch on: each takes the dense path, and state B's results agree with both references."""
    P = _problem(T, n, layout, Kb, Ku)
    cf, ora = _references(T, n, layout, Kb, Ku)
    muB, DB, UB = P["B"]
    ctx = _context(P, wave, ALL_ON)
    try:
        ctx.ngd_init(*P["A"])
        g1A = _s1(ctx)["g"]
        ctx.ngd_init(*P["B"])
        gr1, n1 = _counted(_s1, ctx)
        ctx.ngd_init(*P["A"])
        g2A = _s2(ctx)[0]["g"]
        ctx.ngd_init(*P["B"])
        (gr2, st, cost), n2 = _counted(_s2, ctx)
        ctx.ngd_init(*P["A"])
        ctx.ngd_step(0.55, 10)
        ctx.ngd_init(*P["B"])
        r3, n3 = _counted(ctx.ngd_step, 0.55, 10)
    finally:
        _restore(ctx)
    for tag, cnt in (("S1", n1), ("S2", n2), ("S3", n3)):
        assert cnt[0] >= 1 and cnt[1] == 0, (tag, cnt)          # classified dense, never generic
    _check_gradients("S1", P, gr1, g1A)
    _check_gradients("S2", P, gr2, g2A)
    for k in ("g", "VD", "VU"):                                   # the same ordered sums of the same per-factor results
        assert np.array_equal(gr1[k], gr2[k]), k
    # the accepted trial: formed from the device's own V by the factorisation's first pass (one fused against two rounded
    # operations: an ulp of the larger operand), then against the oracle's trial
    _hold("D vs D_B + step (V_dev - D_B)", rel(st["D"], DB + STEP * (gr2["VD"] - DB)), 1e-14)
    _hold("U vs U_B + step (V_dev - U_B)", rel(st["U"], UB + STEP * (gr2["VU"] - UB)), 1e-14)
    for k in ("D", "U", "SigD", "SigU"):
        _hold(f"trial {k} vs oracle", rel(st[k], ora[k]), TIGHT)
    if Ku:
        for rname, ref in (("oracle", ora), ("closed form", cf)):
            _hold(f"mu vs mu_B + step dmu ({rname})", rel(st["mu"], muB + STEP * ref["dmu"]), TIGHT)
        assert ora["accepted"] and ora["ntrials"] == 1            # (so S2's trial is the step's)
        assert np.isclose(cost, ora["cost"], rtol=1e-9), (cost, ora["cost"])
        assert r3["accepted"] == ora["accepted"] and r3["ntrials"] == ora["ntrials"], (r3, ora["ntrials"])
        assert np.isclose(r3["new_cost"], ora["cost"], rtol=1e-9), (r3, ora["cost"])


@pytest.mark.parametrize("T,n,layout,Kb,Ku,wave", CASES, ids=IDS)
def test_every_load_path_gives_the_same_bits(T, n, layout, Kb, Ku, wave):
    """S2 under asm_dense 0, assemble_on_load 0 and chain_merge 0, each in a fresh context: gradients and accepted state
    equal the all-on run bit for bit; asm_dense 0 runs the generic loop, assemble_on_load 0 assembles in no chain launch."""
    P = _problem(T, n, layout, Kb, Ku)
    gr0, st0, cost0, gA0, cnt0 = _s2_a_then_b(P, wave, ALL_ON)
    assert cnt0[0] >= 1 and cnt0[1] == 0, cnt0
    _check_gradients("all on", P, gr0, gA0)
    for name in ALL_ON:
        gr, st, cost, _, cnt = _s2_a_then_b(P, wave, {**ALL_ON, name: 0})
        if name == "asm_dense":
            assert cnt[0] == 0 and cnt[1] >= 1, (name, cnt)
        elif name == "assemble_on_load":
            assert cnt == (0, 0), (name, cnt)
        else:
            assert cnt[0] >= 1 and cnt[1] == 0, (name, cnt)
        for k in ("g", "VD", "VU", "dmu"):
            assert np.array_equal(gr[k], gr0[k], equal_nan=True), (name, k)
        assert set(st) == set(st0)
        for k in st:
            assert np.array_equal(st[k], st0[k], equal_nan=True), (name, k)
        assert cost == cost0 or (np.isnan(cost) and np.isnan(cost0)), (name, cost, cost0)


def _three_set_context(second_first):
    """Two binary sets (GH degrees 3 and 4) + one unary set on a chain of 21 states, n = 3.  second_first = 12: the chain of
    test_gpu_parity.test_mixed_factor_sets_general_chain, its binary sets on disjoint ranges; 0: both start at state 0"""
    rng = np.random.default_rng(77)
    T, n = 21, 3
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    for K, first, p in ((12, 0, 3), (8, second_first, 4)):
        Phi = np.eye(n)[None] + 0.05 * rng.normal(size=(K, n, n))
        Qh = rng.normal(size=(K, n, n))
        Q = Qh @ Qh.transpose(0, 2, 1) + 2.0 * np.eye(n)
        ctx.factors_add(2 * n, p, np.arange(first, first + K, dtype=np.int32), api.PSI_QUAD_PRIOR,
                        np.concatenate([Phi.reshape(K, -1), Q.reshape(K, -1)], 1))
    Kinv = np.stack([np.eye(n) * 1.5] * T)
    ctx.factors_add(n, 3, np.arange(T, dtype=np.int32), api.PSI_FIXED_PRIOR,
                    np.concatenate([rng.normal(size=(T, n)), Kinv.reshape(T, -1)], 1))
    return ctx, (rng.normal(size=(T, n)), np.stack([np.eye(n) * 4.0] * T), np.stack([np.eye(n) * -0.5] * (T - 1)))


def test_the_host_classifier_keeps_other_graphs_off_the_dense_path():
    """planar (sparse anchor sets), c3lit (a two-anchor unary set: nsp = 2) and a chain with two binary sets assemble on load
    through the generic loop; c3small takes the dense path.  The three-set chain of test_mixed_factor_sets_general_chain
    never reaches the classifier: its second binary set starts at state 12, which is not the start[k] = k layout the
    assemble-on-load reads without indices, so its assemble stays a launch of its own and neither counter moves."""
    def counts(ctx, state):
        try:
            ctx.set_option("asm_dense", 1)
            ctx.set_option("assemble_on_load", 1)
            ctx.ngd_init(*state)
            r, cnt = _counted(ctx.ngd_step, 0.55, 10)
            assert r["accepted"]
        finally:
            ctx.set_option("asm_dense", DENSE_DEFAULT)
            ctx.close()
        return cnt

    for name in ("planar", "c3lit", "c3small"):
        ch = make_chain(name)
        dense, generic = counts(api.context_for_chain(ch)[0], (ch["mu0"], ch["D0"], ch["U0"]))
        if name == "c3small":
            assert dense >= 1 and generic == 0, (name, dense, generic)
        else:
            assert dense == 0 and generic >= 1, (name, dense, generic)
    dense, generic = counts(*_three_set_context(0))
    assert dense == 0 and generic >= 1, ("two binary sets from state 0", dense, generic)
    assert counts(*_three_set_context(12)) == (0, 0)
