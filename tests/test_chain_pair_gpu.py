"""The n = 6 chain eliminations in the two-row layout with DPP row-broadcast pivots (option chain_pair, kernels_chain.hpp
eliminate / gj_rowb) against the oracle and, bit for bit, against the v_readlane form (chain_pair 0) (-m gpu).

The row-broadcast form runs the arithmetic of the v_readlane form (fma(-a, f, c) and fma(a, -f, c) are the same bits), so
every result of a factorisation (1/2 log det, tridiagonal blocks of the inverse), of a pivoted solve and of an NGD run must be
the same words under chain_pair 1 and 0.  Every comparison is made on a state B in a context that has just run a state A under
the same setting, into output arrays of their own: nothing compared can be left over from the other run.

References and tolerances are those of test_gpu_parity.test_bt_ops_vs_oracle (the oracle's inverse_gbp / bt_ldlt_pivots /
bt_solve at TIGHT = 1e-9, the log-det at rtol 1e-12) and, for the indefinite chains, of
test_bt_logdet_nan_when_not_pd_and_solve_indefinite (dense numpy solve at 1e-9).

A pass runs the row-broadcast form where one of its levels is crowded (more than eight eliminations per workgroup: chains of 18
or more states); shorter chains run the v_readlane kernels under either setting, and the switch must not matter there either.

Shapes: n = 6 and 5 run the row-broadcast form (N = 6); n = 4 and 8 show that the other block sizes do not depend on the
switch.  T = 2, 3, 5: nodes without a left or right neighbour; 33: one launch, sixteen eliminations at level 0; 34, 35: an odd
count; 48, 49: the last chain that fits the top pass and the first that needs a segmented pass; 70: a last segment with three
eliminations; 97, 1025: several segments (1025: two segmented levels of passes)."""
import functools
import os

import numpy as np
import pytest

import gvi_oracle as o
from chains import make_chain
from gaussianvi_amd import api
from test_gpu_parity import TIGHT, _spd_chain, rel
from test_handover_fresh_gpu import _state_b

pytestmark = pytest.mark.gpu

PAIR_DEFAULT = int(os.environ.get("GVI_CHAIN_PAIR", "1") != "0")      # the switches as a context reads them at creation
DENSE_DEFAULT = int(os.environ.get("GVI_ASM_DENSE", "1") != "0")
LENGTHS = (2, 3, 5, 33, 34, 35, 48, 49, 70, 97, 1025)
SHAPES = [(T, n) for n in (6, 5) for T in LENGTHS] + [(T, n) for n in (4, 8) for T in (3, 33, 49, 97)]


@functools.lru_cache(maxsize=None)
def problem(T, n):
    """States A and B of a shape with B's oracle results: computed once, never written to."""
    rng = np.random.default_rng(1000 * n + T)
    DA, UA = _spd_chain(T, n, rng)
    DB, UB = _spd_chain(T, n, rng)
    rhsA, rhsB = rng.normal(size=(T, n)), rng.normal(size=(T, n))
    eD, eU = o.inverse_gbp(DB, UB)
    hld = o.logdet_half(o.bt_ldlt_pivots(DB, UB))
    x = o.bt_solve(DB, UB, rhsB.reshape(-1))
    out = (DA, UA, rhsA, DB, UB, rhsB, eD, eU, x)
    for a in out:
        a.setflags(write=False)
    return out + (hld,)


def chain_ops(ctx, pair, A, B):
    """All three operations on state A, then on state B; returns B's results and A's marginals."""
    ctx.set_option("chain_pair", pair)
    SDa, _ = ctx.bt_marginals(A[0], A[1])
    ctx.bt_logdet(A[0], A[1])
    ctx.bt_solve(*A)
    SD, SU = ctx.bt_marginals(B[0], B[1])
    return dict(SD=SD, SU=SU, hld=np.array([ctx.bt_logdet(B[0], B[1])]), x=ctx.bt_solve(*B)), SDa


def same_words(r1, r0):
    assert set(r1) == set(r0)
    for k in r1:
        assert r1[k].tobytes() == r0[k].tobytes(), f"{k}: {int((r1[k] != r0[k]).sum())} of {r1[k].size} words differ"


@pytest.mark.parametrize("T,n", SHAPES)
def test_factorisation_and_solve_vs_oracle_and_vs_the_readlane_form(T, n):
    DA, UA, rhsA, DB, UB, rhsB, eD, eU, ex, ehld = problem(T, n)
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        r1, SDa = chain_ops(ctx, 1, (DA, UA, rhsA), (DB, UB, rhsB))
        r0, _ = chain_ops(ctx, 0, (DA, UA, rhsA), (DB, UB, rhsB))
    finally:
        ctx.set_option("chain_pair", PAIR_DEFAULT)
        ctx.close()
    errs = (rel(r1["SD"], eD), rel(r1["SU"], eU) if T > 1 else 0.0, rel(r1["x"].reshape(-1), ex))
    print(f"T {T} n {n}: SigD {errs[0]:.2e} SigU {errs[1]:.2e} x {errs[2]:.2e} half-logdet {r1['hld'][0]!r} (oracle {ehld!r})")
    assert max(errs) < TIGHT
    assert np.isclose(r1["hld"][0], ehld, rtol=1e-12)
    assert not np.array_equal(SDa, r1["SD"])                     # (A and B are different chains)
    same_words(r1, r0)


def _swap_chain(T, n):
    """State B of the shape with the leading diagonal entry of node 3 (eliminated at level 0, between full nodes) at 1e-3 of its
    column maximum: the natural pivot is refused (threshold 1/8) and rows are swapped -- in that node only."""
    DA, UA, rhsA, DB, UB, rhsB = problem(T, n)[:6]
    D = DB.copy()
    D[3, 0, 0] = 1e-3 * np.abs(D[3, 1:, 0]).max()
    return (DA, UA, rhsA), (D, UB, rhsB)


@pytest.mark.parametrize("n", [6, 5])
def test_solve_with_a_forced_row_swap_in_one_node(n):
    T = 35
    A, B = _swap_chain(T, n)
    ref = np.linalg.solve(o.bt_to_dense(B[0], B[1]), B[2].reshape(-1))
    xs = {}
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        for pair in (1, 0):
            ctx.set_option("chain_pair", pair)
            ctx.bt_solve(*A)
            xs[pair] = ctx.bt_solve(*B)
    finally:
        ctx.set_option("chain_pair", PAIR_DEFAULT)
        ctx.close()
    err = rel(xs[1].reshape(-1), ref)
    print(f"n {n}: forced row swap, x against the dense solve {err:.2e}")
    assert err < TIGHT
    assert xs[1].tobytes() == xs[0].tobytes()


@pytest.mark.parametrize("n", [6, 5])
def test_an_indefinite_block_beside_positive_definite_ones(n):
    """Node 3 is indefinite, its level-0 neighbours in the workgroup are not: the log-det is NaN (and nothing else is), the call
    returns, and the pivoted solve of the same chain is still exact."""
    T = 35
    DA, UA, rhsA, DB, UB, rhsB = problem(T, n)[:6]
    D = DB.copy()
    D[3] -= 5.0 * np.eye(n)
    assert np.isnan(o.logdet_half(o.bt_ldlt_pivots(D, UB)))
    ref = np.linalg.solve(o.bt_to_dense(D, UB), rhsB.reshape(-1))
    out = {}
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        for pair in (1, 0):
            ctx.set_option("chain_pair", pair)
            ok = ctx.bt_logdet(DA, UA)
            out[pair] = (ok, ctx.bt_logdet(D, UB), ctx.bt_solve(D, UB, rhsB), ctx.bt_logdet(DB, UB))
    finally:
        ctx.set_option("chain_pair", PAIR_DEFAULT)
        ctx.close()
    for pair in (1, 0):
        ok, bad, x, after = out[pair]
        assert np.isfinite(ok) and np.isnan(bad) and np.isfinite(after), (pair, ok, bad, after)
        assert rel(x.reshape(-1), ref) < 1e-9
    assert out[1][0] == out[0][0] and out[1][3] == out[0][3] and out[1][2].tobytes() == out[0][2].tobytes()


STEPS = 30


def _ngd(ch, seed, options):
    """ngd_init on the chain's own state and one step, then ngd_init on the perturbed state B(seed) and STEPS steps"""
    muB, DB, UB = _state_b(ch, np.random.default_rng(seed))
    ctx, _ = api.context_for_chain(ch)
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        ctx.ngd_step(0.55, 10)
        ctx.ngd_init(muB, DB, UB)
        results = [ctx.ngd_step(0.55, 10) for _ in range(STEPS)]
        state = ctx.ngd_get_state()
    finally:
        ctx.set_option("chain_pair", PAIR_DEFAULT)               # (the context closes next: harmless)
        ctx.set_option("asm_dense", DENSE_DEFAULT)
        ctx.close()
    return results, state


@pytest.mark.parametrize("options", [{}, {"chain_merge": 0}, {"asm_dense": 0}], ids=["default", "chain_merge0", "asm_dense0"])
@pytest.mark.parametrize("name", ["c3mini", "c3"])
def test_ngd_run_does_not_depend_on_the_form(name, options):
    ch = make_chain(name)
    seed = 40 + ch["T"]
    r1, s1 = _ngd(ch, seed, dict(options, chain_pair=1))
    r0, s0 = _ngd(ch, seed, dict(options, chain_pair=0))
    assert all(np.isfinite(s1[k]).all() for k in s1) and any(r["accepted"] for r in r1)
    assert [(x["accepted"], x["ntrials"]) for x in r1] == [(x["accepted"], x["ntrials"]) for x in r0]
    assert [x["new_cost"] for x in r1] == [x["new_cost"] for x in r0]
    assert [x["cost_iter"] for x in r1] == [x["cost_iter"] for x in r0]
    assert set(s1) == set(s0)
    for k in s1:
        assert s1[k].tobytes() == s0[k].tobytes(), k
