"""The walk's priority bands change no bit (-m gpu): option walk_prio 1 against 0 in ONE context, on small random quadratic
chains of the kind test_fused_pass_shapes_gpu.py builds (QUAD_PRIOR + FIXED_PRIOR, every factor its own temperature).

A walking wave of factor_fused_kernel sets its priority from the share of its modelled walk cost that is still ahead of it
(walk_prio.hpp).  A priority moves instructions in time and nothing else: every wave owns its accumulators and the order of
the LDS adds inside a wave is the program's, so gradients, per-factor costs, the trial state of a step and a whole ngd_run
must be equal bit for bit.  Rows (all three fused instances; blocks of two, three and four items; all of them far inside one
residency round, so the bands are applied under walk_prio 1):
    T5   T = 5, n = 6, degree 5   <6,4,4,12,6>   items per block 3, 2, 2, 2 (the chain pattern)
    T3   T = 3, n = 6, degree 6   <6,6,2,12,6>   3, 2
    T4   T = 4, n = 2, degree 5   <2,4,4,4,2>    4, 4, 4 (three unary factors per binary one)
    U2   T = 5, n = 6, degree 5   <6,4,4,12,6>   3, 3, 3, 3: the unary set twice as long as the binary one
Legs, in this order: (state A, 1), (state B, 0), (state A, 0), (state B, 1) -- the leg before every leg ran on the OTHER
state, and g of B is far from g of A at every node, so a leg that left a previous leg's values in place cannot pass as equal.
Every leg: ngd_gradients + ngd_get_gradients + ngd_factor_costs of every set, then ngd_step(0.55, 10) and the state behind it;
api.fused_launches() says that the row's instance ran in every leg and no other.  Then ngd_run(5) from state B under the step
bases 0.55 and 3.5 with walk_prio 1 and 0: at 3.5 the iterations backtrack (asserted), so the queued-ahead pass of a rejected
iteration leaves through pred_fail."""
import functools

import numpy as np
import pytest

from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import _state
from test_fused_pass_shapes_gpu import _context, _counted
from test_handover_fresh_gpu import far_at_every_node

pytestmark = pytest.mark.gpu

_r = lambda a: list(range(a))
# name: (T, n, degree, binary starts, unary starts, instance: 0 <6,4,4,12,6>, 1 <6,6,2,12,6>, 2 <2,4,4,4,2>)
ROWS = {
    "T5": (5, 6, 5, _r(4), _r(5), 0),
    "T3": (3, 6, 6, _r(2), _r(3), 1),
    "T4": (4, 2, 5, _r(3), [0, 1, 2, 3, 0, 2, 3, 1, 3], 2),
    "U2": (5, 6, 5, _r(4), [0, 1, 2, 3, 4, 0, 2, 4], 0),
}


@functools.lru_cache(maxsize=None)
def _problem(row):
    T, n, p, bs, us, _ = ROWS[row]
    rng = np.random.default_rng(900 * T + 13 * n + p + len(us))
    temps = rng.uniform(0.5, 2.0, len(bs) + len(us))
    K = len(bs)
    G = rng.normal(size=(K, n, n))
    b = dict(kind="b", d=2 * n, p=p, start=np.asarray(bs, dtype=np.int32), temp=temps[:K],
             Phi=np.eye(n)[None] + 0.05 * rng.normal(size=(K, n, n)), Q=G @ G.transpose(0, 2, 1) / n + 2.0 * np.eye(n))
    K = len(us)
    G = rng.normal(size=(K, n, n))
    u = dict(kind="u", d=n, p=p, start=np.asarray(us, dtype=np.int32), temp=temps[len(bs):],
             mu_u=rng.normal(size=(K, n)), Kinv=G @ G.transpose(0, 2, 1) / n + 1.5 * np.eye(n))
    return dict(row=row, T=T, n=n, sets=[b, u],
                A=_state(T, n, np.random.default_rng(5 * T + n + 3)), B=_state(T, n, np.random.default_rng(9 * T + n + 4)))


def _leg(ctx, state, walk_prio):
    ctx.set_option("walk_prio", walk_prio)
    ctx.ngd_init(*state)
    ctx.ngd_gradients()
    out = dict(ctx.ngd_get_gradients())
    for sid in range(len(ctx.sets)):
        out[f"costs{sid}"] = ctx.ngd_factor_costs(sid)
    out["step"] = ctx.ngd_step(0.55, 10)
    for k, v in ctx.ngd_get_state().items():
        out["state_" + k] = v
    return out


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize("row", list(ROWS))
def test_walk_prio_changes_no_bit(row):
    P = _problem(row)
    want = ROWS[row][5]
    ctx = _context(P)
    try:
        legs = {}
        for state, wp in (("A", 1), ("B", 0), ("A", 0), ("B", 1)):
            legs[state, wp], cnt = _counted(_leg, ctx, P[state], wp)
            assert cnt[want] >= 2 and sum(cnt) == cnt[want], (state, wp, cnt)      # the gradients' pass and the step's trial
            assert np.isfinite(legs[state, wp]["g"]).all() and legs[state, wp]["step"]["accepted"]
        for state in ("A", "B"):
            _same_bits(legs[state, 1], legs[state, 0], state)
        assert far_at_every_node(legs["B", 1]["g"], legs["A", 1]["g"], P["T"]) > 1e-3
        assert far_at_every_node(legs["B", 1]["state_mu"], legs["A", 1]["state_mu"], P["T"]) > 1e-3
        for base in (0.55, 3.5):
            runs = {}
            for wp in (1, 0):
                ctx.set_option("walk_prio", wp)
                ctx.ngd_init(*P["A"])                                 # (the other state first: nothing of the last run is left)
                ctx.ngd_run(2, 0.55, 10)
                ctx.ngd_init(*P["B"])
                res, cnt = _counted(ctx.ngd_run, 5, base, 10)
                assert cnt[want] >= 1 and sum(cnt) == cnt[want], (base, wp, cnt)
                runs[wp] = (res, ctx.ngd_get_state())
            print(f"    {row} base {base}: ntrials {[r['ntrials'] for r in runs[1][0]]}")
            assert runs[1][0] == runs[0][0], (base, runs[1][0], runs[0][0])
            for k, v in runs[0][1].items():
                assert np.array_equal(runs[1][1][k], v), (base, k)
            if base > 3.0:
                assert max(r["ntrials"] for r in runs[1][0]) > 1        # the backtracking path was taken
    finally:
        ctx.close()
