"""The chain eliminations with their lane records (kernels_chain.hpp eliminate<ROWB>, chain_lane_record.hpp) through the public
API, at the chain lengths where another body or another operand source is taken (-m gpu).

In the two-row form (N = 6: n = 5 padded by the identity, n = 6; option chain_pair on and a pass with more than eight
eliminations on some level, i.e. T >= 18) a lane of a one-node elimination reads its role, its column and its offsets from a
record in LDS, and the columns of I, of a missing neighbour's coupling and of the lanes outside the tile are loaded from an
identity and a zero block instead of being selected.  Lengths:
  T = 2, 3, 17  below the first crowded level: the v_readlane kernels under every setting, the record is not reached -- the
                reference the other lengths' settings are held to runs the same code here (root only / one elimination
                without a right neighbour / eight eliminations)
  T = 18        the first length in the two-row form: nine eliminations on level 0 (two nodes per wave), every later level
                and the root through the record, the last node of a level without a right neighbour (zero block)
  T = 33        an odd number of eliminations on a paired level
  T = 48, 49    the last one-launch length and the first plan of two passes
  T = 65, 97    a last segment with a single node / a partial segment (next segment's first node present or not)
Per case and per setting of chain_pair x chain_merge: bt_solve, bt_logdet and bt_marginals of a positive definite chain
(cond <= 1e3 asserted; built by test_gpu_parity._spd_chain, the builder test_chain_pivot_gpu.py takes its positive definite
state from -- chain_pivot_ref.py itself builds indefinite chains only) against numpy's dense solve / inverse / slogdet in float64
at the bound of the other chain tests (TIGHT = 1e-9 relative; the measured errors are <= 8e-16), and the same WORDS in all four
settings: chain_pair 0 is the v_readlane form, which does not use the record.
One indefinite chain per n (chain_pivot_ref.indefinite_chain: the pivoted solve swaps rows in a good part of its nodes) takes
the row swaps through the new column loads.

Assemble-on-load (the dense path of the first pass, whose operands the eliminations read) at T = 33, n = 5 and 6, one binary
and one unary set registered in either order (the problems, contexts and sequence of test_asm_dense_vs_reference_gpu.py at
these shapes): g, V_D, V_U, dmu, the accepted state and the trial cost under assemble_on_load 1 equal those under 0 bit for
bit, and the launch classification says the batched path ran."""
import functools
import os

import numpy as np
import pytest

import chain_pivot_ref as R
from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import ALL_ON, _problem, _s2_a_then_b
from test_gpu_parity import TIGHT, _spd_chain, rel

pytestmark = pytest.mark.gpu

PAIR_DEFAULT = int(os.environ.get("GVI_CHAIN_PAIR", "1") != "0")      # the switches as the library read them
MERGE_DEFAULT = int(os.environ.get("GVI_CHAIN_MERGE", "1") != "0")
LENGTHS = (2, 3, 17, 18, 33, 48, 49, 65, 97)
SETTINGS = [(p, m) for p in (1, 0) for m in (1, 0)]


@functools.lru_cache(maxsize=None)
def spd_case(T, n):
    """the chain, a right-hand side and the float64 reference (solution, diagonal and super-diagonal blocks of the inverse,
    half log-determinant), computed once"""
    rng = np.random.default_rng(9100 * n + T)
    D, U = _spd_chain(T, n, rng)
    rhs = rng.normal(size=(T, n))
    A = R.dense(D, U)
    assert np.linalg.cond(A) <= 1e3
    Ai = np.linalg.inv(A)
    x = np.linalg.solve(A, rhs.reshape(-1)).reshape(T, n)
    SD = np.stack([Ai[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    SU = np.stack([Ai[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] for t in range(T - 1)])
    hld = 0.5 * np.linalg.slogdet(A)[1]
    for a in (D, U, rhs, x, SD, SU):
        a.setflags(write=False)
    return D, U, rhs, x, SD, SU, hld


def _all_settings(T, n, fn):
    """fn(ctx) under every (chain_pair, chain_merge); the switches are the context's own; they are put back before it closes"""
    out = {}
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        for pair, merge in SETTINGS:
            ctx.set_option("chain_pair", pair)
            ctx.set_option("chain_merge", merge)
            out[(pair, merge)] = fn(ctx)
    finally:
        ctx.set_option("chain_pair", PAIR_DEFAULT)
        ctx.set_option("chain_merge", MERGE_DEFAULT)
        ctx.close()
    return out


@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("T", LENGTHS)
def test_solve_and_factorisation_at_every_body(T, n):
    D, U, rhs, x_ref, SD_ref, SU_ref, hld_ref = spd_case(T, n)

    def run(ctx):
        SD, SU = ctx.bt_marginals(D, U)
        return ctx.bt_solve(D, U, rhs), np.array([ctx.bt_logdet(D, U)]), SD, SU

    out = _all_settings(T, n, run)
    x, hld, SD, SU = out[SETTINGS[0]]
    errs = (rel(x, x_ref), abs(hld[0] - hld_ref) / abs(hld_ref), rel(SD, SD_ref), rel(SU, SU_ref))
    print(f"lane record T {T} n {n}: x {errs[0]:.2e}  half log det {errs[1]:.2e}  Sig diagonal {errs[2]:.2e}  "
          f"Sig off-diagonal {errs[3]:.2e}  passes {len(R.chain_passes(T, n))}")
    assert max(errs) < TIGHT, errs
    for setting in SETTINGS[1:]:
        for got, want in zip(out[setting], out[SETTINGS[0]]):
            assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (setting, T, n)


@pytest.mark.parametrize("n", [5, 6])
def test_row_swaps_pass_through_the_column_loads(n):
    T = 97
    D, U, rhs = R.indefinite_chain(T, n, 4200 + n)
    ref = np.linalg.solve(R.dense(D, U), rhs.reshape(-1)).reshape(T, n)
    out = _all_settings(T, n, lambda ctx: ctx.bt_solve(D, U, rhs))
    err = rel(out[SETTINGS[0]], ref)
    print(f"lane record, indefinite T {T} n {n}: x {err:.2e}")
    assert err < TIGHT
    for setting in SETTINGS[1:]:
        assert out[setting].tobytes() == out[SETTINGS[0]].tobytes(), setting


@pytest.mark.parametrize("layout", ["bu", "ub"])
@pytest.mark.parametrize("n", [5, 6])
def test_assemble_on_load_feeds_the_same_operands(n, layout):
    T = 33
    P = _problem(T, n, layout, T - 1, T)
    gr1, st1, cost1, _, cnt1 = _s2_a_then_b(P, 1, ALL_ON)
    gr0, st0, cost0, _, cnt0 = _s2_a_then_b(P, 1, {**ALL_ON, "assemble_on_load": 0})
    assert cnt1[0] >= 1 and cnt1[1] == 0 and cnt0 == (0, 0), (cnt1, cnt0)
    assert np.isfinite(gr1["dmu"]).all() and np.isfinite(cost1)
    for k in ("g", "VD", "VU", "dmu"):
        assert np.array_equal(gr1[k], gr0[k]), k
    assert set(st1) == set(st0)
    for k in st1:
        assert np.array_equal(st1[k], st0[k]), k
    assert cost1 == cost0
