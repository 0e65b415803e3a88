"""The pivoted half of the chain kernels (bt_solve; the mean step of an NGD iteration) on chains whose eliminations DO swap rows,
at every compiled block size and at the chain lengths where the pass plan changes (-m gpu).

kernels_chain.hpp eliminate<PIVOT = true> (v_readlane form, every N), gj_rowb (N = 6, also two nodes per wave in eliminate2) and
kernels_chain_wave.hpp gauss_jordan<true> each carry the threshold rule "swap rows when |natural pivot| * 8 < column maximum".
On the positive definite chains of the other tests the natural pivot is always taken.  Here the inputs come from
chain_pivot_ref.py: indefinite, well-conditioned blocks (rows are swapped in a good part of the nodes, on every level, in every
pass, at every step, into the last row, in padded blocks, in nodes without a right neighbour, in the root) and chains with
leading diagonal entries of exactly 0.0, on which an unpivoted elimination divides by zero.  test_chain_pivot_host.py proves on
the CPU, for every case below, that the reference is right, that the input is well conditioned (cond <= 1e2, system and every
inverted block), that no pivot decision is closer than 1e-6 to the threshold and that these swaps do occur.

Per case, in one context: bt_solve of a positive definite state A of the shape, then of the indefinite state B into an array of
its own; only B is compared --
  * with numpy's dense solve (T n <= 1600) or the float64 census at TIGHT = 1e-9 (test_gpu_parity's bound for the operation; the
    reference's own error is ~1e-15 at these condition numbers and a wrong swap is an error of order one), and by its residual;
  * a second solve of B: the same words;
  * bt_logdet of B is NaN and returns; bt_logdet of A is what it was before;
  * plans of two or more passes: chain_merge 1, 0, 1 give the same words; n = 5, 6: chain_pair 1 and 0 give the same words;
  * n <= 2, T <= 65: the lane-per-node kernel and the generic N = 1, 2 kernels (chain_wave 1, 0), each against the reference and
    against each other at 1e-13.

Largest relative error of x per padded block size over all cases (115 of them, 4 s), measured on an MI355X:
  N = 1: 1.2e-16   N = 2: 7.2e-16   N = 3: 8.5e-16   N = 4: 2.0e-15   N = 6: 2.9e-15   N = 8: 2.8e-15   N = 12: 3.9e-15
  N = 16: 5.3e-15   (largest residual: 1.6e-14, N = 12).  No case failed; no kernel was changed.

What these cases can and cannot see: a swap is harmless when every lane of the tile makes the same one, so they catch a swap that
is not the same in all columns of a tile (an error of order one), and, through the zero pivots, a swap that is missing at the first
step.  A kernel that swapped a different row than the rule says, consistently, would still pass: with blocks this well conditioned
any row above the threshold is a good pivot."""
import functools
import os

import numpy as np
import pytest

import chain_pivot_ref as R
from gaussianvi_amd import api
from test_gpu_parity import TIGHT, _spd_chain, rel

pytestmark = pytest.mark.gpu

WAVE_DEFAULT = int(os.environ.get("GVI_CHAIN_WAVE", "1") != "0")      # the switches as the library read them
PAIR_DEFAULT = int(os.environ.get("GVI_CHAIN_PAIR", "1") != "0")
MERGE_DEFAULT = int(os.environ.get("GVI_CHAIN_MERGE", "1") != "0")
IDS = [f"T{T}-n{n}-{gen}" for T, n, gen in R.CASES]


@functools.lru_cache(maxsize=None)
def state_a(T, n):
    rng = np.random.default_rng(7000 * n + T)
    D, U = _spd_chain(T, n, rng)
    rhs = rng.normal(size=(T, n))
    for a in (D, U, rhs):
        a.setflags(write=False)
    return D, U, rhs


@functools.lru_cache(maxsize=None)
def reference(T, n, gen):
    D, U, rhs, xc, _ = R.case(T, n, gen)
    ref = np.linalg.solve(R.dense(D, U), rhs.reshape(-1)).reshape(T, n) if T * n <= 1600 else xc
    ref.setflags(write=False)
    return ref


def solve_b(ctx, A, B, **options):
    """bt_solve of state A, then of state B, under the options; B's result"""
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.bt_solve(*A)
    return ctx.bt_solve(*B)


@pytest.mark.parametrize("T,n,gen", R.CASES, ids=IDS)
def test_pivoted_solve_with_row_swaps(T, n, gen):
    D, U, rhs, _, info = R.case(T, n, gen)
    A, B, ref = state_a(T, n), (D, U, rhs), reference(T, n, gen)
    npass = len(R.chain_passes(T, n))
    merge, pair, wave = [], {}, {}
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        ld_a = ctx.bt_logdet(A[0], A[1])
        x = solve_b(ctx, A, B)
        x_again = ctx.bt_solve(*B)
        ld_b = ctx.bt_logdet(D, U)
        ld_a_after = ctx.bt_logdet(A[0], A[1])
        if npass >= 2:
            merge = [solve_b(ctx, A, B, chain_merge=m) for m in (1, 0, 1)]
            ctx.set_option("chain_merge", MERGE_DEFAULT)
        if n in (5, 6):
            pair = {p: solve_b(ctx, A, B, chain_pair=p) for p in (1, 0)}
        if n <= 2 and T <= 65:
            wave = {w: solve_b(ctx, A, B, chain_wave=w) for w in (1, 0)}
    finally:
        ctx.set_option("chain_merge", MERGE_DEFAULT)
        ctx.set_option("chain_pair", PAIR_DEFAULT)                   # (the context closes next: harmless)
        ctx.set_option("chain_wave", WAVE_DEFAULT)
        ctx.close()
    errs = [rel(x, ref)] + [rel(v, ref) for v in wave.values()]
    res = R.block_residual(D, U, x, rhs)
    nsw = [sum(bool(r["swaps"]) and r["level"] == l for r in info) for l in range(R.chain_levels(T) + 1)]
    print(f"pivot case T {T} n {n} N {R.padded(n)} {gen}: x against the reference {max(errs):.2e}, residual {res:.2e}, "
          f"swapped nodes per level {nsw} of {T}, {sum(len(r['swaps']) for r in info)} swaps, passes {npass}")
    assert max(errs) < TIGHT
    assert res < 1e-9 * max(1.0, np.abs(D).max()) * max(1.0, np.abs(x).max())
    assert x_again.tobytes() == x.tobytes()
    assert np.isnan(ld_b) and np.isfinite(ld_a) and ld_a_after == ld_a, (ld_a, ld_b, ld_a_after)
    if npass >= 2:
        assert merge[0].tobytes() == merge[1].tobytes() and merge[2].tobytes() == merge[1].tobytes()
        assert rel(merge[1], ref) < TIGHT
    if pair:
        assert pair[1].tobytes() == pair[0].tobytes()
        assert rel(pair[0], ref) < TIGHT
    if wave:
        assert rel(wave[1], wave[0]) < 1e-13
