"""The chain's A/B switches belong to the context that set them (-m gpu).

chain_wave, asm_dense and chain_pair are fields of a context's options (options.hpp) and reach the chain launches as
chain_plan.hpp::ChainRules: a value set on one context changes no other context of the process.  Two contexts are alive
together on the smallest graph whose assemble-on-load takes the batched load path -- one binary set B(T - 1) and one unary set
U(T), built as tests/test_asm_dense_vs_reference_gpu.py builds it (the module tests/test_asm_set_layouts_gpu.py takes its
contexts from) -- once at (T, n) = (5, 2), the lane-per-node kernel's range, and once at (70, 6), the two-row form's.  Context A
sets the three switches to 0, context B sets nothing; two ngd_step of each alternate.  gvi_debug_asm_launches counts per
process where a launch with an assemble list went: A's steps move only the generic counter and B's only the dense one, and B's
iterates are bit for bit those of a default context that ran before A existed."""
import numpy as np
import pytest

from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import DENSE_DEFAULT, _counted, _problem

pytestmark = pytest.mark.gpu


def _context(P, **options):
    T, n = P["T"], P["n"]
    ctx = api.Context(0)
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.chain_set(T, n)
    ctx.factors_add(2 * n, 3, np.arange(T - 1, dtype=np.int32), api.PSI_QUAD_PRIOR,
                    np.concatenate([P["Phi"].reshape(T - 1, -1), P["Q"].reshape(T - 1, -1)], 1))
    ctx.factors_add(n, 3, np.arange(T, dtype=np.int32), api.PSI_FIXED_PRIOR, np.concatenate([P["mu_u"], P["Kinv"].reshape(T, -1)], 1))
    ctx.ngd_init(*P["A"])
    return ctx


def _step(ctx):
    """one ngd_step: (its result, the state it left), and what it added to the (dense, generic) counters"""
    return _counted(lambda: (ctx.ngd_step(0.55, 10), ctx.ngd_get_state()))


@pytest.mark.parametrize("T,n", [(5, 2), (70, 6)])
def test_switches_set_on_one_context_leave_another_alone(T, n):
    P = _problem(T, n, "bu", T - 1, T)
    first = _context(P)                                            # default switches, before A exists
    try:
        want = [_step(first)[0] for _ in range(2)]
    finally:
        first.close()
    A = _context(P, asm_dense=0, chain_pair=0, chain_wave=0)
    B = _context(P)
    try:
        got, counts = {"A": [], "B": []}, {"A": [], "B": []}
        for _ in range(2):
            for name, ctx in (("A", A), ("B", B)):
                out, cnt = _step(ctx)
                got[name].append(out)
                counts[name].append(cnt)
    finally:
        A.close()
        B.close()
    print(f"    (T, n) = ({T}, {n}): (dense, generic) launches of A's steps {counts['A']}, of B's steps {counts['B']}")
    for dense, generic in counts["A"]:
        assert dense == 0 and generic >= 1, counts
    for dense, generic in counts["B"]:                              # (B follows the environment the library read, like any default context)
        assert (dense >= 1 and generic == 0) if DENSE_DEFAULT else (dense == 0 and generic >= 1), counts
    for (r, st), (r0, st0) in zip(got["B"], want):
        assert r == r0, (r, r0)
        for k in st0:
            assert np.array_equal(st[k], st0[k]), k
    for (r, st), (r0, st0) in zip(got["A"], want):                  # A's legs compute the same iteration (chain_wave 0: to rounding)
        assert r["accepted"] == r0["accepted"] and r["ntrials"] == r0["ntrials"]
        assert np.abs(st["mu"] - st0["mu"]).max() <= 1e-9 * np.abs(st0["mu"]).max()
