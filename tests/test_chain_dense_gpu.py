"""The batched first-pass load of the chain kernels against the paths it must agree with, bit for bit (-m gpu).

kernels_chain.hpp's dense assemble-on-load (one binary and one unary factor set: every load of a round issued before the
first use) forms the same sums in the same order as the generic set loop and as the stand-alone assemble launch.  So on every
chain an NGD run must not depend on which of them ran: option assemble_on_load 1 against 0, chain_merge 1 against 0, and the
batched path against the generic set loop (asm_dense 1 against 0) give the same state, the same accept decisions and the same
trial counts after six steps.  Every run starts from a freshly perturbed state in a context that has already taken a step
from another state, so nothing a run reads can be left over from the run it is compared with.

Chains: c3small (33 states: one launch, the TOP instance), c3mini (9 states), c3t75 (75 states: a segmented first pass whose
last workgroup holds 11 of 32 nodes -- T - 1 = 74 is not a multiple of 32 -- and the merged top + backward launch) and planar
(sparse anchor sets: the generic loop stays in charge).  api.asm_launches() says which of the two a run's launches were
classified for: the batched path on the three LTV chains, the generic loop on planar and under asm_dense 0, neither where the
assemble is a launch of its own."""
import os

import numpy as np
import pytest

from chains import make_chain
from gaussianvi_amd import api
from gaussianvi_amd import synthetic as syn
from test_handover_fresh_gpu import _state_b

pytestmark = pytest.mark.gpu

syn.CONFIGS.setdefault("c3t75", (39, 75, 6, 5, "ltv"))
STEPS = 6
DENSE_DEFAULT = int(os.environ.get("GVI_ASM_DENSE", "1") != "0")     # the switch as a context reads it at creation
ON_LOAD_DEFAULT = int(os.environ.get("GVI_ASM_ON_LOAD", "1") != "0")  # (per context, read at its creation)


def _run(ch, seed, options):
    """ngd_init on the chain's own state and one step, then ngd_init on the perturbed state B(seed) and STEPS steps"""
    muB, DB, UB = _state_b(ch, np.random.default_rng(seed))
    ctx, _ = api.context_for_chain(ch)
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        ctx.ngd_step(0.55, 10)
        ctx.ngd_init(muB, DB, UB)
        before = api.asm_launches()
        results = [ctx.ngd_step(0.55, 10) for _ in range(STEPS)]
        state = ctx.ngd_get_state()
        after = api.asm_launches()
    finally:
        ctx.set_option("asm_dense", DENSE_DEFAULT)  # (the context closes next: harmless)
        ctx.close()
    # the launches that assembled while loading: all on the batched path, all on the generic loop, or none at all
    dense, generic = after[0] - before[0], after[1] - before[1]
    if not options.get("assemble_on_load", ON_LOAD_DEFAULT):
        assert (dense, generic) == (0, 0), (options, dense, generic)
    elif ch["name"] != "planar" and options.get("asm_dense", DENSE_DEFAULT):
        assert dense >= 1 and generic == 0, (options, dense, generic)
    else:
        assert dense == 0 and generic >= 1, (options, dense, generic)
    return results, state


@pytest.mark.parametrize("name", ["c3small", "c3mini", "c3t75", "planar"])
def test_ngd_does_not_depend_on_the_load_path(name):
    ch = make_chain(name)
    seed = 100 + len(name) + ch["T"]
    base_r, base_s = _run(ch, seed, {})
    assert all(np.isfinite(base_s[k]).all() for k in base_s)
    assert any(r["accepted"] for r in base_r)
    for options in ({"assemble_on_load": 0}, {"chain_merge": 0}, {"asm_dense": 0}):
        r, s = _run(ch, seed, options)
        assert [(x["accepted"], x["ntrials"]) for x in r] == [(x["accepted"], x["ntrials"]) for x in base_r], options
        assert [x["new_cost"] for x in r] == [x["new_cost"] for x in base_r], options
        assert set(s) == set(base_s)
        for k in s:
            assert np.array_equal(s[k], base_s[k]), (options, k)


def test_a_different_start_gives_a_different_run():
    """The comparison above can see a difference: another perturbation moves the state at every node."""
    ch = make_chain("c3mini")
    _, a = _run(ch, 5, {})
    _, b = _run(ch, 6, {})
    assert (np.abs(a["mu"] - b["mu"]).max(axis=1) > 0).all()
