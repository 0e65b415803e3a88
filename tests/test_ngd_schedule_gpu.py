"""The driver of the resident iteration under one script that meets every kind of parked work with a reader other than the
next trial: a parked gradient solve and a pending assemble joined by gvi_ngd_get_gradients, a parked gather flushed by
gvi_ngd_factor_costs, a pipelined run whose first trials are rejected (the host's bookkeeping rolls back), NaN trials, and a
re-init with parked work outstanding.  The script runs under every scheduling switch, under every scheduling mode, and as the
split-form calls of the sharded driver; the one-state chain (T = 1) takes the route where the solve is launched at once.

include/gvi_hip.h calls the scheduling switches bit-identical: those legs are compared with == / np.array_equal (the fused
factor pass of the chain graphs aside, see FUSED_ROUNDS).  The modes are held to the tolerances of
test_gpu_parity.py::test_step_scheduling_modes_give_identical_iterates (costs 1e-12, state 1e-10).
The psi-pass counters are compared with a restatement of the pass order (passes_expected), not with the other leg."""
import functools

import numpy as np
import pytest

from chains import make_chain
from gaussianvi_amd import api

pytestmark = pytest.mark.gpu

GRAPHS = ["c2", "c3mini", "c3small", "planar", "one_state"]
SWITCHES = ["side_solve", "fuse_gather", "assemble_on_load", "pipeline", "fused", "pair_fuse"]
OPTION_LEGS = {name: (name,) for name in SWITCHES}
OPTION_LEGS["all_off"] = tuple(SWITCHES)
MODES = [(0, 0), (1, 0), (1, 1)]
DEFAULT_MODE = (1, 2)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name != "one_state":
        return make_chain(name)
    # the 1-D example of test_gpu_parity.py::test_k8_golden_ngd_trace_on_device: one state, one RANGE_1D factor
    spec = dict(d=1, p=10, start=np.zeros(1, np.int32), kind=api.PSI_RANGE_1D,
                params=np.array([[40.0 / 20.0 - 0.8, 20.0, 40.0, 0.09, 9.0]]), temperature=np.ones(1))
    return dict(T=1, n=1, specs=[spec], mu0=np.array([[20.0]]), D0=np.array([[[1.0 / 9.0]]]), U0=np.zeros((0, 1, 1)))


def fresh_context(name, options=(), mode=None):
    ch = graph(name)
    ctx, ids = api.context_for_chain(ch)
    for opt in options:
        ctx.set_option(opt, 0)
    if mode is not None:
        ctx.ngd_set_mode(*mode)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    ctx.ngd_counters(reset=True)
    return ctx


def gradients_or_none(ctx):
    """gvi_ngd_get_gradients refuses when the current state has no gradients (an accepted trial without speculation)."""
    try:
        return ctx.ngd_get_gradients()
    except api.GviError:
        return None


def perturbed(st, seed):
    """The state moved by a seeded 1e-3: the mean by 1e-3 N(0, 1) per entry, the precision by one factor 1 + 1e-3 u (it stays
    positive definite whatever its conditioning)."""
    rng = np.random.default_rng(seed)
    scale = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0)
    return st["mu"] + 1e-3 * rng.standard_normal(st["mu"].shape), st["D"] * scale, st["U"] * scale


def run_script(ctx):
    """-> dict(runs = the records of the four driver calls, events = records and re-inits in order, grad, fcost, state,
    counters)."""
    runs = [ctx.ngd_run(4, 0.55)]
    grad = gradients_or_none(ctx)               # joins a parked solve, flushes a pending assemble
    fcost = ctx.ngd_factor_costs(0)             # flushes a parked gather
    runs.append(ctx.ngd_run(3, 3.5))            # first trials rejected: the pipeline rolls back
    runs.append([ctx.ngd_step(40.0)])           # NaN trials
    ctx.ngd_init(*perturbed(ctx.ngd_get_state(), 0x5C4ED))   # re-init with parked work outstanding
    runs.append(ctx.ngd_run(3, 0.55))
    events = runs[0] + runs[1] + runs[2] + ["init"] + runs[3]
    return dict(runs=runs, events=events, grad=grad, fcost=fcost, state=ctx.ngd_get_state(), counters=ctx.ngd_counters())


@functools.lru_cache(maxsize=None)
def leg(name, options=(), mode=None):
    ctx = fresh_context(name, options, mode)
    out = run_script(ctx)
    ctx.close()
    return out


def passes_expected(events, speculate, fuse):
    """(full psi passes, cost-only psi passes) of a single-process context with factors, from the accept flags and trial
    counts alone -- the order of gvi_ngd_step (include/gvi_hip.h, gvi_ngd_set_mode):
    entry of an iteration: the cost and the gradients of the state, whichever is missing (one full pass serves both when
    neither is there and trials may be fused); first trial: one full pass when fused (always, or adaptively while first trials
    keep being accepted), else a cost pass plus -- with speculation -- the full pass of the next gradients; every later trial a
    cost pass.  An accepted first trial leaves the speculated gradients, any other accepted trial none."""
    full = cost = 0
    have_cost = have_grad = False
    first_accepted = True
    for e in events:
        if e == "init":
            have_cost = have_grad = False
            first_accepted = True
            continue
        if not have_cost and not have_grad and fuse != 0:
            full += 1
        else:
            cost += 0 if have_cost else 1
            full += 0 if have_grad else 1
        have_cost = have_grad = True
        if speculate and (fuse == 1 or (fuse == 2 and first_accepted)):
            full += 1
        else:
            cost += 1
            full += 1 if speculate else 0
        cost += e["ntrials"] - 1
        first_accepted = e["accepted"] and e["ntrials"] == 1
        if e["accepted"]:
            have_grad = bool(speculate) and e["ntrials"] == 1
    return full, cost


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300))


def records_equal(a, b):
    """== on the records, with NaN costs (a NaN trial that is reported) equal to themselves"""
    return len(a) == len(b) and all(x.keys() == y.keys() and all(
        x[k] == y[k] or (isinstance(x[k], float) and np.isnan(x[k]) and np.isnan(y[k])) for k in x) for x, y in zip(a, b))


def report_differences(label, ref, got):
    """prints what is not bit-identical between two legs, before anything is asserted"""
    for i, (a, b) in enumerate(zip(ref["runs"], got["runs"])):
        for j, (x, y) in enumerate(zip(a, b)):
            for k in x:
                if not (x[k] == y[k] or (x[k] != x[k] and y[k] != y[k])):
                    print(f"    [{label}] run {i} iteration {j} {k}: {x[k]!r} / {y[k]!r}")
    for part in ("grad", "state"):
        for k in (ref[part] or {}):
            if got[part] is not None and ref[part][k].size and not np.array_equal(ref[part][k], got[part][k], equal_nan=True):
                print(f"    [{label}] {part} {k}: rel {rel(got[part][k], ref[part][k]):.2e}")
    if not np.array_equal(ref["fcost"], got["fcost"]):
        print(f"    [{label}] factor costs: rel {rel(got['fcost'], ref['fcost']):.2e}")
    if ref["counters"] != got["counters"]:
        print(f"    [{label}] counters: {ref['counters']} / {got['counters']}")


@pytest.mark.parametrize("name", GRAPHS)
def test_default_leg_takes_the_expected_passes(name):
    ref = leg(name)
    assert [len(r) for r in ref["runs"]][0] == 4 and len(ref["runs"][3]) == 3      # the 0.55 runs go their full length
    assert ref["grad"] is not None
    assert ref["counters"] == passes_expected(ref["events"], *DEFAULT_MODE), (ref["counters"], ref["events"])


@pytest.mark.parametrize("name", ["c2", "c3small"])
def test_script_backtracks(name):
    """Without a rejected first trial the script would not reach the backtracking and roll-back paths (the oracle run on
    the CPU gives ntrials 2 for each of the three base-3.5 iterations on both chains)."""
    ref = leg(name)
    assert any(r["ntrials"] > 1 for r in ref["runs"][1]), ref["runs"][1]
    assert any(r["ntrials"] > 1 for r in ref["events"] if r != "init")


# The one-launch factor pass of the chain graphs (option "fused"; "pair_fuse" 0 switches it off too) sums a factor's chunks in
# another order than the three launches prep -> psi -> epilogue: measured on the parent of the commit that added this module,
# fused 1 / 0 give new_cost 425.0226401808743 / ...744 (c2), cost 137.0049978532434 / ...24268 (c3mini), 486.2860122962786 /
# ...28816 (c3small); gradients differ by up to 1.1e-11, the state by up to 4.9e-13 (relative).  On these graphs the legs
# without the fused pass are held to the modes' tolerances against the default leg and bit for bit against the "fused" 0 leg;
# planar (block3) and the one-state chain are bit-identical under every switch.
FUSED_ROUNDS = {"c2", "c3mini", "c3small"}
LEGS_WITHOUT_FUSED_PASS = {"fused", "pair_fuse", "all_off"}


def assert_bit_identical(ref, got):
    for i, (a, b) in enumerate(zip(ref["runs"], got["runs"])):
        assert records_equal(a, b), (i, a, b)
    assert got["grad"] is not None and same_bits(ref["grad"], got["grad"])
    assert np.array_equal(ref["fcost"], got["fcost"])
    assert same_bits(ref["state"], got["state"])


def assert_same_iterates(ref, got, arrays=("state",)):
    """accept flags and trial counts equal, costs to 1e-12, arrays to 1e-10"""
    for a, b in zip(ref["runs"], got["runs"]):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x["accepted"] == y["accepted"] and x["ntrials"] == y["ntrials"]
            assert np.isclose(x["cost_iter"], y["cost_iter"], rtol=1e-12, atol=0.0, equal_nan=True)
            assert np.isclose(x["new_cost"], y["new_cost"], rtol=1e-12, atol=0.0, equal_nan=True)
    for part in arrays:
        for k in ref[part]:
            if ref[part][k].size:
                assert rel(got[part][k], ref[part][k]) < 1e-10, (part, k)


@pytest.mark.parametrize("switch", sorted(OPTION_LEGS))
@pytest.mark.parametrize("name", GRAPHS)
def test_option_leg_is_bit_identical(name, switch):
    ref, got = leg(name), leg(name, OPTION_LEGS[switch])
    report_differences(f"{name} {switch}", ref, got)
    if name in FUSED_ROUNDS and switch in LEGS_WITHOUT_FUSED_PASS:
        assert got["grad"] is not None
        assert_same_iterates(ref, got, arrays=("state", "grad"))
        assert rel(got["fcost"], ref["fcost"]) < 1e-10
        assert_bit_identical(leg(name, OPTION_LEGS["fused"]), got)
    else:
        assert_bit_identical(ref, got)
    # no switch changes the pass count: the passes follow from the mode and the accept decisions alone
    assert got["counters"] == passes_expected(got["events"], *DEFAULT_MODE) == ref["counters"]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"spec{m[0]}fuse{m[1]}")
@pytest.mark.parametrize("name", GRAPHS)
def test_mode_leg_gives_the_same_iterates(name, mode):
    ref, got = leg(name), leg(name, (), mode)
    assert_same_iterates(ref, got)
    assert got["counters"] == passes_expected(got["events"], *mode), (got["counters"], got["events"])


def split_form_iteration(ctx, step):
    """One iteration written as the sharded driver writes it: first trial at 0.75 step with the next gradients queued behind
    its published cost; -> (cost of the trial, accepted)"""
    c0 = ctx.ngd_cost()
    ctx.ngd_gradients()
    ctx.ngd_trial_local(0.75 * step)
    ctx.ngd_trial_publish()
    ctx.ngd_spec_gradients_local()
    ctx.ngd_spec_gradients_finish()
    c1 = ctx.ngd_trial_wait()
    assert c1 < c0                              # the comparison below is of accepted first trials
    ctx.ngd_accept_spec()
    return c0, c1


@pytest.mark.parametrize("name", ["c3mini", "c2"])
def test_split_form_calls_equal_the_step(name):
    ctx = fresh_context(name, mode=(1, 0))
    want = [ctx.ngd_step(0.55) for _ in range(3)]
    want_grad, want_state = ctx.ngd_get_gradients(), ctx.ngd_get_state()
    ctx.close()
    assert all(r["accepted"] and r["ntrials"] == 1 for r in want)
    ctx = fresh_context(name, mode=(1, 0))
    got = [split_form_iteration(ctx, 0.55) for _ in range(3)]
    got_grad, got_state = ctx.ngd_get_gradients(), ctx.ngd_get_state()
    ctx.close()
    assert [(r["cost_iter"], r["new_cost"]) for r in want] == got
    assert same_bits(want_state, got_state)
    assert same_bits(want_grad, got_grad)


GVI_ERR_STATE = 5


def prior_set(name):
    return next(i for i, spec in enumerate(graph(name)["specs"]) if spec["kind"] == api.PSI_QUAD_PRIOR)


# setters that mark the costs and gradients of the resident iteration stale (the full list: DESIGN.md section 4.5)
SETTERS = {
    "temperature": lambda ctx: ctx.factors_set_temperature(prior_set("c2"), np.full(ctx.sets[prior_set("c2")][0], 2.0)),
    "closed_form": lambda ctx: ctx.factors_set_closed_form(prior_set("c2"), False),
    "option_mirror": lambda ctx: ctx.set_option("mirror", 1),
}


@pytest.mark.parametrize("setter", sorted(SETTERS))
def test_a_setter_drops_the_speculative_gradients(setter):
    """Gradients queued at the trial state were computed under the old setting: after a setter gvi_ngd_accept_spec refuses
    them (GVI_ERR_STATE), gvi_ngd_accept still takes the trial, and the iteration goes on exactly as on a context that never
    speculated and had the setter applied at the same point."""
    first = 0.75 * 0.55
    ctx = fresh_context("c2", mode=(1, 0))
    c0 = ctx.ngd_cost()
    ctx.ngd_gradients()
    ctx.ngd_trial_local(first)
    ctx.ngd_trial_publish()
    ctx.ngd_spec_gradients_local()
    ctx.ngd_spec_gradients_finish()
    c1 = ctx.ngd_trial_wait()
    assert c1 < c0
    SETTERS[setter](ctx)
    with pytest.raises(api.GviError, match="no speculative gradients at the trial state") as e:
        ctx.ngd_accept_spec()
    assert e.value.status == GVI_ERR_STATE
    ctx.ngd_accept()
    got, got_state = ctx.ngd_step(0.55), ctx.ngd_get_state()
    ctx.close()

    ctx = fresh_context("c2", mode=(1, 0))
    assert ctx.ngd_cost() == c0
    ctx.ngd_gradients()
    assert ctx.ngd_trial(first) == c1
    SETTERS[setter](ctx)
    ctx.ngd_accept()
    want, want_state = ctx.ngd_step(0.55), ctx.ngd_get_state()
    ctx.close()
    print(f"{setter}: step after the setter {got} / without speculation {want}")
    assert got == want
    assert same_bits(want_state, got_state)


def test_the_retired_option_name_is_refused():
    ctx = api.Context(0)
    for name in ("dual_chain", "orbit_stack"):
        with pytest.raises(api.GviError, match="unknown option"):
            ctx.set_option(name, 0)
    ctx.close()
