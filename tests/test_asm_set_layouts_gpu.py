"""The set-loop copies of the assemble-on-load against two float64 references, on set lists no fixture has: sparse sets
anywhere, repeated and unsorted starts, several sets of a kind, MAX_SETS sets (-m gpu; the reference test needs no GPU).

The chain kernels form g, V_D and V_U from the per-factor results while they load their first pass.  Next to the dense path
(tests/test_asm_dense_vs_reference_gpu.py) there are two loops over the set list -- asm_element / asm_pair (kernels_chain.hpp,
generic kernels) and asm_loads / asm_node (kernels_chain_wave.hpp, lane-per-node kernel, n <= 2, T <= 65) -- and the stand-alone
CSR kernel they must equal, bt_scatter_all_kernel (kernels_bt.hpp).  Every fixture of synthetic.py has the same list (priors,
one full unary set, anchors at [0, T - 1], n >= 4); the rows here are small random quadratic chains (QUAD_PRIOR / FIXED_PRIOR,
GH degree 3, EVERY factor its own temperature from [0.5, 2], so a factor read from another's slot shows).  B(K) / U(K): binary /
unary set with start = arange(K); S(...): unary set with that start list; Bx(...): binary set with that start list.

Rows and the line each is there for.  W rows run with chain_wave 1 and 0 (the same list on the generic N = 1, 2 kernels):
  W1  asm_node's call asm_loads(a, n, t2 = 64, on2, hasc = false): node 64 in lane 0's second register set takes a sparse hit
      (a.sp[k] == t2), lane 0's own node another; three sets: the last round aliases b to a and drops it (on && second)
  W2  no node 64 (two = false); the sparse set first and descending; U(40): own = t < a.K false on 24 lanes; odd count again
  W3  T = 2, n = 1: r < n && c < n on the identity-padded block; two factors on state 1 (d0[el] += ..., g0[r] += ...), no full set
  W4  one interior anchor (K = 1, start[0] = 2 != 0: sparse); two binary sets, left = t - 1 < a.K of the shorter; even count
  W5  MAX_SETS sets, four rounds of asm_node; S(5, 5, 5, 5): ASM_SPARSE_MAX factors on one state; S(0) has start[k] = k, so it goes
      as U(1) (nsp = 0), S(32) as a sparse set
  W6  no binary set: two = false everywhere, V_U = 0 exactly, up = two && ... && hasc never loads
  W7  (added, see below) four factors on state 2 at n = 2: six four-term sums whose order the bit comparison can see
  G1  N = 3; asm_pair's sparse branch in the first set of the sweep, starts unsorted
  G2  T = 70, the first length the lane-per-node kernel refuses (WT_MAX = 65), four sets, B(30) ends inside the chain
  G3  segmented first pass at N = 1 (cap 128): hits on the partial last workgroup's first node (128), on the last node of the
      workgroup before (127), on the chain's last node (130) and on node 0
  G4  the headline pattern (n = 6, B(T - 1) U(T)) plus anchors: three sets, so chain_asm_dense says no and asm_pair runs
  G5  padded N = 8 (ext_el: xe < 0 on the padding), segmented, two sparse sets, S(0, 13, 13) twice on one state
  G6  N = 12: two load rounds per thread (e0 += 2 nthr)
  G7  (added) four factors on state 3 at n = 4: twenty four-term sums for the bit comparison
  F1  K = ASM_SPARSE_MAX + 1: asm_on_load_ok's s->K <= ASM_SPARSE_MAX
  F2  Bx(0, 0, 3, 7, 7): not start[k] = k and d = 2n, so no sparse form either; CSR lists of length 0 and 2 in bt_scatter_all_kernel
  F3  K = 12 > T = 6 (chain_structured's K <= T; the first T starts are arange) and K > ASM_SPARSE_MAX
  F4  K = T - 1 binary factors, permuted
W and G rows must assemble on load through the set loop, F rows must not assemble on load at all; api.asm_launches() tells.

References.  (1) The oracle (gvi_oracle.ChainNGD; FactorSet takes any start list).  (2) The closed form of asm_closed_form.py,
no quadrature: V = sum of Hessian_k / temperature_k over start, g = sum of the gradients at the mean, dmu = solve(dense V, -g),
cost = sum (psi_k(mu_k) + tr(H_k Sigma_k) / 2) / temperature_k + log det / 2.  The bound is TIGHT = 1e-9.  On the CPU the two
references differ, largest over all rows, by 5.9e-14 (g), 3.9e-12 (V_D), 7.0e-13 (V_U), 7.4e-12 (dmu) and 1.4e-12 (costs):
asserted below TIGHT / 5 in test_rows_are_well_conditioned_and_the_references_agree, with cond(dense V) <= 1e4 for every row
(W2: 1.4e3, the 23 states between U(40) and the anchor on 63 hang on binary factors alone; every other row <= 16).

Sequences, per case in ONE context, on state A and then (ngd_init) on state B, B against B's references and g_B far from g_A
at every node (state B is chosen on the CPU so that the closed-form gradients are): S1 ngd_gradients, ngd_get_gradients;
S2 ngd_gradients, ngd_trial, ngd_get_gradients, ngd_accept; S3 one ngd_step.  Checked: g, V_D, V_U, dmu, the trial D / U / SigD /
SigU, the accepted mu, cost_iter, the trial cost and the accept decision against both references; g, V_D, V_U, dmu, accepted
state and cost bit for bit between assemble_on_load 1 and 0; the launch counters of every sequence.

What the module sees: six breaks of one predicate or summand each (every load stays inside its array), tried in three libraries
-- the first, second and fourth in one, the third and fifth in another; the breaks sharing a library sit in code that different
rows reach.  Each library ran once, the last twice (before and after W7 got its fourth factor):
  asm_node: on && second -> on, if (second) -> if (true) (an odd list's last set counted twice)   W1, W2 on chain_wave 1: g 0.34, 0.57
    (either half alone changes nothing: the loads return zeros, or the sum is skipped)
  asm_pair: d0[u] += -> d0[u] = in the sparse branch (the last factor on a state wins)              W3, W5 on chain_wave 0, G5: V_D 0.30 .. 0.47
  asm_loads: d0[el] += / g0[r] += -> = in the sparse branch                                          W3, W5 on chain_wave 1, the ninth-set test: g 0.27, 0.38
  asm_on_load_ok: s->K <= ASM_SPARSE_MAX + 1                                                         F1: counters (0, 1), its fifth factor lost
  asm_element: the sparse loop descending in k (g summed in the other order)                         NOTHING: W5's S(5, 5, 5, 5) is one scalar at
    n = 1, its four terms gave the same double in either order, and S(0, 13, 13), S(1, 1, 0) are two-term sums (x + y = y + x).
    Rows W7 and G7 were added for that: four factors on one state at n = 2 and 4.  (W7 first had three, S(2, 2, 2, 1): the next
    build did not show on it either, so it got a fourth; the run below is the one with four.)
  all three sparse loops (asm_element, asm_pair, asm_loads) descending in k                          the bit comparison of W5, W7 (both
    chain_wave legs) and G7: V_D on W5, g on W7 and G7; all 47 other cases pass, the comparisons with the references included (the
    error is an ulp) -- only the equal-bits check pins the order, and only rows with four factors on one state show it.
No row exposed a defect in the library.
"""
import functools

import numpy as np
import pytest

import gvi_oracle as o
from asm_closed_form import closed_form, closed_form_cost
from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import STEP, _counted, _hold, _restore, _s1, _s2, _state
from test_gpu_parity import TIGHT, rel
from test_handover_fresh_gpu import far_at_every_node

gpu = pytest.mark.gpu

GVI_ERR_UNSUPPORTED = 3
ASM_SPARSE_MAX, MAX_SETS = 4, 8                                   # kernels_chain.hpp, device_common.hpp
ALL_ON = dict(asm_dense=1, assemble_on_load=1, chain_merge=1)


def B(K): return ("b", list(range(K)))
def U(K): return ("u", list(range(K)))
def S(*start): return ("u", list(start))
def Bx(*start): return ("b", list(start))


# row: (T, n, sets in registration order, assembles on load)
ROWS = {
    "W1": (65, 2, [B(64), U(65), S(0, 64)], True),
    "W2": (64, 2, [S(63, 0), B(63), U(40)], True),
    "W3": (2, 1, [B(1), S(1, 1, 0)], True),
    "W4": (5, 2, [S(2), B(4), U(5), B(3)], True),
    "W5": (33, 1, [B(32), U(33), S(0), S(32), S(5, 5, 5, 5), U(10), B(32), S(16, 3)], True),
    "W6": (3, 2, [U(3), S(1)], True),
    "W7": (4, 2, [B(3), S(2, 2, 2, 2)], True),
    "G1": (9, 3, [S(8, 0, 4), B(8), U(9)], True),
    "G2": (70, 2, [B(69), S(0, 69), U(70), B(30)], True),
    "G3": (131, 1, [B(130), U(131), S(130, 128, 0, 127)], True),
    "G4": (49, 6, [B(48), U(49), S(0, 48)], True),
    "G5": (27, 7, [S(26), B(26), U(27), S(0, 13, 13)], True),
    "G6": (11, 12, [B(10), U(11), S(10, 0)], True),
    "G7": (7, 4, [B(6), U(7), S(3, 3, 3, 3)], True),
    "F1": (9, 2, [B(8), S(0, 2, 4, 6, 8)], False),
    "F2": (9, 2, [Bx(0, 0, 3, 7, 7), U(9)], False),
    "F3": (6, 3, [B(5), S(0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5)], False),
    "F4": (4, 2, [Bx(1, 2, 0), U(4)], False),
}
# W rows: the lane-per-node kernel (chain_wave 1) and the same list on the generic N = 1, 2 kernels (chain_wave 0)
CASES = [(r, w) for r in ROWS for w in ((1, 0) if r[0] == "W" else (1,))]
IDS = [f"{r}-wave{w}" for r, w in CASES]
COND_MAX = 1e4
FAR_REF = 3e-3                                                    # three times what far_at_every_node is asserted at on the device


@functools.lru_cache(maxsize=None)
def _problem(row):
    """The factor sets (every factor with its own temperature from [0.5, 2]) and the two states of a row"""
    T, n, spec, on_load = ROWS[row]
    rng = np.random.default_rng(100 * ord(row[0]) + int(row[1:]))   # (of the row's name: adding a row moves no other)
    sets = []
    for kind, start in spec:
        K = len(start)
        G = rng.normal(size=(K, n, n))
        s = dict(kind=kind, start=np.array(start, dtype=np.int32), temp=rng.uniform(0.5, 2.0, K))
        if kind == "b":
            s["Phi"] = np.eye(n)[None] + 0.05 * rng.normal(size=(K, n, n))
            s["Q"] = G @ G.transpose(0, 2, 1) / n + 2.0 * np.eye(n)
        else:
            s["mu_u"] = rng.normal(size=(K, n))
            s["Kinv"] = G @ G.transpose(0, 2, 1) / n + 1.5 * np.eye(n)
        sets.append(s)
    # state B: the first of a fixed sequence of random states whose gradient (closed form, CPU) is FAR_REF away from state A's
    # at every node -- at n = 1 and T = 131 two random scalars out of 131 pairs come closer than 1e-3 one time in three
    stA = _state(T, n, np.random.default_rng(7 * T + n + 1))
    gA = closed_form(T, n, sets, stA[0], solve=False)["g"]
    for j in range(64):
        stB = _state(T, n, np.random.default_rng(11 * T + n + 2 + 1000 * j))
        if far_at_every_node(closed_form(T, n, sets, stB[0], solve=False)["g"], gA, T) > FAR_REF:
            break
    else:
        raise AssertionError(f"{row}: no state B far from state A")
    return dict(T=T, n=n, sets=sets, on_load=on_load, A=stA, B=stB)


def _oracle_sets(P):
    out = []
    for s in P["sets"]:
        if s["kind"] == "b":
            fs = o.FactorSet(s["start"], 2 * P["n"], 3, o.psi_batch_quad_prior(s["Phi"], s["Q"]))
        else:
            fs = o.FactorSet(s["start"], P["n"], 3, o.psi_batch_fixed_prior(s["mu_u"], s["Kinv"]))
        fs.temperature = s["temp"].copy()
        out.append(fs)
    return out


@functools.lru_cache(maxsize=None)
def _references(row):
    """Both references of state B (closed form, oracle), computed once per row and shared read-only by the tests"""
    P = _problem(row)
    T, n = P["T"], P["n"]
    mu, D, U = P["B"]
    cf = closed_form(T, n, P["sets"], mu)
    cf["cond"] = np.linalg.cond(o.bt_to_dense(cf["VD"], cf["VU"]))
    chain = o.ChainNGD(T, n, _oracle_sets(P), mu, D, U)
    dmu, _, _, (g, VD, VU) = chain.gradients()
    ora = dict(g=g, VD=VD, VU=VU, dmu=dmu)
    for r in (cf, ora):                                           # the first trial of ngd_step(0.55, .), from each reference's own V
        r["D"], r["U"], r["mu"] = D + STEP * (r["VD"] - D), U + STEP * (r["VU"] - U), mu + STEP * r["dmu"]
    ora["SigD"], ora["SigU"] = o.inverse_gbp(ora["D"], ora["U"])
    ora["cost_iter"] = chain.cost_value(mu, D, U)
    ora["cost"] = chain.cost_value(ora["mu"], ora["D"], ora["U"], ora["SigD"], ora["SigU"])
    cf["cost_iter"] = closed_form_cost(T, n, P["sets"], mu, D, U)
    cf["cost"] = closed_form_cost(T, n, P["sets"], cf["mu"], cf["D"], cf["U"])
    ora["accepted"], ora["step_cost"], ora["ntrials"] = chain.step()
    for d in (cf, ora):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cf, ora


def _add_sets(ctx, P, sets):
    n = P["n"]
    for s in sets:
        K = len(s["start"])
        if s["kind"] == "b":
            ctx.factors_add(2 * n, 3, s["start"], api.PSI_QUAD_PRIOR,
                            np.concatenate([s["Phi"].reshape(K, -1), s["Q"].reshape(K, -1)], 1), temperature=s["temp"])
        else:
            ctx.factors_add(n, 3, s["start"], api.PSI_FIXED_PRIOR,
                            np.concatenate([s["mu_u"], s["Kinv"].reshape(K, -1)], 1), temperature=s["temp"])


def _context(P, wave, options):
    ctx = api.Context(0)
    ctx.set_option("chain_wave", wave)
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.chain_set(P["T"], P["n"])
    _add_sets(ctx, P, P["sets"])
    return ctx


def _check_path(tag, P, cnt, on_load=True):
    """W and G rows assemble on load through the set loop, never the dense path; F rows and assemble_on_load 0 in no chain launch"""
    if P["on_load"] and on_load:
        assert cnt[0] == 0 and cnt[1] >= 1, (tag, cnt)
    else:
        assert cnt == (0, 0), (tag, cnt)


def _check_gradients(tag, row, gr, gA):
    """g, V_D, V_U, dmu of state B against both references, the structural zeros, and far from state A's"""
    P = _problem(row)
    binary = any(s["kind"] == "b" for s in P["sets"])
    for rname, ref in zip(("closed form", "oracle"), _references(row)):
        for k in ("g", "VD", "VU", "dmu") if binary else ("g", "VD", "dmu"):
            _hold(f"{tag} {k} vs {rname}", rel(gr[k], ref[k]), TIGHT)
    coupled = np.zeros(P["T"] - 1, dtype=bool)                    # V_U[t] of a pair no binary factor couples is exactly zero
    for s in P["sets"]:
        if s["kind"] == "b":
            coupled[s["start"]] = True
    assert (gr["VU"][~coupled] == 0.0).all()
    assert far_at_every_node(gr["g"], gA, P["T"]) > 1e-3


def test_rows_are_well_conditioned_and_the_references_agree():
    """No GPU.  Every row's dense V is positive definite with condition <= 1e4, its first trial is accepted (so S2's trial is
    the step's), and the two references differ by less than TIGHT / 5 in g, V_D, V_U and dmu (the figures of the docstring)."""
    gap = dict(g=0.0, VD=0.0, VU=0.0, dmu=0.0, cost=0.0)
    for row in ROWS:
        cf, ora = _references(row)
        V = o.bt_to_dense(cf["VD"], cf["VU"])
        assert np.linalg.eigvalsh(V).min() > 0.0, row
        print(f"    {row}: cond(V) = {cf['cond']:.3g}, oracle step {ora['accepted']} after {ora['ntrials']} trial(s)")
        assert cf["cond"] <= COND_MAX, (row, cf["cond"])
        assert ora["accepted"] and ora["ntrials"] == 1, row
        assert ora["step_cost"] == ora["cost"] and cf["cost"] < cf["cost_iter"], row
        for k in ("g", "VD", "VU", "dmu"):
            gap[k] = max(gap[k], rel(ora[k], cf[k]))
        for k in ("cost_iter", "cost"):
            gap["cost"] = max(gap["cost"], abs(ora[k] - cf[k]) / abs(cf[k]))
    print("    oracle vs closed form, largest over the rows:", {k: f"{v:.2e}" for k, v in gap.items()})
    for k, v in gap.items():
        assert v < TIGHT / 5, (k, v)


@gpu
@pytest.mark.parametrize("row,wave", CASES, ids=IDS)
def test_set_loop_assemble_on_load_vs_oracle_and_closed_form(row, wave):
    """S1, S2 and S3 with every switch on, on state A and then on state B of one context: W and G rows assemble through the
    set loop, F rows in a launch of their own, and state B's results agree with both references."""
    P = _problem(row)
    cf, ora = _references(row)
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
        _check_path(tag, P, cnt)
    _check_gradients("S1", row, gr1, g1A)
    _check_gradients("S2", row, gr2, g2A)
    for k in ("g", "VD", "VU"):                                   # the same ordered sums of the same per-factor results
        assert np.array_equal(gr1[k], gr2[k]), k
    _hold("D vs D_B + step (V_dev - D_B)", rel(st["D"], DB + STEP * (gr2["VD"] - DB)), 1e-14)
    _hold("U vs U_B + step (V_dev - U_B)", rel(st["U"], UB + STEP * (gr2["VU"] - UB)), 1e-14)
    for k in ("SigD", "SigU"):
        _hold(f"trial {k} vs oracle", rel(st[k], ora[k]), TIGHT)
    for rname, ref in (("closed form", cf), ("oracle", ora)):
        for k in ("D", "U", "mu"):
            _hold(f"accepted {k} vs {rname}", rel(st[k], ref[k]), TIGHT)
        for what, value, want in (("S2 trial cost", cost, ref["cost"]), ("S3 cost_iter", r3["cost_iter"], ref["cost_iter"]),
                                  ("S3 new_cost", r3["new_cost"], ref["cost"])):
            _hold(f"{what} vs {rname}", abs(value - want) / abs(want), TIGHT)
        assert r3["accepted"] == (ref["cost"] < ref["cost_iter"]), (rname, r3)
    assert r3["accepted"] == ora["accepted"] and r3["ntrials"] == ora["ntrials"], (r3, ora["ntrials"])


def _s2_a_then_b(P, wave, options):
    ctx = _context(P, wave, options)
    try:
        ctx.ngd_init(*P["A"])
        grA, _, _ = _s2(ctx)
        ctx.ngd_init(*P["B"])
        (gr, st, cost), counts = _counted(_s2, ctx)
    finally:
        _restore(ctx)
    return gr, st, cost, grA["g"], counts


@gpu
@pytest.mark.parametrize("row,wave", CASES, ids=IDS)
def test_on_load_sums_equal_the_csr_kernel_bit_for_bit(row, wave):
    """S2 under assemble_on_load 1 and 0, each in a fresh context: g, V_D, V_U, dmu, the accepted state and the trial cost are
    equal bit for bit -- the set loops keep bt_scatter_all_kernel's order, also for repeated and unsorted starts -- and under
    assemble_on_load 0 no chain launch assembles."""
    P = _problem(row)
    gr0, st0, cost0, gA0, cnt0 = _s2_a_then_b(P, wave, ALL_ON)
    _check_path("all on", P, cnt0)
    _check_gradients("all on", row, gr0, gA0)
    gr, st, cost, _, cnt = _s2_a_then_b(P, wave, {**ALL_ON, "assemble_on_load": 0})
    _check_path("assemble_on_load 0", P, cnt, on_load=False)
    for k in ("g", "VD", "VU", "dmu"):
        assert np.array_equal(gr[k], gr0[k]), k
    assert set(st) == set(st0)
    for k in st:
        assert np.array_equal(st[k], st0[k]), k
    assert cost == cost0, (cost, cost0)


@gpu
def test_a_ninth_set_is_refused_and_eight_still_work():
    """W5's eight sets and one more: the resident iteration refuses with GVI_ERR_UNSUPPORTED; the same context, set up again
    without the ninth, gives W5's numbers."""
    P = _problem("W5")
    assert len(P["sets"]) == MAX_SETS
    ctx = _context(P, 1, ALL_ON)
    try:
        _add_sets(ctx, P, P["sets"][1:2])                         # a ninth: the full unary set once more
        with pytest.raises(api.GviError) as e:
            ctx.ngd_init(*P["B"])
            ctx.ngd_step(0.55, 10)
        assert e.value.status == GVI_ERR_UNSUPPORTED and "more than 8 factor sets" in str(e.value), str(e.value)
        ctx.chain_set(P["T"], P["n"])
        _add_sets(ctx, P, P["sets"])
        ctx.ngd_init(*P["A"])
        gA = _s1(ctx)["g"]
        ctx.ngd_init(*P["B"])
        gr, cnt = _counted(_s1, ctx)
    finally:
        _restore(ctx)
    _check_path("eight sets", P, cnt)
    _check_gradients("eight sets", "W5", gr, gA)
