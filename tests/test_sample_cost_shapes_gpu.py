"""Costs of sampled trajectories at the shapes where the launch geometry of kernels_sample_cost.hpp does something: more than
one factor tile (blk % ftiles against blk // ftiles, all four waves, a last tile partly filled), more than one sample chunk
with a partial last one, every row group P = 1 ... 32 and every m = 1 ... 16, every NM instance and half-width body, indefinite
Qinv, Kt up to 513 in the reduction, the point body over several blocks, and a set list that starts with a hinge set and has
an empty set in the middle.  The rows, inputs and references are tests/sample_cost_ref.py; tests/test_sample_cost_shapes_host.py
proves on the CPU that they reach those geometries and that the float64 reference is within 1e-13 of mag of a longdouble one.

Bounds.  Sum-of-squares sets: |got - ref| <= 1e-11 mag entry by entry, mag[s, k] = (|x1| + |Phi| |x0|)^T |Qinv| (...) / T_k from
the public parameters (a max-norm over the matrix hides one wrong small column), and the max-norm 1e-11 of
tests/test_sample_cost_gpu.py.  1e-11 is the project's bound for these kinds; a d-term fma dot product plus an m-term sum of
squares is off by less than 70 units of roundoff of mag, about 8e-15.  Hinge sets: 1e-8 for cost and clearance.  J is
np.array_equal to the restated reduction order (sample_cost_ref.ordered_sum) of the single-set matrices side by side: the
single-set call forms each entry with the operations of the total call, only ld and the column offset differ.

gvi_factors_add takes the K = 0 set of the P rows, so it stays in the list.

The minimum clearance has no entry point that takes the caller's X: it is reached through gvi_ngd_sample_costs alone, whose
samples the device draws.  So clr_min is held bit for bit to the row minimum of sample_clearance on the resident samples
(Kc = 300: the strided loop takes its second step), and the two NaN placements are asserted where a caller's X can put them:
on sample_clearance (NaN at exactly that entry, so its row minimum is NaN for exactly that sample) and on J.

Sensitivity, recorded once on an MI355X (profiles/sample_cost_shapes.txt): each edit below was applied to a copy of the
sources, and this module and tests/test_sample_cost_gpu.py (without its shim test, which links the in-tree library) were run
beside the edited library.  "costs" is test_costs_entry_by_entry_and_the_ordered_total, "chunks" is
test_chunking_changes_no_arithmetic; the summary test fails with any sum-of-squares row.
  1 k formed without the `wave` term: costs fails on every G and W row, C6_1025, C1_684, C1_1400, R255, R256, R257, R513 and
    Rhinge (every row with a live factor beyond wave 0), chunks on the three C rows of those, both resident tests.  The sibling
    fails on c3mini only (4 of 31 tests: its unary set of 9 factors reaches wave 1).
  2 ft and sc swapped: everything fails but costs[P1] (S = 1, one tile: block 0 either way).  The sibling fails too (25 of 31):
    with one tile, blk / 1 makes every chunk a tile.
  3 the store using s0 for s: costs and chunks fail on all five C rows and on nothing else.  Of the sibling only the
    statistical test at S = 2^14 fails; every exact check of it passes.
  4 the J loop striding by 255: costs fails on G1, G2, G3, G4, W1, C1_684, C1_1400, R256, R257, R513 and Rhinge -- the rows
    with Kt >= 256; Kt = 1 and 255 pass, as they must -- and the resident row on 513 columns.  The sibling passes.
  5 koff advanced before cp is taken: NOT run as written -- the last set's columns would start at column Kt, so the last
    sample's row is written past the end of the matrix.  Its in-bounds stand-in was run instead: the sets' columns laid out in
    reverse order (cp = cost + ld - koff after the advance; a single-set call is unchanged).  costs fails through the J check
    on 23 of the 28 rows with two or more sets (G2, G4, G13, R256 and P1 pass: a permutation of the columns changes J only
    where the rounding of the sum happens to differ), and the resident row fails.  The sibling passes.
"""
import functools

import numpy as np
import pytest

import sample_cost_ref as R
from gaussianvi_amd import api
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu
SUMSQ_BOUND, HINGE_BOUND = 1e-11, 1e-8


def context(name):
    c = R.case(name)
    ctx = api.Context(0)
    ctx.chain_set(c["T"], c["n"])
    ids = []
    for sp in c["specs"]:
        ids.append(ctx.factors_add(sp["d"], sp["p"], sp["start"], sp["kind"], sp["params"], sp["temperature"]))
        if sp["kind"] == R.HINGE:
            ctx.factors_set_sdf2d(ids[-1], sp["sdf_origin"], sp["sdf_cell"], sp["sdf_field"])
        elif c["closed_form"]:
            ctx.factors_set_closed_form(ids[-1], True)
    return ctx, ids


@functools.lru_cache(maxsize=None)
def device(name):
    """(per-set cost matrices, per-set clearance matrices or None, J) of the row, each operator called TWICE: the second call
    must give the same words.  Computed once, read-only."""
    c = R.case(name)
    ctx, ids = context(name)
    costs, clrs = [], []
    for sid, sp in zip(ids, c["specs"]):
        costs.append(ctx.sample_factor_costs(sid, c["X"]))
        assert np.array_equal(costs[-1], ctx.sample_factor_costs(sid, c["X"]), equal_nan=True), (name, sid)
        clrs.append(ctx.sample_clearance(sid, c["X"]) if sp["kind"] == R.HINGE else None)
        if clrs[-1] is not None:
            assert np.array_equal(clrs[-1], ctx.sample_clearance(sid, c["X"]), equal_nan=True), (name, sid)
    J = ctx.sample_costs(c["X"])
    assert np.array_equal(J, ctx.sample_costs(c["X"]), equal_nan=True), name
    ctx.close()
    for a in costs + [k for k in clrs if k is not None] + [J]:
        a.setflags(write=False)
    return costs, clrs, J


def entry_error(got, r):
    """max over the entries of |got - ref| / mag"""
    return float((np.abs(got - r["cost"]) / r["mag"]).max())


@pytest.mark.parametrize("name", R.NAMES)
def test_costs_entry_by_entry_and_the_ordered_total(name):
    c = R.case(name)
    costs, clrs, J = device(name)
    for i, (sp, r, got, clr) in enumerate(zip(c["specs"], R.references(name), costs, clrs)):
        K = len(sp["start"])
        assert got.shape == (c["S"], K) == r["cost"].shape
        if K == 0:
            continue
        g = R.geometry([(sp["kind"], sp["d"], K)], c["S"])
        if sp["kind"] in R.SUMSQ:
            err, mx = entry_error(got, r), rel(got, r["cost"])
            s = g["sets"][0]
            print(f"{name}: set {i} kind {sp['kind']} d {sp['d']} K {K}: P {s['P']} NM {g['NM']} body {s['body']} ftiles {s['ftiles']} "
                  f"schunk {s['schunk']}: worst |err| / mag {err:.3e}, max-norm {mx:.3e}")
            assert np.isfinite(got).all() and np.abs(r["cost"]).max() > 0
            assert (np.abs(got - r["cost"]) <= SUMSQ_BOUND * r["mag"]).all(), (name, i, err)
            assert mx <= SUMSQ_BOUND, (name, i, mx)
        else:
            e_cost, e_clr = rel(got, r["cost"]), rel(clr, r["clr"])
            print(f"{name}: set {i} hinge K {K} blocks {g['blocks']}: cost error {e_cost:.3e}, clearance error {e_clr:.3e}")
            assert e_cost <= HINGE_BOUND and e_clr <= HINGE_BOUND, (name, i, e_cost, e_clr)
    want = R.ordered_sum(np.concatenate(costs, axis=1))
    total = R.launches(c)[0]
    print(f"{name}: Kt {sum(m.shape[1] for m in costs)}, launch NM {total['NM']} blocks {total['blocks']}: J differs from the ordered sum in "
          f"{int((J != want).sum())} of {c['S']} samples")
    assert np.array_equal(J, want), name


@pytest.mark.parametrize("name", R.C_NAMES)
def test_chunking_changes_no_arithmetic(name):
    """Rows [a, b) of the large call are the call on X[a:b] alone, bit for bit, in the first chunk, across a chunk boundary and
    in the last chunk."""
    c = R.case(name)
    costs, _, J = device(name)
    ctx, ids = context(name)
    for a, b in R.windows(name):
        Xw = np.ascontiguousarray(c["X"][a:b])
        for sid, big in zip(ids, costs):
            small = ctx.sample_factor_costs(sid, Xw)
            print(f"{name}: window [{a}, {b}) set {sid}: {int((small != big[a:b]).sum())} entries differ")
            assert np.array_equal(small, big[a:b]), (name, a, b, sid)
        assert np.array_equal(ctx.sample_costs(Xw), J[a:b]), (name, a, b)
    ctx.close()


def test_minimum_clearance_and_nan_placements():
    """Rhinge: a QUAD_PRIOR set of 299 factors, then the HINGE_SDF_2D set of 300 (columns 299 ... 598 of the cost row)."""
    name = "Rhinge"
    c = R.case(name)
    costs, clrs, J = device(name)
    ctx, ids = context(name)
    T, n, S = c["T"], c["n"], c["S"]
    for s, k in zip((4, 6), R.R_NAN_FACTORS):
        state = int(c["specs"][1]["start"][k])
        Xb = c["X"].copy()
        Xb[s, state, 1] = np.nan
        clr = ctx.sample_clearance(ids[1], Xb)
        bad = np.zeros(clr.shape, dtype=bool)
        bad[s, k] = True
        assert np.isnan(clr[bad]).all() and np.array_equal(clr[~bad], clrs[1][~bad]), (s, k)
        assert np.array_equal(np.isnan(clr.min(axis=1)), np.arange(S) == s)
        cost = ctx.sample_factor_costs(ids[1], Xb)
        assert np.isnan(cost[bad]).all() and np.array_equal(cost[~bad], costs[1][~bad]), (s, k)
        prior = ctx.sample_factor_costs(ids[0], Xb)                    # the binary factors that end at or start from that state
        touched = np.zeros(prior.shape, dtype=bool)
        touched[s, [j for j in (state - 1, state) if 0 <= j < prior.shape[1]]] = True
        assert np.isnan(prior[touched]).all() and np.array_equal(prior[~touched], costs[0][~touched]), (s, k)
        Jb = ctx.sample_costs(Xb)
        print(f"NaN in state {state} of sample {s}: clearance NaN at {np.argwhere(np.isnan(clr)).tolist()}, J NaN at {np.flatnonzero(np.isnan(Jb)).tolist()}")
        assert np.isnan(Jb[s]) and np.array_equal(np.delete(Jb, s), np.delete(J, s)), (s, k)
    # the resident call: clr_min over Kc = 300 columns, J over Kt = 599
    rng = np.random.default_rng(77)
    ctx.ngd_init(rng.uniform(-3.0, 3.0, size=(T, n)), np.stack([4.0 * np.eye(n)] * T), 0.3 * rng.normal(size=(T - 1, n, n)))
    r = ctx.ngd_sample_costs(S, seed=5, clearance_set=ids[1])
    clr = ctx.sample_clearance(ids[1], r["X"])
    print(f"resident: clr_min differs from the row minimum in {int((r['clr_min'] != clr.min(axis=1)).sum())} of {S} samples; "
          f"minimum at columns {clr.argmin(axis=1).tolist()}")
    assert np.isfinite(clr).all() and np.array_equal(r["clr_min"], clr.min(axis=1))
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    r2 = ctx.ngd_sample_costs(S, seed=5, clearance_set=ids[1])
    assert all(np.array_equal(r[k], r2[k]) for k in ("X", "J", "logq", "clr_min"))
    ctx.close()


def test_resident_row_on_513_columns():
    c = R.case("R513")
    ctx, ids = context("R513")
    T, n = c["T"], c["n"]
    rng = np.random.default_rng(78)
    ctx.ngd_init(rng.normal(size=(T, n)), np.stack([2.0 * np.eye(n)] * T), 0.3 * rng.normal(size=(T - 1, n, n)) / np.sqrt(n))
    r = ctx.ngd_sample_costs(7, seed=11)
    assert np.isfinite(r["X"]).all() and np.isfinite(r["J"]).all()
    assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    want = R.ordered_sum(np.concatenate([ctx.sample_factor_costs(sid, r["X"]) for sid in ids], axis=1))
    print(f"resident, Kt 513: J differs from the ordered sum in {int((r['J'] != want).sum())} of 7 samples")
    assert np.array_equal(r["J"], want)
    r2 = ctx.ngd_sample_costs(7, seed=11)
    assert np.array_equal(r["J"], r2["J"]) and np.array_equal(r["X"], r2["X"])
    ctx.close()


def test_worst_errors_per_row_group_and_instance():
    """The figures of profiles/sample_cost_shapes.txt: the worst |err| / mag per P and per NM over every sum-of-squares row."""
    by_P, by_NM = {}, {}
    for name in R.SUMSQ_NAMES:
        c = R.case(name)
        costs = device(name)[0]
        for sp, r, got in zip(c["specs"], R.references(name), costs):
            g = R.geometry([(sp["kind"], sp["d"], len(sp["start"]))], c["S"])
            err = entry_error(got, r)
            by_P[g["sets"][0]["P"]] = max(by_P.get(g["sets"][0]["P"], 0.0), err)
            by_NM[g["NM"]] = max(by_NM.get(g["NM"], 0.0), err)
    print("worst |err| / mag per P:  " + ", ".join(f"P {P}: {e:.3e}" for P, e in sorted(by_P.items())))
    print("worst |err| / mag per NM: " + ", ".join(f"NM {w}: {e:.3e}" for w, e in sorted(by_NM.items())))
    assert sorted(by_P) == [1, 2, 4, 8, 16, 32] and sorted(by_NM) == list(R.NM_STEPS)
    assert max(by_P.values()) <= SUMSQ_BOUND
