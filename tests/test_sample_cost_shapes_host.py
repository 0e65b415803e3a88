"""CPU checks of tests/sample_cost_ref.py: the references of tests/test_sample_cost_shapes_gpu.py agree with each other far
inside that module's bound, the inputs are what the rows claim (magnitudes positive, indefinite sets of both signs), the case
tables reach every launch geometry they are there for, and the restated reduction order is the documented one."""
import math

import numpy as np
import pytest

import sample_cost_ref as R


@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_against_the_longdouble_form(name):
    """At most 1e-13 of mag per entry, on every sum-of-squares set of every row: the float64 reference alone sits 100x inside
    the device bound of 1e-11."""
    c = R.case(name)
    assert any("mag" in r for r in R.references(name))
    for i, (sp, r) in enumerate(zip(c["specs"], R.references(name))):
        if "mag" not in r:                                                    # a hinge set, or the empty set of the P rows
            continue
        assert r["cost"].shape == (c["S"], len(sp["start"])) == r["mag"].shape
        assert (r["mag"] > 0).all(), (name, i)
        err = float((np.abs(r["cost"].astype(np.longdouble) - r["ld"]) / r["mag"]).max())
        print(f"{name}: set {i} kind {sp['kind']} d {sp['d']}: oracle vs longdouble {err:.3e} of mag")
        assert err <= 1e-13, (name, i, err)
        assert (np.abs(r["cost"]) <= r["mag"] * (1 + 1e-12)).all()            # mag bounds the form term by term


@pytest.mark.parametrize("n", R.G_INDEFINITE)
def test_indefinite_rows_have_costs_of_both_signs(n):
    c = R.case(f"G{n}")
    sp, r = c["specs"][0], R.references(f"G{n}")[0]
    ev = np.linalg.eigvalsh(sp["Qinv"])
    assert sp["indefinite"] and (ev.min(axis=1) < 0).all() and (ev.max(axis=1) > 0).all()
    both = ((r["cost"] < 0).any(axis=0) & (r["cost"] > 0).any(axis=0)).mean()
    print(f"G{n}: share of factors with costs of both signs over the samples {both:.3f}")
    assert both >= 0.25, both


def test_every_other_set_is_positive_definite():
    for name in R.SUMSQ_NAMES:
        for sp in R.case(name)["specs"]:
            if not sp["indefinite"]:
                assert (np.linalg.eigvalsh(sp["Qinv"] if sp["kind"] == R.QUAD else sp["Kinv"]) > 0).all(), name


def _sumsq_sets(names):
    return [(name, L, g) for name in names for L in R.launches(R.case(name)) for g in L["sets"] if g["kind"] in R.SUMSQ]


def test_the_tables_reach_every_geometry():
    sets = _sumsq_sets(R.NAMES)
    assert {g["P"] for _, _, g in sets} == {1, 2, 4, 8, 16, 32}
    assert {g["m"] for _, _, g in sets} >= set(range(1, 17)) | {18, 24, 32}
    assert {g["m"] for _, _, g in _sumsq_sets(R.W_NAMES)} == {2, 4, 6, 10, 16, 18, 24, 32}
    assert {L["NM"] for _, L, _ in sets} == {4, 8, 12, 16, 24, 32}
    assert {g["body"] for _, L, g in sets if g["body"] != L["NM"]} == {4, 6, 8, 12, 16}
    assert {g["body"] for _, L, g in sets if g["body"] == L["NM"]} == {4, 8, 12, 16, 24, 32}
    assert {g["ftiles"] for _, _, g in sets} == {1, 2, 3}
    for P in (1, 2, 4, 8, 16, 32):                 # per row group: three tiles with ONE factor in the last, all four waves live
        assert any(g["P"] == P and g["ftiles"] == 3 and g["last_tile"] == 1 and g["waves"] == [0, 1, 2, 3] for _, _, g in sets), P
    assert any(1 < g["last_tile"] < g["F"] and g["ftiles"] > 1 for _, _, g in sets)      # a last tile partly filled
    chunked = {(g["schunk"], g["last"] < g["schunk"]) for _, _, g in sets}
    assert chunked >= {(1, False), (2, False), (2, True), (3, True)}
    assert any(g["schunk"] > 1 and g["ftiles"] > 1 for _, _, g in sets)                 # blk % ftiles and blk // ftiles both move


def test_the_g_rows_are_the_shapes_of_the_issue():
    for n in R.G_N:
        c = R.case(f"G{n}")
        assert c["T"] == {1: 514, 2: 258, 3: 130, 4: 130}.get(n, 66 if n <= 8 else 34) == 2 * R.tile(n) + 2 and c["S"] == 5
        q, f = c["specs"][:2]
        assert (q["kind"], q["d"], len(q["start"])) == (R.QUAD, 2 * n, c["T"] - 1) and (f["kind"], f["d"], len(f["start"])) == (R.FIXED, n, c["T"])
        assert q["indefinite"] == (n in R.G_INDEFINITE) and len(c["specs"]) == (3 if n in R.G_DESCENDING else 2)
        assert ((q["temperature"] >= 0.5) & (q["temperature"] <= 2.0)).all() and np.unique(q["temperature"]).size == len(q["start"])
    for n in R.G_DESCENDING:
        s = R.case(f"G{n}")["specs"][2]["start"]
        assert (np.diff(s) <= 0).all() and (np.diff(s) == 0).sum() == 1 and (np.diff(s) == -2).sum() == 1
    for n in R.G_UNARY_ONLY:
        (L,) = R.launches(R.case(f"G{n}u"))[:1]
        assert [(g["d"], g["body"]) for g in L["sets"]] == [(n, L["NM"])]
    assert R.case(f"G{R.G_CLOSED}cf")["closed_form"]


def test_the_c_rows_chunk_as_the_issue_states():
    for name, (schunk, last) in R.C_EXPECT.items():
        c = R.case(name)
        total = R.launches(c)[0]
        assert [(g["schunk"], g["last"]) for g in total["sets"]] == [(schunk, last)] * len(c["specs"]), name
        for a, b in R.windows(name):
            assert 0 <= a < b <= c["S"] and b - a <= 64
        (a0, b0), (a1, b1), (a2, b2) = R.windows(name)
        assert (a0, b0) == (0, schunk) and a1 % schunk == schunk - 1 and b1 - a1 > schunk and b2 == c["S"] and a2 % schunk == 0
    assert [g["ftiles"] for g in R.launches(R.case("C6_1025"))[0]["sets"]] == [2, 2]
    assert [g["ftiles"] for g in R.launches(R.case("C1_1400"))[0]["sets"]] == [3]


def test_the_r_and_p_rows():
    off_grid = 0
    for kt in R.R_KT:
        c = R.case(f"R{kt}")
        Ks = [len(sp["start"]) for sp in c["specs"]]
        assert sum(Ks) == kt and c["n"] in (1, 2)
        off_grid += len(Ks) >= 2 and all(b % 256 for b in np.cumsum(Ks)[:-1])
    assert off_grid >= 2
    h = R.case("Rhinge")
    assert (h["specs"][1]["kind"], h["specs"][1]["d"], len(h["specs"][1]["start"]), h["T"], h["n"]) == (R.HINGE, 2, 300, 300, 2)
    psi = R.references("Rhinge")[1]["cost"]
    assert 0.03 <= (psi > 0).mean() <= 0.97                                            # both hinge branches
    for s in R.P_S:
        c = R.case(f"P{s}")
        assert [(sp["kind"], len(sp["start"])) for sp in c["specs"]] == [(R.HINGE, 3), (R.FIXED, 4), (R.FIXED, 0), (R.QUAD, 3), (R.HINGE, 1)]
        assert list(c["specs"][0]["start"]) == [0, 2, 3] and (c["T"], c["n"], c["S"]) == (4, 2, s)
    blocks = {g["blocks"] for s in R.P_S for g in R.launches(R.case(f"P{s}"))[0]["sets"] if g["kind"] == R.HINGE}
    assert blocks >= {1, 2, 4}                                                         # the point body in one block and in several


def test_geometry_of_known_launches():
    """The restatement on shapes worked out by hand from run_sample_cost."""
    g = R.geometry([(R.QUAD, 12, 1024), (R.FIXED, 6, 1025)], 1024)                     # the benchmark's chain at S = 1024
    q, f = g["sets"]
    assert g["NM"] == 12 and (q["P"], q["F"], q["ftiles"], q["schunk"], q["blocks"], q["body"]) == (8, 32, 32, 16, 32 * 64, 12)
    assert (f["ftiles"], f["schunk"], f["chunks"], f["blocks"], f["body"], f["boff"]) == (33, 17, 61, 33 * 61, 6, 2048) and g["blocks"] == 4061
    g = R.geometry([(R.HINGE, 2, 3), (R.FIXED, 2, 0), (R.FIXED, 4, 5)], 100)
    assert [s["blocks"] for s in g["sets"]] == [2, 100] and g["NM"] == 4 and g["sets"][1]["boff"] == 2
    assert [R.tile(m) for m in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [256, 128, 64, 64, 32, 32, 16, 16, 8, 8]


def test_ordered_sum_is_the_documented_order():
    # Kt = 3 by hand: the partial sums of threads 0, 1, 2 are the entries; the fold adds red[2] to red[0] at width 2, then red[1]
    # at width 1: (1e16 + -1e16) + 1 = 1, where left to right (1e16 + 1) + -1e16 = 0
    assert R.ordered_sum(np.array([[1e16, 1.0, -1e16]]))[0] == 1.0
    assert (1e16 + 1.0) + -1e16 == 0.0
    # Kt = 257: thread 0 adds entry 256 to entry 0 BEFORE the fold
    row = np.zeros((1, 257))
    row[0, 0], row[0, 128], row[0, 256] = 1e16, 1.0, -1e16
    assert R.ordered_sum(row)[0] == 1.0
    row[0, 256], row[0, 255] = 0.0, -1e16                                               # ... and entry 255 only at the last fold
    assert R.ordered_sum(row)[0] == 0.0
    rng = np.random.default_rng(5)
    for Kt in (1, 2, 255, 256, 257, 513, 1000):
        M = rng.uniform(0.1, 3.0, size=(4, Kt)) * rng.choice([-1.0, 1.0], size=(4, Kt))
        got = R.ordered_sum(M)
        for s in range(4):
            assert abs(got[s] - math.fsum(M[s])) <= 1e-13 * math.fsum(np.abs(M[s])), (Kt, s)
    nan = np.ones((3, 300))
    nan[1, 290] = np.nan
    assert np.array_equal(np.isnan(R.ordered_sum(nan)), [False, True, False])
