"""CPU side of the spectral-stage tests: the input classes are what their names claim, and the float64 restatements the GPU
module (tests/test_spectral_prep_gpu.py) compares the device with are themselves held to 50-digit references (mpmath).  The
whole module is skipped where mpmath is not installed; the GPU module does not need it, it reads the recorded errors from
tests/golden/spectral_ref_err.json, which this module re-derives number by number."""
import json

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")

import spectral_ref as sp  # noqa: E402


@pytest.mark.parametrize("d", sp.D_ALL)
def test_every_class_is_spd_with_the_spectrum_it_claims(d):
    cases = sp.sigma_cases(d, np.random.default_rng(100 + d))
    assert tuple(cases) == sp.classes_of(d) and (d == 1 or tuple(cases) == sp.CLASSES)
    for name, S in cases.items():
        assert S.shape == (d, d) and np.array_equal(S, S.T), name
        lam = np.linalg.eigvalsh(S)
        assert lam.min() > 0, (name, lam.min())
        want = sp.spectrum(name, d)
        if want is None:                                                 # near_diag: `diagonal` moved by at most |1e-9 E|_2
            assert np.abs(lam - sp.spectrum("diagonal", d)).max() < 1e-9 * 2 * np.sqrt(d) * 4
            off = S - np.diag(np.diag(S))
            assert 0 < np.abs(off).max() < 1e-8 and np.array_equal(np.diag(S), sp.spectrum("diagonal", d))
        else:
            assert np.abs(lam - np.sort(want)).max() < 1e-12 * want.max(), name      # (a symmetric solver is good to eps |Sigma|)
        if name in ("identity", "diagonal"):
            assert np.count_nonzero(S - np.diag(np.diag(S))) == 0
        if name == "clustered":
            assert np.all((np.abs(lam - 1.0) < 1e-12) | (np.abs(lam - 4.0) < 1e-12))
            assert (np.abs(lam - 1.0) < 1e-12).sum() == d // 2 and np.abs(S - np.diag(np.diag(S))).max() > (1e-3 if d > 2 else 0)


def test_the_recorded_file_covers_exactly_the_rows_of_the_gpu_module():
    import test_spectral_prep_gpu as g
    rows = g.NODE_ROWS + g.MOMENT_ROWS + g.JKO_ROWS
    keys = [sp.key(r) for r in rows]
    assert len(set(keys)) == len(keys) == len(sp.all_rows())
    with open(sp.ERR_FILE) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(keys)
    assert all(isinstance(v, float) and 0.0 <= v < 1e-6 for v in rec.values())


@pytest.fixture(scope="module")
def recomputed():
    return {sp.key(r): sp.ref_err(r) for r in sp.all_rows()}


def test_every_recorded_number_is_within_a_factor_two_of_its_recomputation(recomputed):
    """(a number that fell out of the factor is RAISED in the file, a bound is never lowered to fit; values under 1e-17 --
    an exact result -- count as 1e-17)"""
    rec = sp.recorded()
    bad = {k: (rec[k], v) for k, v in recomputed.items() if not 0.5 <= max(rec[k], 1e-17) / max(v, 1e-17) <= 2.0}
    assert not bad, bad


def test_the_jko_reference_alone_stays_inside_the_floor(recomputed):
    """32 x (float64 bw_jko against mpmath) <= 1e-8 on every JKO row, small h included: no such row passes or fails on the
    device because of the reference"""
    rec = sp.recorded()
    worst = max((max(rec[sp.key(r)], recomputed[sp.key(r)]), sp.key(r)) for r in sp.jko_rows())
    print(f"    worst JKO reference error {worst[0]:.2e} ({worst[1]})")
    assert sp.MARGIN * worst[0] <= 1e-8, worst


def test_no_jko_row_has_a_singular_step_matrix():
    """I - h S singular makes Sig_half singular, l (l + 4h) can round negative and both restatements give NaN: no row goes
    there.  With gap = min |1 - h lambda(S)| the smallest eigenvalue of Sig_half is >= gap^2 lambda_min(Sigma) >= 1e-10 * 1e-2,
    a hundred times the rounding eps |Sigma| = 1e-14 of forming it.  (The seeded data comes close once: unary d = 5, cond1e4,
    h = 0.55 has gap 1.7e-5 -- kept, it is the row with the widest spectrum of Sig_half.)"""
    for kind in ("u", "b"):
        for d in sp.JKO_D[kind]:
            for cls in sp.JKO_CLASSES:
                if cls in sp.classes_of(d):
                    lam = np.linalg.eigvalsh(sp.jko_case(kind, d, cls)["hess"])
                    gap = min(np.abs(1.0 - h * lam).min() for h in sp.H_ALL)
                    assert gap > 1e-5, (kind, d, cls, gap)


@pytest.mark.parametrize("h", sp.H_ALL)
@pytest.mark.parametrize("sigma,s", [(0.3, 1.7), (2.0, -0.4), (1e-2, 5.0), (1e2, 0.01)])
def test_the_map_in_one_dimension_is_its_closed_form(sigma, s, h):
    mp = sp._mp()
    got = sp.mp_jko(mp.matrix([[sigma]]), mp.matrix([[s]]), h)[0, 0]
    want = sp.jko_scalar(sigma, s, h)
    assert abs(got - want) <= mp.mpf(10) ** -40 * abs(want), (got, want)


def test_the_references_reproduce_their_inputs():
    """S S = Sigma to 1e-45 and, for the quadratic psi of the JKO rows, the oracle's S is the factor's Hessian"""
    mp = sp._mp()
    for d in (1, 5, 12):
        Sg = sp.operator_case(d)["Sigma"][0]
        S = sp.mp_sym_sqrt(Sg)
        R = S * S - mp.matrix(Sg.tolist())
        assert max(abs(R[i, j]) for i in range(d) for j in range(d)) < mp.mpf(10) ** -45
    for kind, d in (("u", 5), ("b", 12)):
        case = sp.jko_case(kind, d, "well")
        assert np.abs(sp.jko_oracle(case, 0.55)["S"] - case["hess"]).max() < 1e-10 * np.abs(case["hess"]).max()
