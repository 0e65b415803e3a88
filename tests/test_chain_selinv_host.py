"""The reference and the inputs of test_chain_selinv_gpu.py, proved on the CPU (no GPU mark).

  * the float64 recursion (chain_selinv_ref.selinv) against numpy's dense inverse and slogdet wherever T n <= 1600: 1e-13
    relative; measured here about 1e-15 (SD / SU) and at most 8.2e-15 (half log-det); the block solve used for the NGD rows likewise;
  * the longdouble path: eps < 1e-18 (1.08e-19 here) and agreement with mpmath at 40 digits on a small stiff chain;
  * conditioning: well cases at most 1e3 (measured about 17 to 41), stiff cases in [1e6, 1e8] (7.5e6 to 9.8e6);
  * the yardstick of the GPU bounds on the stiff chains: the float64 recursion against the longdouble one.  Measured here:
        (T, n)      cond      SD / SU deviation   in cond eps   half log-det (relative)
        (65, 2)    8.4e6          4.7e-11            0.02            7.3e-13
        (65, 3)    7.8e6          2.2e-11            0.01            6.2e-13
        (97, 4)    9.8e6          8.4e-10            0.39            2.4e-12
        (49, 6)    7.5e6          1.2e-10            0.07            1.5e-12
        (40, 8)    8.1e6          5.5e-09            3.04            7.5e-11
        (65, 11)   8.5e6          1.1e-09            0.57            1.1e-12
        (65, 12)   8.3e6          5.2e-09            2.85            1.3e-11
        (65, 16)   8.2e6          6.9e-09            3.78            2.0e-11
    maximum 3.8 cond eps and 7.5e-11, so the GPU test's 100 cond eps sits 26 times above the reference's own deviation and its
    log-det bound is 8 * 7.5e-11 = 6.0e-10;
  * the case table holds every pass count the issue asks for, and the not-positive-definite inputs are found out by the last
    pass only."""
import numpy as np
import pytest

import chain_pivot_ref as P
import chain_selinv_ref as R

EPS = np.finfo(np.float64).eps
DENSE = [(T, n) for T, n in R.WELL_CASES if T * n <= 1600]


def _ids(cases):
    return [f"T{T}-n{n}" for T, n in cases]


@pytest.mark.parametrize("T,n,stiff", [c + (False,) for c in DENSE] + [c + (True,) for c in R.STIFF_CASES],
                         ids=_ids(DENSE) + ["stiff-" + i for i in _ids(R.STIFF_CASES)])
def test_float64_recursion_against_the_dense_inverse(T, n, stiff):
    D, U = R.stiff_state(T, n) if stiff else R.state_b(T, n)
    SD, SU, hld = R.selinv(D, U) if stiff else R.reference(T, n)
    dSD, dSU, dhld = R.dense_selinv(D, U)
    err, eh = max(R.rel(SD, dSD), R.rel(SU, dSU)), abs(hld - dhld) / abs(dhld)
    print(f"selinv against the dense inverse T {T} n {n}: SD / SU {err:.2e}, half log-det {eh:.2e}")
    if stiff:                                                # both sides carry cond eps here: the longdouble test below decides
        assert err < 100 * R.stiff_reference(T, n)["cond"] * EPS
        return
    assert err < 1e-13 and eh < 1e-13
    rhs = np.random.default_rng(T + n).normal(size=(T, n))
    x = R.solve(D, U, rhs)
    assert R.rel(x.reshape(-1), np.linalg.solve(P.dense(D, U), rhs.reshape(-1))) < 1e-13


def test_longdouble_path_against_mpmath():
    import mpmath as mp
    assert np.finfo(np.longdouble).eps < 1e-18
    T, n = 5, 3
    D, U = R.stiff(T, n, 1)
    SD, SU, hld = R.selinv(D, U, np.longdouble)
    assert SD.dtype == np.longdouble and type(hld) == np.longdouble
    with mp.workdps(40):
        A = mp.matrix(P.dense(D, U).tolist())
        Ai, ld = A ** -1, mp.log(mp.det(A)) / 2
        cond = float(mp.norm(A, mp.inf) * mp.norm(Ai, mp.inf))
        err = max(abs(mp.mpf(str(np.format_float_scientific(v, precision=25, unique=False))) - Ai[t * n + i, u * n + j])
                  for M, off in ((SD, 0), (SU, 1)) for t in range(T - off) for u in (t + off,)
                  for i in range(n) for j in range(n) for v in (M[t, i, j],))
        scale = max(abs(Ai[i, j]) for i in range(T * n) for j in range(T * n))
        eh = abs(mp.mpf(str(np.format_float_scientific(hld, precision=25, unique=False))) - ld) / abs(ld)
    print(f"longdouble against mpmath: cond {cond:.2e}, SD / SU {float(err / scale):.2e}, half log-det {float(eh):.2e}")
    leps = float(np.finfo(np.longdouble).eps)
    assert cond > 1e5
    assert float(err / scale) < 100 * cond * leps and float(eh) < 100 * cond * leps


@pytest.mark.parametrize("T,n", R.WELL_CASES, ids=_ids(R.WELL_CASES))
def test_well_cases_are_well_conditioned(T, n):
    """bt_extreme_eigs where it is quick (T n <= 1600: it costs O((T n)^2)); the longer chains by what the generator guarantees
    and a block Gershgorin bound: every link is >= 0.3 I on its two nodes, so lambda_min >= 0.3 (0.6 at inner nodes), and
    lambda_max <= max_t (|D_t| + |U_t| + |U_{t-1}|) in the spectral norm."""
    D, U = R.state_b(T, n)
    assert np.array_equal(D, np.swapaxes(D, 1, 2)) and not np.array_equal(D, R.state_a(T, n)[0])
    if T * n <= 1600:
        from test_gpu_parity import bt_extreme_eigs
        lo, hi = bt_extreme_eigs(D, U)
    else:
        nU = np.concatenate([[0.0], np.linalg.norm(U, 2, axis=(1, 2)), [0.0]])
        lo, hi = 0.3, (np.linalg.norm(D, 2, axis=(1, 2)) + nU[:-1] + nU[1:]).max()
    assert lo > 0 and hi / lo <= 1e3, (lo, hi)


def test_stiff_cases_and_the_float64_yardstick():
    worst, worst_h = 0.0, 0.0
    for T, n in R.STIFF_CASES:
        r = R.stiff_reference(T, n)
        units = r["dev"] / (r["cond"] * EPS)
        print(f"stiff T {T} n {n} N {R.padded(n)}: cond {r['cond']:.2e}, float64 recursion against longdouble: SD / SU {r['dev']:.2e} = "
              f"{units:.2f} cond eps, half log-det {r['dev_hld']:.2e}")
        assert 1e6 <= r["cond"] <= 1e8
        worst, worst_h = max(worst, units), max(worst_h, r["dev_hld"])
    assert worst_h == R.stiff_logdet_yardstick()
    assert worst <= 100 / 5 and worst_h < 1e-9 / 8           # the GPU bounds stay 5 times above the reference and below TIGHT


def test_case_table_holds_every_pass_count():
    counts = {}
    for T, n in R.WELL_CASES:
        counts.setdefault(R.padded(n), set()).add(len(R.chain_passes(T, n)))
    assert all(counts[N] >= {1, 2, 3, 4} for N in (6, 8, 12, 16)), counts
    assert all(counts[N] >= {1, 2, 3} for N in (1, 2, 3, 4)), counts
    assert R.chain_passes(49153, 6) == [(0, 5, False), (5, 5, False), (10, 5, False), (15, 1, True)]
    assert len(R.chain_passes(49152, 6)) == 3 and len(R.chain_passes(512, 12)) == 3 and len(R.chain_passes(513, 16)) == 4
    for n, T in ((9, 130), (11, 130), (13, 130), (7, 385)):
        assert (T, n) in R.WELL_CASES and R.padded(n) > n and len(R.chain_passes(T, n)) == 3
    assert max(T for T, _ in R.WELL_CASES) <= 50000 and len(set(R.WELL_CASES)) == len(R.WELL_CASES)
    assert sorted(R.padded(n) for _, n in R.SCALE_CASES) == list(P.PADDED)
    assert all(len(R.chain_passes(T, n)) == max(counts[R.padded(n)]) for T, n in R.SCALE_CASES)
    assert sorted(R.padded(n) for _, n in R.NOT_PD_CASES) == list(P.PADDED)
    assert all((T, n) in R.WELL_CASES for T, n in R.NOT_PD_CASES)


@pytest.mark.parametrize("T,n", R.NOT_PD_CASES, ids=_ids(R.NOT_PD_CASES))
def test_not_pd_state_is_found_out_by_the_last_pass_only(T, n):
    D, U, e, h, (c_lo, c, c_hi) = R.not_pd_state(T, n)
    passes = R.chain_passes(T, n)
    last = len(passes) - 1
    bad = R.cr_not_pd_nodes(D, U)
    print(f"not-pd T {T} n {n}: node {e} - {c:.4f} I (positive definite up to {c_lo:.4f}, without node {h} up to {c_hi:.4f}); "
          f"non-positive pivots at nodes {bad}")
    assert len(passes) >= 3 and R.pass_of(R.node_level(e, T), passes) == 0
    assert c_hi - c_lo > 1e-6 * c                            # a margin no rounding crosses
    assert bad and e not in bad and all(R.pass_of(R.node_level(b, T), passes) == last for b in bad)
    assert np.linalg.eigvalsh(D[e]).min() > 0
    assert np.isnan(R.selinv(D, U)[2])                       # and the recursion says so too
    assert R.cr_not_pd_nodes(*R.state_b(T, n)) == []
