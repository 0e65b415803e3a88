"""The factorisation half of the chain kernels -- half log-determinant and, with need_back, the selected inverse SigD / SigU -- at
every compiled block size and on pass plans of one to four passes, against a reference that shares no algorithm with them
(chain_selinv_ref.selinv, proved on the CPU by test_chain_selinv_host.py), through api.Context only (-m gpu).

Well-conditioned chains (chain_selinv_ref.WELL_CASES: condition 17 to 41 measured where T n <= 1600, bounded by 1e3 from the
generator's structure on the longer ones -- test_chain_selinv_host.py), per case in ONE context, after bt_marginals and
bt_logdet of another positive definite state of the shape:
  * SD, SU against the float64 recursion at TIGHT = 1e-9 and bt_logdet at rtol 1e-12 (test_bt_ops_vs_oracle's bounds);
  * SD[t] symmetric to 1e-13 of its scale;
  * a second call gives the same words; bt_logdet alone (need_back 0) gives the word that the factorisation WITH the selected
    inverse leaves for the cost (read through ngd_init + ngd_cost of the same context: no factor sets, cost = 0 + half log-det);
  * plans of two or more passes: chain_merge 1, 0, 1 bit for bit; n = 5, 6: chain_pair 1 and 0 bit for bit; n <= 2, T <= 65:
    chain_wave 1 and 0 against the reference and against each other at 1e-13.
Power-of-two scaling (SCALE_CASES: per padded N the deepest plan, on padded blocks), 2^k with k = +-40 and +-300: the marginals
are the unscaled words times 2^-k and the half log-det moves by T n k ln2 / 2 (1e-12 relative) -- at k = +-300 a plain product
of pivots overflows or underflows after a handful of nodes.
Not positive definite (NOT_PD_CASES): c I subtracted from a first-pass node so that only the last pass meets a non-positive
pivot: bt_logdet is NaN, the call returns, and the positive definite state gives its earlier word afterwards.
Stiff chains (STIFF_CASES, condition 7.5e6 to 9.8e6) against the LONGDOUBLE recursion: SD / SU within 100 cond eps
(test_c3_literal_chain_operator_parity's form; the float64 recursion itself deviates by at most 3.8 cond eps), half log-det
within 8 times the float64 recursion's largest deviation (8 * 7.5e-11 = 6.0e-10 relative).
Two NGD rows (n = 12 at T = 513 and n = 6 at T = 49153: four passes each) take the deep plans through ngd_init + ngd_gradients on
the quadratic problems of test_asm_dense_vs_reference_gpu._problem: dmu and the state's SigD against the closed form
(asm_closed_form.closed_form + the sequential block solve) at TIGHT, assemble_on_load 1 against 0 bit for bit.

Measured on an MI355X (122 cases, 9.4 s; no case failed, no kernel was changed).  Well cases, largest per padded N:
    N     SD / SU vs reference   half log-det (relative)   asymmetry of SD[t] / scale
    1          5.2e-16                 1.2e-15                    0 (one entry)
    2          7.0e-16                 2.0e-15                    9.1e-17
    3          6.2e-16                 1.9e-15                    7.8e-17
    4          1.3e-15                 1.0e-14                    1.5e-16
    6          1.0e-15                 4.2e-15                    1.7e-16
    8          1.2e-15                 1.7e-14                    1.4e-16
    12         1.5e-15                 9.3e-16                    1.6e-16
    16         1.2e-15                 5.1e-16                    1.9e-16
SD[t] is symmetric to an ulp of its scale but NOT in equal bits for N >= 2 (the two Schur products that meet in an entry and
its mirror are summed in different orders), so the assertion is the 1e-13 one.
Scaling: SD and SU came out bit-exact at k = +-40 AND k = +-300 for every N (no operation of the path is scale-inexact); the half
log-det followed T n k ln2 / 2 to at most 2.1e-16 relative (e.g. T = 49153, n = 5, k = 300: 25649897.36848485).
Stiff cases against longdouble (absolute in rel's form = relative to the largest entry; cond eps; half log-det relative, bound
6.0e-10):
    (65, 2)   5.5e-11  0.03    8.8e-13        (40, 8)    1.2e-10  0.06    8.3e-13
    (65, 3)   2.0e-11  0.01    5.2e-14        (65, 11)   5.1e-11  0.03    2.5e-13
    (97, 4)   6.8e-11  0.03    2.6e-13        (65, 12)   8.4e-11  0.05    1.5e-13
    (49, 6)   8.9e-11  0.05    3.4e-13        (65, 16)   8.1e-11  0.04    1.5e-13
-- the kernels' cyclic reduction is up to 60 times CLOSER to the longdouble result than the sequential float64 recursion (whose
error grows along the chain; a tree of depth log2 T does not), and the log-det figure sits 700 times inside its bound.
NGD rows: dmu 5.9e-12 (T = 513, n = 12) and 2.6e-12 (T = 49153, n = 6; 2.3 s, its closed form 3 s on the CPU), SigD 1.1e-15 and
9.4e-16; assemble_on_load 1 and 0 in equal bits.

What the module sees: five libraries with ONE line of kernels_chain.hpp's forward_body broken, values only (no address depends
on the changed line), each run against this module and against the earlier tests of the same operators
(test_bt_ops_vs_oracle, test_merged_chain_launch_operators_on_multi_pass_plans, test_c3_literal_chain_operator_parity):
  B1  the fold of a non-first pass reads W_LS + par, the buffer the pass itself writes, instead of W_LS + (par ^ 1):
      all 46 well cases of two or more passes that it was run on (the full-segment rows of B2 were not among them), all 8
      scaling, all 8 not-pd, 7 of 8 stiff (not the one-pass (65, 2)) and both NGD rows (then 513 and 1537) fail, with errors of
      order one (earlier tests: 18 cases).
  B2  the top pass folds the earlier passes' log-pivot entries up to lp_off - 1, one entry short: NOTHING failed on the case
      table as the issue lists it, here or in the earlier tests.  Every multi-pass length of that table is 2^k + 1 or close
      to it: the last workgroup of the earlier pass holds one or two nodes, its last wave eliminates nothing and its entry is
      the neutral (1.0, 0).  Hence the rows with a FULL last segment (T = 160 at n = 1, 2; 96 at n = 3, 4; 64 at n = 5, 6; 32
      at n = 8; 16 and 128 at n = 12; 16 at n = 16): with them the log-det assertion fails at (160, 1), (160, 2), (96, 3),
      (96, 4), (64, 5), (64, 6) and nowhere else.  At N >= 8 a workgroup has more waves than a segment has level-0 nodes, the
      last wave's entry is neutral at any length, and the line is the same template line the N <= 6 rows cover.
  B3  the top pass's own reduction leaves out its last wave (k2 < nwaves - 1): 19 well cases (one-pass and deep plans, every
      N), all 8 scaling (the log-det no longer moves by the formula) and 4 not-pd cases (the NaN is lost) fail.
  B4  the identity padding takes 0.125 instead of 0.0 off the diagonal -- what a padding element let through ext_el does to
      the values; ext_el itself also forms the addresses of the stores, so it cannot be broken without writing past a block:
      all 34 well cases with n < N fail (n = 5, 7, 9, 11, 13), as do the 4 padded scaling, the 4 padded not-pd cases and the
      padded stiff case (65, 11); no unpadded case does.
  B5  the forward boundary test has_b = jb < cnt turned into jb <= cnt: nothing fails, and nothing can.  The phantom neighbour
      is slot cnt of the segment: its coupling is read from LDS, the Schur update goes to the zero-filled slot cnt and the new
      coupling to the W_NU entry of a node whose next-pass reader is switched off by x + st < T; pivots, factors and every
      slot a real node reads are untouched, and the backward recursion has its own test.  The same change in the BACKWARD
      tests (marginal_node's has_b) steers the SigU store of the last node one block past the array on one-pass plans; it was
      not built."""
import functools
import math
import os

import numpy as np
import pytest

import chain_selinv_ref as R
from asm_closed_form import closed_form
from gaussianvi_amd import api
from test_asm_dense_vs_reference_gpu import _context, _problem
from test_gpu_parity import TIGHT, rel

pytestmark = pytest.mark.gpu

WAVE_DEFAULT = int(os.environ.get("GVI_CHAIN_WAVE", "1") != "0")      # the switches as the library read them
PAIR_DEFAULT = int(os.environ.get("GVI_CHAIN_PAIR", "1") != "0")
MERGE_DEFAULT = int(os.environ.get("GVI_CHAIN_MERGE", "1") != "0")
DENSE_DEFAULT = int(os.environ.get("GVI_ASM_DENSE", "1") != "0")
EPS = np.finfo(np.float64).eps


def _ids(cases):
    return [f"T{T}-n{n}" for T, n in cases]


def _restore(ctx):
    ctx.set_option("chain_merge", MERGE_DEFAULT)
    ctx.set_option("chain_pair", PAIR_DEFAULT)                       # (the context closes next: harmless)
    ctx.set_option("chain_wave", WAVE_DEFAULT)
    ctx.close()


def factor_b(ctx, A, B, **options):
    """bt_marginals / bt_logdet of state A, then of state B, under the options; B's (SD, SU, half log-det)"""
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.bt_marginals(*A)
    ctx.bt_logdet(*A)
    SD, SU = ctx.bt_marginals(*B)
    return SD, SU, ctx.bt_logdet(*B)


def same_words(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()


def errors(got, ref):
    """(SD / SU error in test_gpu_parity.rel's form, relative half log-det error)"""
    return max(rel(got[0], ref[0]), rel(got[1], ref[1]) if got[1].size else 0.0), abs(got[2] - ref[2]) / abs(ref[2])


@pytest.mark.parametrize("T,n", R.WELL_CASES, ids=_ids(R.WELL_CASES))
def test_selected_inverse_and_logdet_against_the_sequential_recursion(T, n):
    A, B, ref = R.state_a(T, n), R.state_b(T, n), R.reference(T, n)
    npass = len(R.chain_passes(T, n))
    merge, pair, wave = [], {}, {}
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        got = factor_b(ctx, A, B)
        again = ctx.bt_marginals(*B) + (ctx.bt_logdet(*B),)
        ctx.ngd_init(np.zeros((T, n)), *A)                           # (state A first: it dirties the slot that B's word is read from)
        ctx.ngd_cost()
        ctx.ngd_init(np.zeros((T, n)), *B)
        hld_back = ctx.ngd_cost()                                    # the word left beside the selected inverse
        if npass >= 2:
            merge = [factor_b(ctx, A, B, chain_merge=m) for m in (1, 0, 1)]
            ctx.set_option("chain_merge", MERGE_DEFAULT)
        if n in (5, 6):
            pair = {p: factor_b(ctx, A, B, chain_pair=p) for p in (1, 0)}
        if n <= 2 and T <= 65:
            wave = {w: factor_b(ctx, A, B, chain_wave=w) for w in (1, 0)}
    finally:
        _restore(ctx)
    SD = got[0]
    err, err_h = errors(got, ref)
    for v in wave.values():
        err, err_h = max(err, errors(v, ref)[0]), max(err_h, errors(v, ref)[1])
    asym = np.abs(SD - np.swapaxes(SD, 1, 2)).max() / np.abs(SD).max()
    print(f"selinv case T {T} n {n} N {R.padded(n)} passes {npass}: SD / SU against the reference {err:.2e}, half log-det {err_h:.2e}, "
          f"asymmetry of SD {asym:.2e}, bits symmetric {np.array_equal(SD, np.swapaxes(SD, 1, 2))}")
    assert err < TIGHT
    assert np.isclose(got[2], ref[2], rtol=1e-12) and all(np.isclose(v[2], ref[2], rtol=1e-12) for v in wave.values())
    assert asym <= 1e-13
    assert same_words(again, got)
    assert np.float64(hld_back).tobytes() == np.float64(got[2]).tobytes(), (hld_back, got[2])
    if npass >= 2:
        assert same_words(merge[0], merge[1]) and same_words(merge[2], merge[1])
        assert errors(merge[1], ref)[0] < TIGHT and np.isclose(merge[1][2], ref[2], rtol=1e-12)
    if pair:
        assert same_words(pair[1], pair[0])
        assert errors(pair[0], ref)[0] < TIGHT and np.isclose(pair[0][2], ref[2], rtol=1e-12)
    if wave:
        assert max(rel(wave[1][0], wave[0][0]), rel(wave[1][1], wave[0][1])) < 1e-13
        assert abs(wave[1][2] - wave[0][2]) <= 1e-13 * abs(wave[0][2])


@pytest.mark.parametrize("T,n", R.SCALE_CASES, ids=_ids(R.SCALE_CASES))
def test_power_of_two_scaling_is_exact_and_the_logdet_accumulator_does_not_overflow(T, n):
    D, U = R.state_b(T, n)
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        base = factor_b(ctx, R.state_a(T, n), (D, U))
        scaled = {k: ctx.bt_marginals(np.ldexp(D, k), np.ldexp(U, k)) + (ctx.bt_logdet(np.ldexp(D, k), np.ldexp(U, k)),)
                  for k in (40, -40, 300, -300)}
    finally:
        _restore(ctx)
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all() and np.isfinite(base[2])
    for k, (SD, SU, hld) in scaled.items():
        want = base[2] + T * n * k * math.log(2.0) / 2
        print(f"scale case T {T} n {n} N {R.padded(n)} k {k}: SD exact {np.array_equal(SD, np.ldexp(base[0], -k))}, SU exact "
              f"{np.array_equal(SU, np.ldexp(base[1], -k))}, half log-det {hld!r} against {want!r}: {abs(hld - want) / abs(want):.2e}")
    for k, (SD, SU, hld) in scaled.items():
        assert np.isfinite(hld) and np.isfinite(SD).all() and np.isfinite(SU).all(), k
        assert np.array_equal(SD, np.ldexp(base[0], -k)) and np.array_equal(SU, np.ldexp(base[1], -k)), k
        assert np.isclose(hld, base[2] + T * n * k * math.log(2.0) / 2, rtol=1e-12, atol=0.0), k


@pytest.mark.parametrize("T,n", R.NOT_PD_CASES, ids=_ids(R.NOT_PD_CASES))
def test_logdet_is_nan_when_only_the_last_pass_meets_a_non_positive_pivot(T, n):
    B = R.state_b(T, n)
    Dn, U, e, h, _ = R.not_pd_state(T, n)
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        before = ctx.bt_logdet(*B)
        bad = ctx.bt_logdet(Dn, U)
        after = ctx.bt_logdet(*B)
    finally:
        _restore(ctx)
    print(f"not-pd case T {T} n {n} N {R.padded(n)}: node {e} shifted, found at node {h}: {bad}, positive definite state {before!r} / {after!r}")
    assert np.isnan(bad)
    assert np.isclose(before, R.reference(T, n)[2], rtol=1e-12) and np.float64(after).tobytes() == np.float64(before).tobytes()


@pytest.mark.parametrize("T,n", R.STIFF_CASES, ids=_ids(R.STIFF_CASES))
def test_stiff_chains_against_the_longdouble_recursion(T, n):
    ref = R.stiff_reference(T, n)
    ctx = api.Context(0)
    try:
        ctx.chain_set(T, n)
        SD, SU, hld = factor_b(ctx, R.state_a(T, n), R.stiff_state(T, n))
    finally:
        _restore(ctx)
    ce = ref["cond"] * EPS
    err = max(rel(SD.astype(np.longdouble), ref["SD"]), rel(SU.astype(np.longdouble), ref["SU"]))
    err_h = float(abs(np.longdouble(hld) - ref["hld"]) / abs(ref["hld"]))
    bound_h = 8 * R.stiff_logdet_yardstick()
    print(f"stiff case T {T} n {n} N {R.padded(n)} cond {ref['cond']:.2e}: SD / SU against longdouble {err:.2e} = {err / ce:.2f} cond eps "
          f"(float64 recursion {ref['dev'] / ce:.2f}), half log-det {err_h:.2e} (float64 recursion {ref['dev_hld']:.2e}, bound {bound_h:.2e})")
    assert err < 100 * ce
    assert err_h < bound_h


# ---- the deep plans inside the iteration ----
NGD_ROWS = [(513, 12), (49153, 6)]                                   # four passes each


@functools.lru_cache(maxsize=None)
def _ngd_reference(T, n):
    P = _problem(T, n, "bu", T - 1, T)
    mu, D, U = P["B"]
    sets = [dict(kind="b", start=np.arange(T - 1), Phi=P["Phi"], Q=P["Q"]), dict(kind="u", start=np.arange(T), mu_u=P["mu_u"], Kinv=P["Kinv"])]
    cf = closed_form(T, n, sets, mu, solve=False)
    dmu = R.solve(cf["VD"], cf["VU"], -cf["g"])
    SD = R.selinv(D, U)[0]
    for a in (dmu, SD):
        a.setflags(write=False)
    return dmu, SD


@pytest.mark.parametrize("T,n", NGD_ROWS, ids=_ids(NGD_ROWS))
def test_ngd_gradients_on_deep_plans_against_the_closed_form(T, n):
    P = _problem(T, n, "bu", T - 1, T)
    dmu_ref, SD_ref = _ngd_reference(T, n)
    out = {}
    for on_load in (1, 0):
        ctx = _context(P, WAVE_DEFAULT, dict(assemble_on_load=on_load))
        try:
            ctx.ngd_init(*P["A"])
            ctx.ngd_gradients()
            ctx.ngd_get_gradients()
            ctx.ngd_init(*P["B"])
            ctx.ngd_gradients()
            out[on_load] = (ctx.ngd_get_gradients(), ctx.ngd_get_state())
        finally:
            ctx.set_option("asm_dense", DENSE_DEFAULT)
            _restore(ctx)
    G, st = out[1]
    print(f"ngd row T {T} n {n} passes {len(R.chain_passes(T, n))}: dmu against the closed form {rel(G['dmu'], dmu_ref):.2e}, "
          f"SigD {rel(st['SigD'], SD_ref):.2e}")
    assert rel(G["dmu"], dmu_ref) < TIGHT and rel(st["SigD"], SD_ref) < TIGHT
    for k in G:
        assert G[k].tobytes() == out[0][0][k].tobytes(), k
    for k in st:
        assert st[k].tobytes() == out[0][1][k].tobytes(), k
