"""Costs of sampled trajectories on the device (include/gvi_hip.h, "costs of sampled trajectories"): per-factor costs of every
psi kind and the clearance of the hinge-on-SDF kinds against the oracle's closures, the total J and its reduction, the resident
path (samples, J, log q, minimum clearance in one call), determinism, fresh inputs, a statistical end-to-end check and the
non-finite / argument rules.

Bounds: max-norm relative error (rel of tests/test_gpu_parity.py) <= 1e-11 for the sum-of-squares kinds and <= 1e-8 for every
other kind -- the bounds of that file's operator-level parity tests."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o
from chains import make_chain
from gaussianvi_amd import api, build, synthetic as syn
from test_gpu_parity import quad_params, rel
from test_sample_cost_host import OBSTACLE_CHAINS, clearance_ref, factor_slices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 33                                       # no multiple of any tile
NAMES = ["tiny", "c3t2", "c3t3", "c3mini", "planar", "quad2d", "pr3d", "arm7", "range1d", "wide"]
SUMSQ = (syn.PSI_QUAD_PRIOR, syn.PSI_FIXED_PRIOR)
BOUND = {True: 1e-11, False: 1e-8}


@functools.lru_cache(maxsize=None)
def chain(name):
    if name == "range1d":                    # one state, one factor, the parameters of o.psi_batch_range_1d
        params = np.array([[1.2, 20.0, 40.0, 0.09, 9.0]])
        spec = dict(kind=syn.PSI_RANGE_1D, d=1, p=3, start=np.zeros(1, dtype=np.int32), params=params, temperature=np.ones(1),
                    psi_batch=o.psi_batch_range_1d(*params[0]))
        return dict(name=name, T=1, n=1, specs=[spec], mu0=np.array([[20.0]]), D0=np.array([[[1.0]]]), U0=np.zeros((0, 1, 1)))
    if name == "wide":                       # the widest register row: d = 24, twelve residual rows, temperatures != 1
        rng = np.random.default_rng(2401)
        T, n, K = 3, 12, 2
        Phi, Qinv = quad_params(rng, K, n)
        spec = dict(kind=syn.PSI_QUAD_PRIOR, d=2 * n, p=3, start=np.arange(K, dtype=np.int32),
                    params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1), temperature=rng.uniform(0.5, 2.0, K),
                    psi_batch=o.psi_batch_quad_prior(Phi, Qinv))
        return dict(name=name, T=T, n=n, specs=[spec], mu0=rng.normal(size=(T, n)), D0=np.stack([2.0 * np.eye(n)] * T),
                    U0=0.3 * rng.normal(size=(T - 1, n, n)) / np.sqrt(n))
    ch = make_chain(name)
    if name == "planar":                     # the obstacle set at the high temperature planar1k runs at
        ch["specs"][1]["temperature"] = np.full(len(ch["specs"][1]["start"]), 30.0)
    return ch


def context(name):
    return api.context_for_chain(chain(name))


def reference_costs(ch, X):
    """[cost [S][K] per set]: the spec's psi_batch at the factor slices over the temperature."""
    return [(sp["psi_batch"](factor_slices(X, sp, ch["n"])) / np.asarray(sp["temperature"])[:, None]).T for sp in ch["specs"]]


def obstacle_share(ch, X):
    psi = ch["specs"][1]["psi_batch"](factor_slices(X, ch["specs"][1], ch["n"]))
    return float((psi > 0).mean())


SEED = 4100        # shares of (sample, factor) pairs with psi > 0 at this seed: planar 0.353, quad2d 0.091, pr3d 0.539, arm7 0.921


@functools.lru_cache(maxsize=None)
def samples(name):
    """(X [S][T][n], reference costs): device samples of the chain's initial state, computed once.  On the obstacle chains the
    share of (sample, factor) pairs with psi > 0 must lie in [0.03, 0.97], so that both hinge branches are exercised."""
    ch = chain(name)
    ctx = api.Context(0)
    ctx.chain_set(ch["T"], ch["n"])
    X = ctx.bt_sample(ch["D0"], ch["U0"], ch["mu0"], S, seed=SEED)
    ctx.close()
    assert np.isfinite(X).all()
    if name in OBSTACLE_CHAINS:
        share = obstacle_share(ch, X)
        print(f"{name}: share of pairs with psi > 0: {share:.3f}")
        assert 0.03 <= share <= 0.97, "both hinge branches must be exercised"
    return X, reference_costs(ch, X)


@pytest.mark.parametrize("name", NAMES)
def test_factor_costs_vs_oracle(name):
    ch = chain(name)
    X, ref = samples(name)
    ctx, ids = context(name)
    for sid, sp, r in zip(ids, ch["specs"], ref):
        got = ctx.sample_factor_costs(sid, X)
        err = rel(got, r)
        print(f"{name}: set {sid} kind {sp['kind']} d {sp['d']}: cost error {err:.3e}")
        assert got.shape == r.shape and np.abs(r).max() > 0
        assert err <= BOUND[sp["kind"] in SUMSQ], (name, sid, err)
    ctx.close()


@pytest.mark.parametrize("name", OBSTACLE_CHAINS)
def test_clearance_vs_restatement(name):
    ch = chain(name)
    X, _ = samples(name)
    ctx, ids = context(name)
    ref = clearance_ref(ch["specs"][1], factor_slices(X, ch["specs"][1], ch["n"])).T
    got = ctx.sample_clearance(ids[1], X)
    err = rel(got, ref)
    print(f"{name}: clearance error {err:.3e}; min {ref.min():.3f}, share negative {(ref < 0).mean():.3f}")
    assert err <= 1e-8, err
    with pytest.raises(api.GviError) as e:
        ctx.sample_clearance(ids[0], X)                     # the QUAD_PRIOR set
    assert e.value.status == 3
    ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_total_cost_and_minimum_clearance(name):
    ch = chain(name)
    X, ref = samples(name)
    ctx, ids = context(name)
    Jref = np.sum([r.sum(axis=1) for r in ref], axis=0)
    J = ctx.sample_costs(X)
    err = np.abs(J - Jref).max() / np.abs(Jref).max()
    print(f"{name}: J error {err:.3e}")
    assert err <= 1e-10, err
    if name in OBSTACLE_CHAINS:
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        r = ctx.ngd_sample_costs(S, seed=5, clearance_set=ids[1])
        clr = ctx.sample_clearance(ids[1], r["X"])
        assert np.array_equal(r["clr_min"], clr.min(axis=1))
        assert np.array_equal(r["J"], ctx.sample_costs(r["X"]))
    ctx.close()


def _resident():
    ch = chain("planar")
    ctx, ids = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    steps = [ctx.ngd_step(0.55, 10) for _ in range(3)]
    return ctx, ids, steps


def test_resident_path():
    import torch
    ctx, ids, steps = _resident()
    T, n, Sr, seed, first = ctx.T, ctx.n, 17, 77, 4
    before = ctx.ngd_get_state()
    r = ctx.ngd_sample_costs(Sr, seed, first, clearance_set=ids[1])
    X = r["X"]
    assert np.array_equal(X, ctx.ngd_sample(Sr, seed, first))
    assert np.array_equal(r["J"], ctx.sample_costs(X))
    assert np.array_equal(r["logq"], ctx.bt_logpdf(before["D"], before["U"], before["mu"], X))
    assert np.array_equal(r["clr_min"], ctx.sample_clearance(ids[1], X).min(axis=1))
    assert np.isfinite(r["J"]).all() and np.isfinite(r["logq"]).all() and np.isfinite(r["clr_min"]).all()
    r2 = ctx.ngd_sample_costs(Sr, seed, first, clearance_set=ids[1], want_X=False)
    assert r2["X"] is None
    for k in ("J", "logq", "clr_min"):
        assert np.array_equal(r2[k], r[k]), k
    # device twin, with and without the samples
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")   # noqa: E731
    dX, dJ, dl, dc, dJ2, dl2, dc2 = nan(Sr, T, n), nan(Sr), nan(Sr), nan(Sr), nan(Sr), nan(Sr), nan(Sr)
    torch.cuda.synchronize()
    ctx.ngd_sample_costs_dev(Sr, dJ.data_ptr(), seed, first, ids[1], x_ptr=dX.data_ptr(), logq_ptr=dl.data_ptr(), clr_min_ptr=dc.data_ptr())
    ctx.ngd_sample_costs_dev(Sr, dJ2.data_ptr(), seed, first, ids[1], logq_ptr=dl2.data_ptr(), clr_min_ptr=dc2.data_ptr())
    ctx.sync()
    assert np.array_equal(dX.cpu().numpy(), X)
    for a, b, k in ((dJ, dJ2, "J"), (dl, dl2, "logq"), (dc, dc2, "clr_min")):
        assert np.array_equal(a.cpu().numpy(), r[k]) and np.array_equal(b.cpu().numpy(), r[k]), k
    # the operator twins on the device samples
    dJ3, dK = nan(Sr), nan(Sr, ctx.sets[ids[1]][0])
    torch.cuda.synchronize()
    ctx.sample_costs_dev(Sr, dX.data_ptr(), dJ3.data_ptr())
    ctx.sample_clearance_dev(ids[1], Sr, dX.data_ptr(), dK.data_ptr())
    ctx.sync()
    assert np.array_equal(dJ3.cpu().numpy(), r["J"]) and np.array_equal(dK.cpu().numpy().min(axis=1), r["clr_min"])
    # the state is untouched, and the next step is the step of a context that never sampled
    after = ctx.ngd_get_state()
    for k in ("mu", "D", "U", "SigD", "SigU"):
        assert np.array_equal(before[k], after[k]), k
    ref, _, ref_steps = _resident()
    assert steps == ref_steps and ctx.ngd_step(0.55, 10) == ref.ngd_step(0.55, 10)
    ctx.close()
    ref.close()


def test_determinism_and_batch_independence():
    ctx, ids, _ = _resident()
    a = ctx.ngd_sample_costs(8, 123, 0, clearance_set=ids[1])
    b = ctx.ngd_sample_costs(8, 123, 0, clearance_set=ids[1])
    c = ctx.ngd_sample_costs(3, 123, 5, clearance_set=ids[1])
    for k in ("X", "J", "logq", "clr_min"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][5:8], c[k]), k
    X, _ = samples("planar")
    assert np.array_equal(ctx.sample_costs(X), ctx.sample_costs(X))
    assert np.array_equal(ctx.sample_costs(X)[7:19], ctx.sample_costs(X[7:19]))
    assert np.array_equal(ctx.sample_factor_costs(ids[0], X)[30:], ctx.sample_factor_costs(ids[0], X[30:]))
    ctx.close()


@pytest.mark.parametrize("name", ["c3mini", "quad2d"])
def test_fresh_inputs_in_one_context(name):
    """X1 and then a different X2 of another S in ONE context: every X2 result is X2's (a stale scratch buffer or set list would
    return X1's numbers)."""
    ch = chain(name)
    X1, _ = samples(name)
    rng = np.random.default_rng(99)
    X2 = (X1[:12] + 0.05 * rng.normal(size=X1[:12].shape))[::-1].copy()
    ref2 = reference_costs(ch, X2)
    ctx, ids = context(name)
    J1 = ctx.sample_costs(X1)
    for sid in ids:
        ctx.sample_factor_costs(sid, X1)
    J2 = ctx.sample_costs(X2)
    Jref = np.sum([r.sum(axis=1) for r in ref2], axis=0)
    assert np.abs(J2 - Jref).max() <= 1e-10 * np.abs(Jref).max()
    assert not np.any(J2 == J1[:12])
    for sid, sp, r in zip(ids, ch["specs"], ref2):
        got = ctx.sample_factor_costs(sid, X2)
        assert rel(got, r) <= BOUND[sp["kind"] in SUMSQ], sid
    if name in OBSTACLE_CHAINS:
        k1 = ctx.sample_clearance(ids[1], X1)
        k2 = ctx.sample_clearance(ids[1], X2)
        assert rel(k2, clearance_ref(ch["specs"][1], factor_slices(X2, ch["specs"][1], ch["n"])).T) <= 1e-8
        assert not np.array_equal(k2, k1[:12])
    ctx.close()


def test_mean_cost_of_samples_is_the_expected_cost():
    """c3mini, S = 2^14: the sample mean of J estimates sum E_q[psi_k] / T_k, which the sparse Gauss-Hermite rule gives exactly
    for these quadratic psi at p = 5 (gvi_ngd_factor_costs); 6 standard errors, the multiplier of test_sample_statistics."""
    ch = chain("c3mini")
    ctx, ids = context("c3mini")
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    Sn = 2 ** 14
    r = ctx.ngd_sample_costs(Sn, seed=2026, want_X=False, want_logq=False)
    expected = sum(ctx.ngd_factor_costs(sid).sum() for sid in ids)
    J = r["J"]
    se = J.std() / np.sqrt(Sn)
    print(f"mean J {J.mean():.6f}, expected {expected:.6f}, standard error {se:.3e}")
    assert np.isfinite(J).all() and abs(J.mean() - expected) <= 6 * se
    ctx.close()


def test_non_finite_samples_and_argument_rules():
    ch = chain("planar")
    T, n = ch["T"], ch["n"]
    X = samples("planar")[0][:4].copy()
    ctx, ids = context("planar")
    clean = [ctx.sample_factor_costs(sid, X) for sid in ids]
    clean_clr = ctx.sample_clearance(ids[1], X)
    clean_J = ctx.sample_costs(X)
    Xb = X.copy()
    Xb[2, 5, 1] = np.nan
    touched = [np.array([st <= 5 < st + sp["d"] // n for st in sp["start"]]) for sp in ch["specs"]]
    assert [int(t.sum()) for t in touched] == [2, 1, 0]
    for sid, t, c in zip(ids, touched, clean):
        got = ctx.sample_factor_costs(sid, Xb)
        bad = np.zeros(c.shape, dtype=bool)
        bad[2, t] = True
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], c[~bad]), sid
    got = ctx.sample_clearance(ids[1], Xb)
    bad = np.zeros(clean_clr.shape, dtype=bool)
    bad[2, 5] = True
    assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean_clr[~bad])
    J = ctx.sample_costs(Xb)
    assert np.isnan(J[2]) and np.array_equal(np.delete(J, 2), np.delete(clean_J, 2))
    Xi = X.copy()
    Xi[0, 0, 0] = np.inf
    assert np.isnan(ctx.sample_factor_costs(ids[2], Xi)[0, 0]) and np.isnan(ctx.sample_costs(Xi)[0])
    # argument rules through raw ctypes
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    lib, h = ctx.lib, ctx.h
    K0 = len(ch["specs"][0]["start"])
    out, Jb = np.full((4, K0), 7.0), np.full(4, 7.0)
    assert lib.gvi_sample_costs(h, 0, p(X), p(Jb)) == 0 and (Jb == 7.0).all()                     # S = 0: a no-op
    assert lib.gvi_sample_factor_costs(h, ids[0], 0, p(X), p(out)) == 0 and (out == 7.0).all()
    assert ctx.sample_costs(np.empty((0, T, n))).shape == (0,)
    assert lib.gvi_sample_costs(h, -1, p(X), p(Jb)) == 1
    assert lib.gvi_sample_costs(h, 4, None, p(Jb)) == 1 and lib.gvi_sample_costs(h, 4, p(X), None) == 1
    assert lib.gvi_sample_costs_dev(h, 4, None, p(Jb)) == 1
    for fn in (lib.gvi_sample_factor_costs, lib.gvi_sample_clearance, lib.gvi_sample_clearance_dev):
        assert fn(h, len(ids), 4, p(X), p(out)) == 1 and fn(h, -1, 4, p(X), p(out)) == 1
        assert fn(h, ids[1], -1, p(X), p(out)) == 1
        assert fn(h, ids[1], 4, None, p(out)) == 1 and fn(h, ids[1], 4, p(X), None) == 1
    assert lib.gvi_sample_clearance(h, ids[2], 4, p(X), p(out)) == 3                              # the anchors: no clearance
    # the resident calls before gvi_ngd_init, then their argument checks
    Xo = np.empty((4, T, n))
    for fn in (lib.gvi_ngd_sample_costs, lib.gvi_ngd_sample_costs_dev):
        assert fn(h, 4, 0, 0, -1, p(Xo), p(Jb), None, None) == 5
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    for fn in (lib.gvi_ngd_sample_costs, lib.gvi_ngd_sample_costs_dev):
        assert fn(h, -1, 0, 0, -1, None, p(Jb), None, None) == 1
        assert fn(h, 4, 0, 0, -1, None, None, None, None) == 1
        assert fn(h, 4, 0, -1, -1, None, p(Jb), None, None) == 1
        assert fn(h, 4, 0, 0, len(ids), None, p(Jb), None, p(Jb)) == 1
        assert fn(h, 4, 0, 0, ids[0], None, p(Jb), None, p(Jb)) == 3                              # clearance of the priors
        assert fn(h, 0, 0, 0, -1, None, p(Jb), None, None) == 0
    assert (Jb == 7.0).all()
    assert lib.gvi_ngd_sample_costs(h, 4, 0, 0, -1, None, p(Jb), None, None) == 0 and np.isfinite(Jb).all()
    ctx.close()
    # before gvi_chain_set
    fresh = api.Context(0)
    assert fresh.lib.gvi_sample_costs(fresh.h, 4, p(X), p(Jb)) == 5
    assert fresh.lib.gvi_sample_factor_costs(fresh.h, 0, 4, p(X), p(out)) == 5
    fresh.close()
    # a context that holds a PSI_HOST_CALLBACK set
    cb = api.Context(0)
    cb.chain_set(T, n)
    s_cb = cb.factors_add(n, 3, np.zeros(2, np.int32), api.PSI_HOST_CALLBACK)
    sp = ch["specs"][2]
    s_ok = cb.factors_add(sp["d"], sp["p"], sp["start"], sp["kind"], sp["params"], sp["temperature"])
    two = np.empty((4, 2))
    assert cb.lib.gvi_sample_factor_costs(cb.h, s_cb, 4, p(X), p(two)) == 3
    assert cb.lib.gvi_sample_clearance(cb.h, s_cb, 4, p(X), p(two)) == 3
    assert cb.lib.gvi_sample_costs(cb.h, 4, p(X), p(Jb)) == 3
    assert cb.lib.gvi_sample_factor_costs(cb.h, s_ok, 4, p(X), p(two)) == 0 and np.array_equal(two, clean[2])
    cb.ngd_init(ch["mu0"], ch["D0"], ch["U0"])                                                   # the resident calls too
    for fn in (cb.lib.gvi_ngd_sample_costs, cb.lib.gvi_ngd_sample_costs_dev):
        assert fn(cb.h, 4, 0, 0, -1, None, p(Jb), None, None) == 3
    cb.close()


def test_not_positive_definite_resident_precision_gives_nan():
    ch = chain("tiny")
    ctx, ids = context("tiny")
    D = ch["D0"].copy()
    D[2] = -D[2]
    ctx.ngd_init(ch["mu0"], D, ch["U0"])
    r = ctx.ngd_sample_costs(5, 1)
    assert np.isnan(r["X"]).all() and np.isnan(r["J"]).all() and np.isnan(r["logq"]).all()
    ctx.close()


def test_shim_sample_costs(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "sample_cost_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "sample_cost_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
