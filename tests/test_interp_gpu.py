"""Dense-time posterior on the device (gvi_interp_set / gvi_bt_interp / gvi_ngd_interp(_dev) / gvi_bt_interp_samples /
gvi_ngd_sample_interp(_dev), GVIGH::set_interpolation / interpolate / sample_interpolated).  Tolerances are the project's own: the
relative 1e-10 of the sample and solve tests where only rounding differs, the operator-level 1e-9 where the device's Cholesky of
Qt enters (kappa(Qt) <= 1e4 is asserted for those inputs)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from gaussianvi_amd import api, build, synthetic as syn
from test_solve_host import dense, random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1), (2, 16), (3, 2), (7, 4), (9, 9), (33, 6), (20, 14)]
TOL, TOL_OP = 1e-10, 1e-9


def ctx_for(T, n):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    return ctx


@functools.lru_cache(maxsize=None)
def problem(T, n):
    """(D, U, mu, SigD, SigU) of a shape, the marginals from the dense float64 inverse: computed once, never written to."""
    D, U, mu = random_chain(T, n, 500 + T * n)
    Sig = np.linalg.inv(dense(D, U))
    SigD = np.stack([Sig[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    SigU = np.stack([Sig[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] for t in range(T - 1)])
    for a in (D, U, mu, SigD, SigU):
        a.setflags(write=False)
    return D, U, mu, SigD, SigU


@functools.lru_cache(maxsize=None)
def queries(T, n, Q=None, noise=True):
    """Q = 3 (T - 1) + 1 queries by default: every interval three times and one more, shuffled (unsorted, duplicates, idx = 0 and
    idx = T - 2 included); random A, B, c; Qt random SPD with kappa <= 1e4, or None."""
    rng = np.random.default_rng(900 + 31 * T + n + (Q or 0))
    if Q is None:
        idx = np.concatenate([np.repeat(np.arange(T - 1), 3), [T - 2]])
        rng.shuffle(idx)
    else:
        idx = rng.integers(0, T - 1, Q)
    Q = idx.size
    A = rng.standard_normal((Q, n, n)) / np.sqrt(n)
    B = rng.standard_normal((Q, n, n)) / np.sqrt(n)
    c = rng.standard_normal((Q, n))
    Qt = None
    if noise:
        W = rng.standard_normal((Q, n, n))
        Qt = W @ W.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        assert max(np.linalg.cond(M) for M in Qt) <= 1e4
        Qt.setflags(write=False)
    idx = idx.astype(np.int32)
    for a in (idx, A, B, c):
        a.setflags(write=False)
    return idx, A, B, c, Qt


def moments_ref(idx, A, B, c, Qt, mu, SigD, SigU):
    mean = np.einsum("qrk,qk->qr", A, mu[idx]) + np.einsum("qrk,qk->qr", B, mu[idx + 1]) + c
    ASB = A @ SigU[idx] @ B.transpose(0, 2, 1)
    cov = A @ SigD[idx] @ A.transpose(0, 2, 1) + ASB + ASB.transpose(0, 2, 1) + B @ SigD[idx + 1] @ B.transpose(0, 2, 1)
    return mean, cov if Qt is None else cov + Qt


def rel(X, ref):
    return np.abs(X - ref).max() / np.abs(ref).max()


def samples_ref(idx, A, B, c, L, X, z):
    """(expected Xq, component-wise magnitude) of A x_i + B x_i+1 + c + L z for X [S][T][n], z [S][Q][n] or None."""
    xi, xj = X[:, idx], X[:, idx + 1]                        # [S][Q][n]
    ref = np.einsum("qrk,sqk->sqr", A, xi) + np.einsum("qrk,sqk->sqr", B, xj) + c
    mag = np.einsum("qrk,sqk->sqr", np.abs(A), np.abs(xi)) + np.einsum("qrk,sqk->sqr", np.abs(B), np.abs(xj)) + np.abs(c)
    if z is not None:
        ref = ref + np.einsum("qrk,sqk->sqr", L, z)
        mag = mag + np.einsum("qrk,sqk->sqr", np.abs(L), np.abs(z))
    return ref, mag


def sweep_tile(S, Q, n):
    """The sweep's launch geometry (run_interp_sweep): queries per workgroup, samples per workgroup."""
    qpb = 4 * (64 // n)
    qblocks = (Q + qpb - 1) // qpb
    tile = 1
    while tile < 16 and qblocks * ((S + 2 * tile - 1) // (2 * tile)) >= 1024:
        tile *= 2
    return qpb, tile


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("T,n", SHAPES)
def test_moments(T, n, noise):
    _, _, mu, SigD, SigU = problem(T, n)
    idx, A, B, c, Qt = queries(T, n, None, noise)
    ctx = ctx_for(T, n)
    ctx.interp_set(idx, A, B, c, Qt)
    assert ctx.interp_info() == (3 * (T - 1) + 1, 0)
    mean, cov = ctx.bt_interp(mu, SigD, SigU)
    rmean, rcov = moments_ref(idx, A, B, c, Qt, mu, SigD, SigU)
    em, ec, es = rel(mean, rmean), rel(cov, rcov), np.abs(cov - cov.transpose(0, 2, 1)).max() / np.abs(rcov).max()
    print("moments", T, n, noise, em, ec, es)
    assert em <= TOL and ec <= TOL and es <= TOL, (em, ec, es)
    # one query, no c
    ctx.interp_set(idx[:1], A[:1], B[:1], None, None if Qt is None else Qt[:1])
    mean1, cov1 = ctx.bt_interp(mu, SigD, SigU)
    rmean1, rcov1 = moments_ref(idx[:1], A[:1], B[:1], 0.0, None if Qt is None else Qt[:1], mu, SigD, SigU)
    assert mean1.shape == (1, n) and rel(mean1, rmean1) <= TOL and rel(cov1, rcov1) <= TOL
    ctx.close()


def planner_problem(T=9, m=4):
    """make_planar_chain's initial precision (prior + end anchors + 0.5 I on every state) and the fine chain with m - 1 more
    prior states per interval that has the same posterior at the support states."""
    ch = syn.make_planar_chain(T=T)
    n, nd, dt = 4, 2, 0.25
    Nf = (T - 1) * m + 1
    Phi, Qinv = syn._minacc(nd, syn.QC, dt / m)
    G = np.hstack([-Phi, np.eye(n)])
    M = G.T @ Qinv @ G
    Lf = np.zeros((Nf * n, Nf * n))
    for k in range(Nf - 1):
        Lf[k * n:(k + 2) * n, k * n:(k + 2) * n] += M
    Phic, Qinvc = syn._minacc(nd, syn.QC, dt)
    Gc = np.hstack([-Phic, np.eye(n)])
    Mc = Gc.T @ Qinvc @ Gc
    for t in range(T):                                       # what D0 holds beyond the prior's own blocks
        extra = ch["D0"][t] - (Mc[:n, :n] if t < T - 1 else 0) - (Mc[n:, n:] if t > 0 else 0)
        Lf[t * m * n:(t * m + 1) * n, t * m * n:(t * m + 1) * n] += extra
    return ch, np.linalg.inv(Lf), dt, m


def test_planner_case():
    ch, Sf, dt, m = planner_problem()
    T, n, nd = ch["T"], ch["n"], 2
    idx, A, B, Qt, node = [], [], [], [], []
    for i in range(T - 1):
        for j in range(m + 1):
            a, b, q = syn.minacc_interpolation(nd, syn.QC, dt, dt if j == m else j * (dt / m))
            idx.append(i); A.append(a); B.append(b); Qt.append(q); node.append(i * m + j)
    ctx = ctx_for(T, n)
    SigD, SigU = ctx.bt_marginals(ch["D0"], ch["U0"])
    ctx.interp_set(idx, np.stack(A), np.stack(B), None, np.stack(Qt))
    assert ctx.interp_info() == (len(idx), 0)
    mean, cov = ctx.bt_interp(ch["mu0"], SigD, SigU)
    ref = np.stack([Sf[f * n:(f + 1) * n, f * n:(f + 1) * n] for f in node])
    err = np.abs(cov - ref).max() / np.abs(ref).max()
    print("planner covariance against the fine chain", err)
    assert err <= TOL_OP, err
    for q, (i, f) in enumerate(zip(idx, node)):
        if f % m == 0:                                       # a support time: tau = 0 of interval i or tau = dt of interval i
            t = f // m
            assert np.array_equal(mean[q], ch["mu0"][t]) and np.array_equal(cov[q], SigD[t]), (q, i, t)
    ctx.close()


def run_samples(T, n, S, Q=None, first=2, seed=11, noise_seed=12):
    D, U, mu, _, _ = problem(T, n)
    idx, A, B, c, Qt = queries(T, n, Q)
    ctx = ctx_for(T, n)
    ctx.interp_set(idx, A, B, c, Qt)
    assert ctx.interp_info() == (idx.size, 0)
    X = ctx.bt_sample(D, U, mu, S, seed, first)
    z = ctx.randn(noise_seed, first * idx.size * n, S * idx.size * n).reshape(S, idx.size, n)
    Xq = ctx.bt_interp_samples(X, noise_seed, first)
    ref, mag = samples_ref(idx, A, B, c, np.linalg.cholesky(Qt), X, z)
    worst = (np.abs(Xq - ref) / mag).max()
    print("samples", T, n, S, idx.size, worst)
    assert (np.abs(Xq - ref) <= TOL_OP * mag).all(), worst
    return ctx, idx, A, B, c, Qt, X, mag


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("T,n", SHAPES)
def test_samples_reconstructed(T, n, S):
    ctx, idx, A, B, c, Qt, X, _ = run_samples(T, n, S)
    # the caller's normals instead of the generator: same bound
    eps = np.random.default_rng(S + T).standard_normal((S, idx.size, n))
    Xe = ctx.bt_interp_samples(X, 0, 0, eps)
    ref, mag = samples_ref(idx, A, B, c, np.linalg.cholesky(Qt), X, eps)
    assert (np.abs(Xe - ref) <= TOL_OP * mag).all(), (np.abs(Xe - ref) / mag).max()
    ctx.close()


def test_samples_ragged_tiles():
    T, n, S, Q = 9, 6, 257, 401
    qpb, tile = sweep_tile(S, Q, n)
    assert tile > 1 and S % tile == 1 and Q % qpb == 1       # the last tile is ragged in both directions
    run_samples(T, n, S, Q)[0].close()


def test_degenerate_noise():
    T, n, S = 7, 4, 3
    D, U, mu, _, _ = problem(T, n)
    idx, A, B, c, _ = queries(T, n)
    Q = idx.size
    ctx = ctx_for(T, n)
    X = ctx.bt_sample(D, U, mu, S, 5, 0)
    ctx.interp_set(idx, A, B, c, None)
    assert ctx.interp_info() == (Q, 0)
    X0 = ctx.bt_interp_samples(X, 9, 0)
    ref, mag = samples_ref(idx, A, B, c, None, X, None)
    assert (np.abs(X0 - ref) <= TOL * mag).all()
    # Qt = 0 adds nothing
    ctx.interp_set(idx, A, B, c, np.zeros((Q, n, n)))
    assert ctx.interp_info() == (Q, 0)
    assert np.array_equal(ctx.bt_interp_samples(X, 9, 0), X0)
    # Qt = v v^T: noise along v only, driven by the query's first normal
    v = np.array([0.7, -1.3, 0.2, 2.1])
    ctx.interp_set(idx, A, B, c, np.tile(np.outer(v, v), (Q, 1, 1)))
    assert ctx.interp_info() == (Q, 0)
    z = ctx.randn(9, 0, S * Q * n).reshape(S, Q, n)
    want = z[:, :, :1] * v
    got = ctx.bt_interp_samples(X, 9, 0) - X0
    err = np.abs(got - want).max() / np.abs(want).max()
    print("rank-one noise", err)
    assert err <= 1e-12, err
    # an indefinite Qt: that query is NaN in every sample, no other query is; moments are still computed
    Qt = np.tile(np.eye(n), (Q, 1, 1))
    Qt[5] = np.diag([1.0, 1.0, -1.0, 1.0])
    ctx.interp_set(idx, A, B, c, Qt)
    assert ctx.interp_info() == (Q, 1)
    Xb = ctx.bt_interp_samples(X, 9, 0)
    assert np.isnan(Xb[:, 5]).all() and not np.isnan(np.delete(Xb, 5, axis=1)).any()
    _, _, _, SigD, SigU = problem(T, n)
    mean, cov = ctx.bt_interp(mu, SigD, SigU)
    rmean, rcov = moments_ref(idx, A, B, c, Qt, mu, SigD, SigU)
    assert rel(mean, rmean) <= TOL and rel(cov, rcov) <= TOL
    ctx.close()


def test_splitting_and_repeatability():
    T, n, S, first = 9, 9, 5, 3
    D, U, mu, _, _ = problem(T, n)
    idx, A, B, c, Qt = queries(T, n)
    ctx = ctx_for(T, n)
    ctx.interp_set(idx, A, B, c, Qt)
    X = ctx.bt_sample(D, U, mu, S, 21, first)
    whole = ctx.bt_interp_samples(X, 22, first)
    parts = np.concatenate([ctx.bt_interp_samples(X[:2], 22, first), ctx.bt_interp_samples(X[2:], 22, first + 2)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole, ctx.bt_interp_samples(X, 22, first))
    assert not np.array_equal(whole, ctx.bt_interp_samples(X, 23, first))
    ctx.close()


def _planar_queries(ch, dt=0.25):
    idx, A, B, Qt = [], [], [], []
    for q, frac in enumerate([0.0, 0.5, 0.25, 1.0, 0.8, 0.1, 0.5]):
        a, b, qt = syn.minacc_interpolation(2, syn.QC, dt, frac * dt)
        idx.append([3, ch["T"] - 2, 0, 5, 3, 9, 0][q]); A.append(a); B.append(b); Qt.append(qt)
    return idx, np.stack(A), np.stack(B), np.stack(Qt)


def _resident(calls_between):
    ch = syn.make_planar_chain()
    ctx, _ = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    steps = [ctx.ngd_step(0.55, 10) for _ in range(2)]
    return ch, ctx, steps


def test_resident_state():
    import torch
    ch, ctx, steps = _resident(True)
    T, n, S = ctx.T, ctx.n, 4
    idx, A, B, Qt = _planar_queries(ch)
    Q = len(idx)
    ctx.interp_set(idx, A, B, None, Qt)
    st = ctx.ngd_get_state()
    mean, cov = ctx.ngd_interp()
    bm, bc = ctx.bt_interp(st["mu"], st["SigD"], st["SigU"])
    assert np.array_equal(mean, bm) and np.array_equal(cov, bc)
    assert np.array_equal(mean[0], st["mu"][3]) and np.array_equal(cov[0], st["SigD"][3])       # tau = 0
    X, Xq = ctx.ngd_sample_interp(S, 31, 32, 1)
    assert np.array_equal(X, ctx.ngd_sample(S, 31, 1))
    assert np.array_equal(Xq, ctx.bt_interp_samples(X, 32, 1))
    assert np.isfinite(Xq).all()
    assert np.array_equal(ctx.ngd_sample_interp(S, 31, 32, 1, want_X=False)[1], Xq)
    # the set survives the other consumers of the sampler's workspace
    ctx.ngd_sample(7, 1, 0)
    ctx.ngd_cov_columns([0, T - 1])
    assert ctx.interp_info() == (Q, 0)
    m2, c2 = ctx.ngd_interp()
    assert np.array_equal(m2, mean) and np.array_equal(c2, cov)
    # device twins
    dm = torch.full((Q, n), float("nan"), dtype=torch.float64, device="cuda:0")
    dc = torch.full((Q, n, n), float("nan"), dtype=torch.float64, device="cuda:0")
    dX = torch.full((S, T, n), float("nan"), dtype=torch.float64, device="cuda:0")
    dXq = torch.full((S, Q, n), float("nan"), dtype=torch.float64, device="cuda:0")
    dXq2 = torch.full((S, Q, n), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ngd_interp_dev(dm.data_ptr(), dc.data_ptr())
    ctx.ngd_sample_interp_dev(S, dXq.data_ptr(), 31, 32, 1, x_ptr=dX.data_ptr())
    ctx.ngd_sample_interp_dev(S, dXq2.data_ptr(), 31, 32, 1)
    ctx.sync()
    assert np.array_equal(dm.cpu().numpy(), mean) and np.array_equal(dc.cpu().numpy(), cov)
    assert np.array_equal(dX.cpu().numpy(), X) and np.array_equal(dXq.cpu().numpy(), Xq) and np.array_equal(dXq2.cpu().numpy(), Xq)
    # a third step after the calls: the same record, state and counters as a context that never made them
    third = ctx.ngd_step(0.55, 10)
    _, ref, ref_steps = _resident(False)
    assert steps == ref_steps and third == ref.ngd_step(0.55, 10)
    st, st_ref = ctx.ngd_get_state(), ref.ngd_get_state()
    for k in ("mu", "D", "U", "SigD", "SigU"):
        assert np.array_equal(st[k], st_ref[k]), k
    assert ctx.ngd_counters() == ref.ngd_counters()
    ctx.close()
    ref.close()


def test_status_codes():
    T, n = 5, 3
    D, U, mu, SigD, SigU = problem(T, n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    ctx = ctx_for(T, n)
    lib, h = ctx.lib, ctx.h
    idx, A, B, c, Qt = queries(T, n)
    Q = idx.size
    mean, cov = np.empty((Q, n)), np.empty((Q, n, n))
    X, Xq = np.zeros((2, T, n)), np.empty((2, Q, n))
    # a query before gvi_interp_set
    assert lib.gvi_bt_interp(h, p(mu), p(SigD), p(SigU), p(mean), p(cov)) == 5
    assert lib.gvi_bt_interp_samples(h, 2, p(X), 0, 0, None, p(Xq)) == 5
    assert ctx.interp_info() == (0, 0)
    ctx.interp_set(idx, A, B, c, Qt)
    # idx outside [0, T - 2], a negative count, a required NULL: the set is left unchanged
    for bad in (T - 1, -1):
        ib = idx.copy()
        ib[2] = bad
        assert lib.gvi_interp_set(h, Q, p(ib), p(A), p(B), p(c), p(Qt)) == 1
    assert lib.gvi_interp_set(h, -1, p(idx), p(A), p(B), p(c), p(Qt)) == 1
    assert lib.gvi_interp_set(h, Q, None, p(A), p(B), p(c), p(Qt)) == 1
    assert lib.gvi_interp_set(h, Q, p(idx), None, p(B), p(c), p(Qt)) == 1
    assert lib.gvi_interp_set(h, Q, p(idx), p(A), None, p(c), p(Qt)) == 1
    assert ctx.interp_info() == (Q, 0)
    assert lib.gvi_bt_interp(h, p(mu), p(SigD), p(SigU), p(mean), p(cov)) == 0
    assert rel(mean, moments_ref(idx, A, B, c, Qt, mu, SigD, SigU)[0]) <= TOL
    # argument checks of the query calls
    assert lib.gvi_bt_interp(h, None, p(SigD), p(SigU), p(mean), p(cov)) == 1
    assert lib.gvi_bt_interp(h, p(mu), p(SigD), p(SigU), None, p(cov)) == 1
    assert lib.gvi_bt_interp_samples(h, -1, p(X), 0, 0, None, p(Xq)) == 1
    assert lib.gvi_bt_interp_samples(h, 2, None, 0, 0, None, p(Xq)) == 1
    assert lib.gvi_bt_interp_samples(h, 2, p(X), 0, 0, None, None) == 1
    assert lib.gvi_bt_interp_samples(h, 2, p(X), 0, -1, None, p(Xq)) == 1
    Xq[:] = 7.0
    assert lib.gvi_bt_interp_samples(h, 0, p(X), 0, 0, None, p(Xq)) == 0 and (Xq == 7.0).all()     # S = 0: a no-op
    # the resident forms before gvi_ngd_init, then their argument checks
    assert lib.gvi_ngd_interp(h, p(mean), p(cov)) == 5
    assert lib.gvi_ngd_interp_dev(h, p(mean), p(cov)) == 5
    assert lib.gvi_ngd_sample_interp(h, 2, 0, 0, 0, p(X), p(Xq)) == 5
    assert lib.gvi_ngd_sample_interp_dev(h, 2, 0, 0, 0, p(X), p(Xq)) == 5
    ctx.ngd_init(mu, D, U)
    assert lib.gvi_ngd_interp(h, None, p(cov)) == 1
    assert lib.gvi_ngd_interp_dev(h, p(mean), None) == 1
    for fn in (lib.gvi_ngd_sample_interp, lib.gvi_ngd_sample_interp_dev):
        assert fn(h, -1, 0, 0, 0, p(X), p(Xq)) == 1
        assert fn(h, 2, 0, 0, 0, p(X), None) == 1
        assert fn(h, 2, 0, 0, -1, p(X), p(Xq)) == 1
        assert fn(h, 0, 0, 0, 0, p(X), p(Xq)) == 0
    assert lib.gvi_ngd_sample_interp(h, 2, 0, 0, 0, None, p(Xq)) == 0
    # Q = 0 clears the set; gvi_chain_set clears it
    ctx.interp_set([], np.empty((0, n, n)), np.empty((0, n, n)))
    assert ctx.interp_info() == (0, 0)
    assert lib.gvi_ngd_interp(h, p(mean), p(cov)) == 5
    ctx.interp_set(idx, A, B, c, Qt)
    assert ctx.interp_info() == (Q, 0)
    ctx.chain_set(T, n)
    assert ctx.interp_info() == (0, 0)
    assert lib.gvi_bt_interp(h, p(mu), p(SigD), p(SigU), p(mean), p(cov)) == 5
    ctx.close()
    # no interval at T = 1
    one = ctx_for(1, n)
    i0 = np.zeros(1, dtype=np.int32)
    assert one.lib.gvi_interp_set(one.h, 1, p(i0), p(A), p(B), None, None) == 1
    one.close()
    # before gvi_chain_set
    fresh = api.Context(0)
    assert fresh.lib.gvi_interp_set(fresh.h, 1, p(i0), p(A), p(B), None, None) == 5
    assert fresh.lib.gvi_bt_interp(fresh.h, p(mu), p(SigD), p(SigU), p(mean), p(cov)) == 5
    fresh.close()
    # n = 17
    big = ctx_for(3, 17)
    Ab = np.zeros((1, 17, 17))
    assert big.lib.gvi_interp_set(big.h, 1, p(i0), p(Ab), p(Ab), None, None) == 3
    big.close()


def test_shim_interpolation(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "interp_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "interp_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
