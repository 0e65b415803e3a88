"""Samples of q = N(mu, Lambda^-1) and log q on the device (gvi_randn / gvi_bt_sample / gvi_ngd_sample(_dev) /
gvi_bt_logpdf, GVIGH::sample / log_density)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from gaussianvi_amd import api, build, synthetic as syn
from test_sample_host import randn as py_randn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2PI = math.log(2.0 * math.pi)


def random_chain(T, n, seed):
    """Random SPD block-tridiagonal (D, U) (block diagonal dominance) and a mean."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((max(T - 1, 0), n, n)) * 0.4 / math.sqrt(n)
    nrm = np.array([np.linalg.norm(u, 2) for u in U])
    D = np.empty((T, n, n))
    for t in range(T):
        B = rng.standard_normal((n, n))
        s = (nrm[t] if t < T - 1 else 0.0) + (nrm[t - 1] if t > 0 else 0.0)
        D[t] = B @ B.T / n + (s + 0.5) * np.eye(n)
    mu = rng.uniform(-2.0, 2.0, (T, n))
    return D, U, mu


def dense(D, U):
    T, n = D.shape[0], D.shape[1]
    A = np.zeros((T * n, T * n))
    for t in range(T):
        A[t * n:(t + 1) * n, t * n:(t + 1) * n] = D[t]
        if t + 1 < T:
            A[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = U[t]
            A[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = U[t].T
    return A


def ctx_for(T, n):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    return ctx


@pytest.mark.parametrize("T,n", [(1, 1), (1, 5), (2, 3), (7, 4), (16, 6), (9, 9), (33, 16), (20, 14)])
def test_exact_covariance_from_identity_eps(T, n):
    D, U, mu = random_chain(T, n, 100 + T * n)
    N = T * n
    ctx = ctx_for(T, n)
    X = ctx.bt_sample(D, U, mu, N, eps=np.eye(N))
    F = (X - mu).reshape(N, N).T                  # column j = the draw from eps = e_j
    Sig = np.linalg.inv(dense(D, U))
    err = np.abs(F @ F.T - Sig).max() / np.abs(Sig).max()
    assert err < 1e-10, err
    ctx.close()


def test_generator_matches_restatement():
    ctx = ctx_for(2, 2)
    for seed in (0, 1, 0x123456789ABCDEF):
        for first in (0, 7, 2 ** 32 - 3, 2 ** 33 + 1):
            z = ctx.randn(seed, first, 37)
            np.testing.assert_allclose(z, py_randn(seed, first, 37), rtol=1e-12, atol=1e-14)
    ctx.close()


def test_stream_properties():
    T, n = 11, 3
    D, U, mu = random_chain(T, n, 5)
    ctx = ctx_for(T, n)
    seed = 424242
    X8 = ctx.bt_sample(D, U, mu, 8, seed=seed, first=0)
    X3 = ctx.bt_sample(D, U, mu, 3, seed=seed, first=5)
    assert np.array_equal(X3, X8[5:8])
    eps = ctx.randn(seed, 5 * T * n, 3 * T * n)
    assert np.array_equal(ctx.bt_sample(D, U, mu, 3, eps=eps), X3)
    X8b = ctx.bt_sample(D, U, mu, 8, seed=seed + 1, first=0)
    assert not np.any(X8b == X8)
    ctx.close()


def test_sample_statistics():
    T, n, S = 64, 6, 2 ** 15
    D, U, mu = random_chain(T, n, 64)
    ctx = ctx_for(T, n)
    X = ctx.bt_sample(D, U, mu, S, seed=2026)
    SD, SU = ctx.bt_marginals(D, U)
    se = np.sqrt(np.einsum("tii->ti", SD) / S)
    assert np.all(np.abs(X.mean(axis=0) - mu) <= 6 * se)
    Y = X - mu
    for t in range(T):
        Ct = Y[:, t].T @ Y[:, t] / S
        d = np.diag(SD[t])
        assert np.all(np.abs(Ct - SD[t]) <= 6 * np.sqrt((np.outer(d, d) + SD[t] ** 2) / S)), t
        if t + 1 < T:
            Cu = Y[:, t].T @ Y[:, t + 1] / S
            d1 = np.diag(SD[t + 1])
            assert np.all(np.abs(Cu - SU[t]) <= 6 * np.sqrt((np.outer(d, d1) + SU[t] ** 2) / S)), t
    ctx.close()


def test_logpdf_matches_dense():
    T, n, S = 7, 4, 5
    D, U, mu = random_chain(T, n, 9)
    ctx = ctx_for(T, n)
    X = mu + np.random.default_rng(1).standard_normal((S, T, n)) * 0.3
    lq = ctx.bt_logpdf(D, U, mu, X)
    A = dense(D, U)
    sgn, ld = np.linalg.slogdet(A)
    assert sgn > 0
    Y = (X - mu).reshape(S, -1)
    ref = -0.5 * np.einsum("si,ij,sj->s", Y, A, Y) + 0.5 * ld - 0.5 * T * n * LOG2PI
    np.testing.assert_allclose(lq, ref, rtol=1e-10)
    ctx.close()


@pytest.mark.parametrize("T,n", [(1025, 6), (4097, 12)])
def test_logpdf_of_samples_full_size(T, n):
    D, U, mu = random_chain(T, n, T)
    ctx = ctx_for(T, n)
    S = 16
    eps = np.random.default_rng(T).standard_normal((S, T, n))
    X = ctx.bt_sample(D, U, mu, S, eps=eps)
    lq = ctx.bt_logpdf(D, U, mu, X)
    hld = ctx.bt_logdet(D, U)
    ref = -0.5 * (eps.reshape(S, -1) ** 2).sum(axis=1) + hld - 0.5 * T * n * LOG2PI
    np.testing.assert_allclose(lq, ref, rtol=1e-9)
    ctx.close()


def _resident(name, sample_between):
    ch = syn.make_chain(name)
    ctx, _ = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    steps = []
    for i in range(4):
        steps.append(ctx.ngd_step(0.55, 10))
        if sample_between:
            ctx.ngd_sample(16, seed=i)
    return ctx, steps


@pytest.mark.parametrize("name", ["c2", "planar"])
def test_resident_state_samples(name):
    import torch
    ctx, steps = _resident(name, True)
    st = ctx.ngd_get_state()
    S, seed = 6, 77
    X = ctx.ngd_sample(S, seed=seed, first=3)
    assert np.array_equal(X, ctx.bt_sample(st["D"], st["U"], st["mu"], S, seed=seed, first=3))
    buf = torch.full((S, ctx.T, ctx.n), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ngd_sample_dev(S, buf.data_ptr(), seed=seed, first=3)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), X)
    # sampling between the steps leaves the iteration bit-identical
    ref, ref_steps = _resident(name, False)
    assert steps == ref_steps
    st_ref = ref.ngd_get_state()
    for k in ("mu", "D", "U", "SigD", "SigU"):
        assert np.array_equal(st[k], st_ref[k]), k
    assert ctx.ngd_counters() == ref.ngd_counters()
    ctx.close()
    ref.close()


def test_errors():
    T, n = 5, 3
    D, U, mu = random_chain(T, n, 3)
    ctx = ctx_for(T, n)
    Dbad = D.copy()
    Dbad[2] = -np.eye(n)
    X = ctx.bt_sample(Dbad, U, mu, 4, seed=1)
    assert np.all(np.isnan(X))
    assert np.all(np.isnan(ctx.bt_logpdf(Dbad, U, mu, np.zeros((2, T, n)))))
    lib, h = ctx.lib, ctx.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = np.empty((4, T, n))
    assert lib.gvi_bt_sample(h, p(D), p(U), p(mu), -1, 0, 0, None, p(out)) == 1
    assert lib.gvi_bt_sample(h, p(D), p(U), p(mu), 4, 0, 0, None, None) == 1
    assert lib.gvi_bt_sample(h, None, p(U), p(mu), 4, 0, 0, None, p(out)) == 1
    assert lib.gvi_bt_sample(h, p(D), p(U), p(mu), 0, 0, 0, None, p(out)) == 0
    assert lib.gvi_bt_logpdf(h, p(D), p(U), p(mu), -1, p(out), p(out)) == 1
    assert lib.gvi_bt_logpdf(h, p(D), p(U), p(mu), 4, p(out), None) == 1
    assert lib.gvi_randn(h, 0, 0, -1, p(out)) == 1
    assert lib.gvi_randn(h, 0, 0, 4, None) == 1
    assert lib.gvi_ngd_sample(h, 4, 0, 0, p(out)) == 5
    assert lib.gvi_ngd_sample_dev(h, 4, 0, 0, p(out)) == 5
    ctx.close()
    big = ctx_for(3, 17)
    Db, Ub, mb = random_chain(3, 17, 1)
    outb = np.empty((1, 3, 17))
    assert big.lib.gvi_bt_sample(big.h, p(Db), p(Ub), p(mb), 1, 0, 0, None, p(outb)) == 3
    big.close()


def test_shim_sample_matches_binding(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "sample_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "sample_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    v = {}
    for line in r.stdout.splitlines():
        tok = line.split()
        v[tok[0]] = tok[1:]
    T, n, S, seed = int(v["T"][0]), int(v["T"][2]), int(v["T"][4]), int(v["T"][6])
    mu = np.array(v["mu"], dtype=float).reshape(T, n)
    D = np.array(v["D"], dtype=float).reshape(T, n, n)
    U = np.array(v["U"], dtype=float).reshape(T - 1, n, n)
    X = np.array(v["X"], dtype=float).reshape(S, T, n)
    Xf = np.array(v["Xf"], dtype=float).reshape(S, T, n)
    logq = np.array(v["logq"], dtype=float)
    ctx = ctx_for(T, n)
    assert np.array_equal(X, ctx.bt_sample(D, U, mu, S, seed=seed))
    assert np.array_equal(Xf, X)
    np.testing.assert_allclose(logq, ctx.bt_logpdf(D, U, mu, X), rtol=1e-12)
    ctx.close()
