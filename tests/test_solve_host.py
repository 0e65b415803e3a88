"""CPU checks of the multi-right-hand-side solve's boundary (include/gvi_hip.h, "many right-hand sides"): the recurrences of
kernels_solve.hpp restated in numpy against a dense float64 solve, the ctypes table, and GVIGH::solve /
covariance_columns / cross_covariance compiling against the shim."""
import math
import os
import subprocess

import numpy as np
import pytest

from gaussianvi_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 2), (7, 4), (16, 6), (9, 9), (33, 16), (20, 14), (65, 6)]
NAMES = ["gvi_bt_solve_multi", "gvi_bt_cov_columns", "gvi_ngd_cov_columns", "gvi_ngd_cov_columns_dev"]


def random_chain(T, n, seed):
    """Random SPD block-tridiagonal (D, U) (block diagonal dominance) and a mean: the generator of tests/test_sample_gpu.py."""
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


def levels(T):
    L = 0
    while (1 << L) < T:
        L += 1
    return L


def cr_factor(D, U):
    """Block cyclic reduction of (D, U): level l keeps the multiples of 2^(l+1) and eliminates e = 2^l (mod 2^(l+1)) against
    a = e - 2^l, b = e + 2^l.  Per node R (R R^T = E = P_e^-1), GA = E Ua^T, GB = E Ub (kernels_sample.hpp)."""
    T, n = D.shape[0], D.shape[1]
    P = D.copy()
    C = {x: U[x] for x in range(T - 1)}              # C[x] = A[x, x + step] at the current level
    R, GA, GB = np.zeros_like(D), np.zeros_like(D), np.zeros_like(D)
    for l in range(levels(T)):
        step = 1 << l
        Cn = {}
        for e in range(step, T, 2 * step):
            a, b = e - step, e + step
            R[e] = np.linalg.inv(np.linalg.cholesky(P[e])).T
            E = R[e] @ R[e].T
            GA[e] = E @ C[a].T
            P[a] = P[a] - C[a] @ GA[e]
            if b < T:
                GB[e] = E @ C[e]
                P[b] = P[b] - C[e].T @ GB[e]
                Cn[a] = -C[a] @ GB[e]
        C = Cn
    R[0] = np.linalg.inv(np.linalg.cholesky(P[0])).T
    return R, GA, GB


def cr_solve(D, U, B, factor=None):
    """The sweep of solve_sweep_kernel for B [R][T][n]: up (the survivor gathers), then down.
    factor: a cr_factor(D, U) computed before (it is not written to)."""
    T = D.shape[0]
    L = levels(T)
    R, GA, GB = cr_factor(D, U) if factor is None else factor
    Y = np.array(B, dtype=float)
    for l in range(L):
        step = 1 << l
        for x in range(0, T, 2 * step):
            if x + step < T:
                Y[:, x] -= Y[:, x + step] @ GA[x + step]          # r_x -= GA^T r_{x+step}, for every right-hand side
            if x - step >= 0:
                Y[:, x] -= Y[:, x - step] @ GB[x - step]
    Y[:, 0] = (Y[:, 0] @ R[0]) @ R[0].T                            # x_root = R (R^T r)
    for l in range(L - 1, -1, -1):
        step = 1 << l
        for e in range(step, T, 2 * step):
            v = (Y[:, e] @ R[e]) @ R[e].T - Y[:, e - step] @ GA[e].T
            if e + step < T:
                v -= Y[:, e + step] @ GB[e].T
            Y[:, e] = v
    return Y


@pytest.mark.parametrize("T,n", SHAPES)
def test_recurrences_match_the_dense_solve(T, n):
    D, U, _ = random_chain(T, n, 300 + T * n)
    A = dense(D, U)
    B = np.random.default_rng(T * n).standard_normal((5, T, n))
    ref = np.linalg.solve(A, B.reshape(5, -1).T).T.reshape(5, T, n)
    X = cr_solve(D, U, B)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    assert err <= 1e-10, err
    # unit columns give the dense inverse
    N = T * n
    Cn = cr_solve(D, U, np.eye(N).reshape(N, T, n)).reshape(N, N)
    Sig = np.linalg.inv(A)
    err = np.abs(Cn - Sig).max() / np.abs(Sig).max()
    assert err <= 1e-10, err


def test_signatures_are_bound():
    for name in NAMES:
        assert name in _lib.SIGNATURES, name


def test_solve_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "solve_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "solve_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
