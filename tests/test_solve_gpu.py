"""Multi-right-hand-side solve and block columns of Lambda^-1 on the device (gvi_bt_solve_multi / gvi_bt_cov_columns /
gvi_ngd_cov_columns(_dev), GVIGH::solve / covariance_columns / cross_covariance).  Every tolerance is the 1e-10 relative of
test_sample_gpu.test_exact_covariance_from_identity_eps on the same generator (the float64 restatement of the recurrences in
test_solve_host.py stays under 1e-15 at every shape used here)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from gaussianvi_amd import api, build, synthetic as syn
from test_solve_host import SHAPES, dense, random_chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def ctx_for(T, n, lds=1):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    ctx.set_option("solve_lds", lds)
    return ctx


@functools.lru_cache(maxsize=None)
def problem(T, n):
    """(D, U, dense Lambda, dense Lambda^-1) of a shape: computed once, never written to."""
    D, U, _ = random_chain(T, n, 300 + T * n)
    A = dense(D, U)
    Sig = np.linalg.inv(A)
    for a in (D, U, A, Sig):
        a.setflags(write=False)
    return D, U, A, Sig


def rel(X, ref):
    return np.abs(X - ref).max() / np.abs(ref).max()


def unit_columns(T, n, nodes):
    """B [len(nodes) n][T][n]: right-hand side c n + k is the unit vector at (nodes[c], k)."""
    B = np.zeros((len(nodes) * n, T, n))
    for c, t in enumerate(nodes):
        for k in range(n):
            B[c * n + k, t, k] = 1.0
    return B


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("T,n", SHAPES)
def test_dense_parity(T, n, lds):
    D, U, A, _ = problem(T, n)
    B = np.random.default_rng(T * n).standard_normal((5, T, n))
    ref = np.linalg.solve(A, B.reshape(5, -1).T).T.reshape(5, T, n)
    ctx = ctx_for(T, n, lds)
    X = ctx.bt_solve_multi(D, U, B)
    err = rel(X, ref)
    print("dense parity", T, n, lds, err)
    assert err <= TOL, err
    X1 = ctx.bt_solve_multi(D, U, B[:1])
    assert rel(X1, ref[:1]) <= TOL
    err1 = rel(X1[0], ctx.bt_solve(D, U, B[0]))
    print("against bt_solve", err1)
    assert err1 <= TOL, err1
    ctx.close()


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("T,n", SHAPES)
def test_columns_against_the_dense_inverse(T, n, lds):
    D, U, _, Sig = problem(T, n)
    ctx = ctx_for(T, n, lds)
    nodes = list(range(T))
    Cc = ctx.bt_cov_columns(D, U, nodes)                       # [c][t][r][k] = Sig[t n + r, c n + k]
    ref = Sig.reshape(T, n, T, n).transpose(2, 0, 1, 3)
    err = rel(Cc, ref)
    print("columns", T, n, lds, err)
    assert err <= TOL, err
    scale = np.abs(ref).max()
    # block (t, j) of column j is the transpose of block (j, t) of column t
    assert np.abs(Cc - Cc.transpose(1, 0, 3, 2)).max() <= TOL * scale
    # the tridiagonal part is what the selected inverse gives
    SD, SU = ctx.bt_marginals(D, U)
    for j in range(T):
        assert np.abs(Cc[j][j] - SD[j]).max() <= TOL * scale, j
        if j + 1 < T:
            assert np.abs(Cc[j][j + 1] - SU[j].T).max() <= TOL * scale, j
        if j > 0:
            assert np.abs(Cc[j][j - 1] - SU[j - 1]).max() <= TOL * scale, j
    # the same numbers as the general solve on explicit unit columns
    X = ctx.bt_solve_multi(D, U, unit_columns(T, n, nodes))   # [c n + k][t][r]
    assert np.array_equal(Cc, X.reshape(T, n, T, n).transpose(0, 2, 3, 1))
    # duplicates, descending order
    pick = [T - 1, T // 2, T // 2, 0]
    Cp = ctx.bt_cov_columns(D, U, pick)
    assert Cp.shape == (4, T, n, n)
    for c, t in enumerate(pick):
        assert np.array_equal(Cp[c], Cc[t]), (c, t)
    ctx.close()


def test_tiles():
    T, n, R = 7, 4, 1100                                        # tile length 3, last tile ragged (2 right-hand sides)
    D, U, A, _ = problem(T, n)
    B = np.random.default_rng(11).standard_normal((R, T, n))
    ref = np.linalg.solve(A, B.reshape(R, -1).T).T.reshape(R, T, n)
    for lds in (1, 0):
        ctx = ctx_for(T, n, lds)
        X = ctx.bt_solve_multi(D, U, B)
        err = rel(X, ref)
        print("tiles", lds, err)
        assert err <= TOL, err
        assert np.array_equal(ctx.bt_solve_multi(D, U, B[1097:1100]), X[1097:1100])
        assert np.array_equal(ctx.bt_solve_multi(D, U, B), X)
        ctx.close()


def block_matvec(D, U, X):
    """Lambda X for X [R][T][n]."""
    Y = np.einsum("tij,rtj->rti", D, X)
    Y[:, :-1] += np.einsum("tij,rtj->rti", U, X[:, 1:])
    Y[:, 1:] += np.einsum("tji,rtj->rti", U, X[:, :-1])
    return Y


@pytest.mark.parametrize("T,n", [(1025, 6), (4097, 12)])         # the second is on the output-buffer path by size
def test_full_size_forward_error(T, n):
    D, U, _ = random_chain(T, n, T)
    Xt = np.random.default_rng(T).standard_normal((16, T, n))
    B = block_matvec(D, U, Xt)
    ctx = ctx_for(T, n)
    X = ctx.bt_solve_multi(D, U, B)
    err = rel(X, Xt)
    print("forward error", T, n, err)
    assert err <= TOL, err
    ctx.close()


def test_not_positive_definite_gives_nan():
    T, n = 5, 3
    D, U, _ = random_chain(T, n, 3)
    Dbad = D.copy()
    Dbad[2] = -np.eye(n)
    for lds in (1, 0):
        ctx = ctx_for(T, n, lds)
        X = ctx.bt_solve_multi(Dbad, U, np.ones((4, T, n)))
        assert X.shape == (4, T, n) and np.all(np.isnan(X))
        Cc = ctx.bt_cov_columns(Dbad, U, [0, 4, 2])
        assert Cc.shape == (3, T, n, n) and np.all(np.isnan(Cc))
        ctx.close()


def test_status_codes():
    T, n = 5, 3
    D, U, mu = random_chain(T, n, 3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    B, X = np.ones((4, T, n)), np.empty((4, T, n))
    nodes = np.array([0, 4], dtype=np.int32)
    Cc = np.empty((2, T, n, n))
    fresh = api.Context(0)                        # no gvi_chain_set yet
    assert fresh.lib.gvi_bt_solve_multi(fresh.h, p(D), p(U), 4, p(B), p(X)) == 5
    assert fresh.lib.gvi_bt_cov_columns(fresh.h, p(D), p(U), 2, p(nodes), p(Cc)) == 5
    assert fresh.lib.gvi_ngd_cov_columns(fresh.h, 2, p(nodes), p(Cc)) == 5
    assert fresh.lib.gvi_ngd_cov_columns_dev(fresh.h, 2, p(nodes), p(Cc)) == 5
    fresh.close()
    ctx = ctx_for(T, n)
    lib, h = ctx.lib, ctx.h
    assert lib.gvi_bt_solve_multi(h, p(D), p(U), 0, p(B), p(X)) == 0
    assert lib.gvi_bt_solve_multi(h, p(D), p(U), -1, p(B), p(X)) == 1
    assert lib.gvi_bt_solve_multi(h, None, p(U), 4, p(B), p(X)) == 1
    assert lib.gvi_bt_solve_multi(h, p(D), None, 4, p(B), p(X)) == 1
    assert lib.gvi_bt_solve_multi(h, p(D), p(U), 4, None, p(X)) == 1
    assert lib.gvi_bt_solve_multi(h, p(D), p(U), 4, p(B), None) == 1
    assert lib.gvi_bt_cov_columns(h, p(D), p(U), 0, p(nodes), p(Cc)) == 0
    assert lib.gvi_bt_cov_columns(h, p(D), p(U), -1, p(nodes), p(Cc)) == 1
    assert lib.gvi_bt_cov_columns(h, None, p(U), 2, p(nodes), p(Cc)) == 1
    assert lib.gvi_bt_cov_columns(h, p(D), p(U), 2, None, p(Cc)) == 1
    assert lib.gvi_bt_cov_columns(h, p(D), p(U), 2, p(nodes), None) == 1
    for bad in (T, -1):
        nb = np.array([0, bad], dtype=np.int32)
        assert lib.gvi_bt_cov_columns(h, p(D), p(U), 2, p(nb), p(Cc)) == 1
    # the resident forms: before gvi_ngd_init, then the same argument checks
    assert lib.gvi_ngd_cov_columns(h, 2, p(nodes), p(Cc)) == 5
    assert lib.gvi_ngd_cov_columns_dev(h, 2, p(nodes), p(Cc)) == 5
    ctx.ngd_init(mu, D, U)
    for fn in (lib.gvi_ngd_cov_columns, lib.gvi_ngd_cov_columns_dev):
        assert fn(h, 0, p(nodes), p(Cc)) == 0
        assert fn(h, -1, p(nodes), p(Cc)) == 1
        assert fn(h, 2, None, p(Cc)) == 1
        assert fn(h, 2, p(nodes), None) == 1
        assert fn(h, 2, p(np.array([0, T], dtype=np.int32)), p(Cc)) == 1
    assert lib.gvi_ngd_cov_columns(h, 2, p(nodes), p(Cc)) == 0
    assert np.array_equal(Cc, ctx.bt_cov_columns(D, U, nodes))
    ctx.close()
    big = ctx_for(3, 17)
    Db, Ub, _ = random_chain(3, 17, 1)
    Bb, Xb = np.ones((1, 3, 17)), np.empty((1, 3, 17))
    n1 = np.array([1], dtype=np.int32)
    Cb = np.empty((1, 3, 17, 17))
    assert big.lib.gvi_bt_solve_multi(big.h, p(Db), p(Ub), 1, p(Bb), p(Xb)) == 3
    assert big.lib.gvi_bt_cov_columns(big.h, p(Db), p(Ub), 1, p(n1), p(Cb)) == 3
    big.close()


def _resident(name, columns_between):
    ch = syn.make_chain(name)
    ctx, _ = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    steps = []
    for i in range(4):
        steps.append(ctx.ngd_step(0.55, 10))
        if columns_between:
            ctx.ngd_cov_columns([i, ctx.T - 1])
    return ctx, steps


@pytest.mark.parametrize("name", ["c2", "planar"])
def test_resident_state_columns(name):
    import torch
    ctx, steps = _resident(name, True)
    st = ctx.ngd_get_state()
    nodes = [ctx.T - 1, 0, ctx.T // 2, 0]
    Cc = ctx.ngd_cov_columns(nodes)
    assert np.array_equal(Cc, ctx.bt_cov_columns(st["D"], st["U"], nodes))
    buf = torch.full((len(nodes), ctx.T, ctx.n, ctx.n), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ngd_cov_columns_dev(nodes, buf.data_ptr())
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), Cc)
    # the calls between the steps leave the iteration bit-identical
    ref, ref_steps = _resident(name, False)
    assert steps == ref_steps
    st_ref = ref.ngd_get_state()
    for k in ("mu", "D", "U", "SigD", "SigU"):
        assert np.array_equal(st[k], st_ref[k]), k
    assert ctx.ngd_counters() == ref.ngd_counters()
    ctx.close()
    ref.close()


def test_shim_solve_matches_binding(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "solve_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "solve_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    v = {}
    for line in r.stdout.splitlines():
        tok = line.split()
        v[tok[0]] = tok[1:]
    T, n, R, ci, cj = (int(v["T"][i]) for i in (0, 2, 4, 6, 8))
    states = [int(s) for s in v["states"]]
    nc = len(states)
    D = np.array(v["D"], dtype=float).reshape(T, n, n)
    U = np.array(v["U"], dtype=float).reshape(T - 1, n, n)
    B = np.array(v["B"], dtype=float).reshape(R, T, n)              # printed one right-hand side after the other
    X = np.array(v["X"], dtype=float).reshape(R, T, n)
    Xf = np.array(v["Xf"], dtype=float).reshape(R, T, n)
    Cc = np.array(v["C"], dtype=float).reshape(nc, n, T, n).transpose(0, 2, 3, 1)    # column c n + k, row t n + r -> [c][t][r][k]
    Cf = np.array(v["Cf"], dtype=float).reshape(nc, n, T, n).transpose(0, 2, 3, 1)
    Cij = np.array(v["Cij"], dtype=float).reshape(n, n).T
    ctx = ctx_for(T, n)
    assert np.array_equal(X, ctx.bt_solve_multi(D, U, B))
    assert np.array_equal(Xf, X)
    ref = ctx.bt_cov_columns(D, U, states)
    assert np.array_equal(Cc, ref)
    assert np.array_equal(Cf, Cc)
    assert np.array_equal(Cij, ctx.bt_cov_columns(D, U, [cj])[0][ci])
    ctx.close()
