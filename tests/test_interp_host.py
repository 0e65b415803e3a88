"""CPU checks of the dense-time posterior's boundary (include/gvi_hip.h, "dense-time posterior"): the interpolation identity
against a dense fine-grid chain, the semidefinite Cholesky rule of kernels_interp.hpp restated in numpy, the ctypes table, and
MinimumAccGP::interpolation / GVIGH::set_interpolation / interpolate / sample_interpolated compiling against the shim."""
import os
import subprocess

import numpy as np
import pytest

from gaussianvi_amd import _lib, build, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gvi_interp_set", "gvi_interp_info", "gvi_bt_interp", "gvi_ngd_interp", "gvi_ngd_interp_dev", "gvi_bt_interp_samples",
         "gvi_ngd_sample_interp", "gvi_ngd_sample_interp_dev"]
QC, DT = 0.8, 0.37
FINE_SHAPES = [(1, 3, 2), (2, 5, 4), (3, 9, 3), (8, 2, 2)]


def semidefinite_cholesky(Qt):
    """The rule of interp_prepare_kernel: (L, bad) from the lower triangle of Qt."""
    n = Qt.shape[0]
    L = np.zeros((n, n))
    bad = False
    for k in range(n):
        qkk = Qt[k, k]
        p = qkk - np.sum(L[k, :k] ** 2)
        thr = 64.0 * 2.0 ** -52 * qkk
        if np.isnan(p) or p < -thr or qkk < 0:
            bad = True
        elif p > thr:
            d = np.sqrt(p)
            L[k, k] = d
            for i in range(k + 1, n):
                L[i, k] = (Qt[i, k] - np.sum(L[i, :k] * L[k, :k])) / d
    return L, bad


def prior_chain(nd, N, h, rng, every):
    """Dense precision and information vector of N constant-velocity states at spacing h, with a random SPD likelihood block
    and a linear term on every `every`-th node (drawn in node order, so a fine and a coarse chain get the same ones)."""
    n = 2 * nd
    Phi, Qinv = synthetic._minacc(nd, QC, h)
    Lam = np.zeros((N * n, N * n))
    eta = np.zeros(N * n)
    G = np.hstack([-Phi, np.eye(n)])
    M = G.T @ Qinv @ G
    for k in range(N - 1):
        Lam[k * n:(k + 2) * n, k * n:(k + 2) * n] += M
    for k in range(0, N, every):
        W = rng.standard_normal((n, n))
        Lam[k * n:(k + 1) * n, k * n:(k + 1) * n] += W @ W.T / n + 0.5 * np.eye(n)
        eta[k * n:(k + 1) * n] += rng.standard_normal(n)
    return Lam, eta


@pytest.mark.parametrize("nd,T,m", FINE_SHAPES)
def test_fine_chain_identity(nd, T, m):
    """q of a fine chain whose likelihood terms sit on every m-th node, at EVERY fine node, equals the three formulas applied to
    the coarse chain's marginals: mean, covariance, and -- what the sample formula x = A x_i + B x_i+1 + c + L eps implies --
    the cross-covariance with the left support state."""
    n = 2 * nd
    Nf = (T - 1) * m + 1
    Lf, ef = prior_chain(nd, Nf, DT / m, np.random.default_rng(7 * nd + T), m)
    Lc, ec = prior_chain(nd, T, DT, np.random.default_rng(7 * nd + T), 1)
    Sf, Sc = np.linalg.inv(Lf), np.linalg.inv(Lc)
    mf, mc = Sf @ ef, Sc @ ec
    worst = 0.0
    for i in range(T - 1):
        Sii = Sc[i * n:(i + 1) * n, i * n:(i + 1) * n]
        Sij = Sc[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n]
        Sjj = Sc[(i + 1) * n:(i + 2) * n, (i + 1) * n:(i + 2) * n]
        for j in range(m + 1):
            tau = DT if j == m else j * (DT / m)
            A, B, Qt = synthetic.minacc_interpolation(nd, QC, DT, tau)
            f = i * m + j
            mean = A @ mc[i * n:(i + 1) * n] + B @ mc[(i + 1) * n:(i + 2) * n]
            ASB = A @ Sij @ B.T
            cov = A @ Sii @ A.T + ASB + ASB.T + B @ Sjj @ B.T + Qt
            cross = A @ Sii + B @ Sij.T
            rm, rc = mf[f * n:(f + 1) * n], Sf[f * n:(f + 1) * n, f * n:(f + 1) * n]
            rx = Sf[f * n:(f + 1) * n, i * m * n:(i * m + 1) * n]
            worst = max(worst, np.abs(mean - rm).max() / np.abs(mf).max(), np.abs(cov - rc).max() / np.abs(Sf).max(),
                        np.abs(cross - rx).max() / np.abs(Sf).max())
    print(f"fine-chain identity (nd={nd}, T={T}, m={m}): worst relative difference {worst:.3e}")
    assert worst <= 1e-11, worst


def test_end_points_are_exact():
    for nd in (1, 3):
        n = 2 * nd
        A, B, Qt = synthetic.minacc_interpolation(nd, QC, DT, 0.0)
        assert np.array_equal(A, np.eye(n)) and not B.any() and not Qt.any()
        A, B, Qt = synthetic.minacc_interpolation(nd, QC, DT, DT)
        assert not A.any() and np.array_equal(B, np.eye(n)) and not Qt.any()


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
def test_cholesky_rule_on_interior_operators(nd):
    for frac in (0.25, 1 / 3, 0.5, 0.75):
        Qt = synthetic.minacc_interpolation(nd, QC, DT, frac * DT)[2]
        assert np.linalg.eigvalsh(Qt).min() / np.abs(Qt).max() > 1e-6      # the rule never triggers here
        L, bad = semidefinite_cholesky(Qt)
        assert not bad and (np.diag(L) > 0).all()
        assert np.abs(L @ L.T - Qt).max() <= 1e-14 * np.abs(Qt).max()
        assert np.abs(L - np.linalg.cholesky(Qt)).max() <= 1e-12 * np.abs(L).max()


def test_cholesky_rule_degenerate_inputs():
    n = 5
    L, bad = semidefinite_cholesky(np.zeros((n, n)))
    assert not bad and not L.any()                                          # exactly zero
    v = np.array([0.7, -1.3, 0.2, 2.1, -0.4])
    L, bad = semidefinite_cholesky(np.outer(v, v))
    assert not bad and not L[:, 1:].any()                                   # L = [v, 0, ...]
    assert np.abs(L[:, 0] - v).max() <= 1e-15 * np.abs(v).max()
    # noise in two of four directions only (zero rows and columns): zero columns there, still a factor
    M = np.zeros((4, 4))
    M[np.ix_([0, 2], [0, 2])] = [[2.0, 0.6], [0.6, 1.0]]
    L, bad = semidefinite_cholesky(M)
    assert not bad and not L[:, [1, 3]].any() and np.abs(L @ L.T - M).max() <= 1e-15 * np.abs(M).max()
    # indefinite, negative diagonal, NaN: bad
    assert semidefinite_cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))[1]
    assert semidefinite_cholesky(np.diag([1.0, -1e-3]))[1]
    assert semidefinite_cholesky(np.array([[1.0, 0.0], [0.0, np.nan]]))[1]


def test_signatures_are_bound():
    for name in NAMES:
        assert name in _lib.SIGNATURES, name


def test_interp_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "interp_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "interp_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the Python helper's numbers for MinimumAccGP::interpolation to reproduce
    nd, taus = 3, [0.0, 0.1 * DT, 0.5 * DT, 0.93 * DT, DT]
    lines = [f"{nd} {QC!r} {DT!r} {len(taus)}"]
    for tau in taus:
        ops = synthetic.minacc_interpolation(nd, QC, DT, tau)
        lines.append(repr(tau) + " " + " ".join(repr(float(x)) for M in ops for x in M.reshape(-1)))
    path = tmp_path / "operators.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "host", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernels_on_cpu_under_sanitizers(tmp_path):
    """kernels_interp.hpp compiled for the CPU, one thread per lane, under AddressSanitizer and UBSan, against a plain reference
    (tests/stubs/interp_kernels_on_cpu.cpp): the arithmetic and every index of the three kernels without a device."""
    exe = str(tmp_path / "interp_kernels_on_cpu")
    cmd = ["g++", "-std=c++20", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "tests", "stubs", "hip_on_cpu"), "-I", os.path.join(ROOT, "gaussianvi_amd", "csrc"),
           os.path.join(ROOT, "tests", "stubs", "interp_kernels_on_cpu.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout + r.stderr
