"""CPU checks of the samplers' boundary: the Python restatement of the generator (include/gvi_hip.h, "samples of q")
reproduces the Random123 Philox4x32-10 known answers, GVIGH::sample / GVIGH::log_density compile against the shim, and the
float64 restatement of the sweep (tests/sample_ref.py) is proven at every shape tests/test_sample_sweep_gpu.py compares the device
with: against the dense inverse up to T n = 600, through F^T Lambda F = I on random vectors above, with the conditioning of
every dense matrix formed."""
import math
import os
import subprocess

import numpy as np
import pytest

import sample_ref as sr
from gaussianvi_amd import build
from test_solve_host import SHAPES, cr_factor, dense, random_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
    return c0, c1, c2, c3


def randn(seed, first, count):
    """Normal numbers first .. first + count - 1 of stream `seed`: the generator gvi_randn / gvi_bt_sample use."""
    out = np.empty(count)
    key = (seed & M32, (seed >> 32) & M32)
    for i in range(first, first + count):
        c = i >> 1
        w = philox4x32_10((c & M32, (c >> 32) & M32, 0, 0), key)
        u1 = (((w[0] | w[1] << 32) >> 11) + 0.5) * 2.0 ** -53
        u2 = (((w[2] | w[3] << 32) >> 11) + 0.5) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        out[i - first] = r * (math.cos(2 * math.pi * u2) if i % 2 == 0 else math.sin(2 * math.pi * u2))
    return out


def test_philox_known_answers():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_restated_generator_is_split_invariant_and_standard():
    z = randn(7, 3, 4000)
    assert np.array_equal(z[10:20], randn(7, 13, 10))           # number i depends on (seed, i) only
    assert not np.array_equal(z[:100], randn(8, 3, 100))
    assert abs(z.mean()) < 6 / math.sqrt(len(z)) and abs(z.var() - 1.0) < 6 * math.sqrt(2.0 / len(z))


# ---- the per-entry reference of the sweep (tests/sample_ref.py) at every shape tests/test_sample_sweep_gpu.py uses ----
_SHAPES = sorted(set(sr.gpu_shapes()) | set(SHAPES))
SMALL = [s for s in _SHAPES if s[0] * s[1] <= sr.SMALL_TN]
LARGE = [s for s in _SHAPES if s[0] * s[1] > sr.SMALL_TN]
DENSE_LOGDET_TN = 1600
REF_TOL = 1e-13                      # three orders inside the 1e-10 of the GPU tests
COND_MAX = 1e2


def _cond(A):
    w = np.linalg.eigvalsh(A)
    assert w[0] > 0
    return w[-1] / w[0]


@pytest.mark.parametrize("T,n", SMALL)
def test_reference_sweep_gives_the_dense_covariance(T, n):
    D, U, _ = random_chain(T, n, 100 + T * n)
    A = dense(D, U)
    assert _cond(A) <= COND_MAX
    N = T * n
    F = sr.cr_sample(D, U, np.eye(N).reshape(N, T, n)).reshape(N, N).T       # column j = the draw from eps = e_j
    Sig = np.linalg.inv(A)
    err = np.abs(F @ F.T - Sig).max() / np.abs(Sig).max()
    assert err <= REF_TOL, err
    sgn, ld = np.linalg.slogdet(A)
    assert sgn > 0 and abs(sr.half_logdet(D, U) - 0.5 * ld) <= REF_TOL * max(1.0, abs(0.5 * ld))


@pytest.mark.parametrize("T,n", LARGE)
def test_reference_sweep_keeps_the_quadratic_form(T, n):
    """F^T Lambda F = I on random vectors: y^T Lambda y = |eps|^2 and y_i^T Lambda y_j = eps_i . eps_j, no dense matrix."""
    D, U, _ = random_chain(T, n, 100 + T * n)
    fac = cr_factor(D, U)
    eps = np.random.default_rng(T + n).standard_normal((3, T, n))
    Y = sr.cr_sample(D, U, eps, fac).reshape(3, -1)
    G = Y @ sr.block_matvec(D, U, Y.reshape(3, T, n)).reshape(3, -1).T
    E = eps.reshape(3, -1) @ eps.reshape(3, -1).T
    err = np.abs(G - E).max() / np.abs(E).max()
    assert err <= REF_TOL, err
    if T * n <= DENSE_LOGDET_TN:
        A = dense(D, U)
        assert _cond(A) <= COND_MAX
        sgn, ld = np.linalg.slogdet(A)
        assert sgn > 0 and abs(sr.half_logdet(D, U, fac) - 0.5 * ld) <= REF_TOL * abs(0.5 * ld)


def test_restated_sweep_plan():
    """The plan's own arithmetic at its edges (the GPU cases assert the rows they were written for against it)."""
    assert sr.sweep_plan(1, 1, 1) == (True, 1) and sr.sweep_plan(512, 7, 4) == (True, 1) and sr.sweep_plan(513, 7, 4) == (True, 2)
    assert sr.sweep_plan(4096, 7, 4) == (True, 8) and sr.sweep_plan(10 ** 6, 7, 4) == (True, 8)
    assert sr.sweep_plan(10 ** 6, 640, 16) == (True, 1) and sr.sweep_plan(3, 641, 16) == (False, 1)
    assert sr.sweep_plan(10 ** 6, 641, 16) == (False, 8)
    for T, n, S, lds, tile, last in sr.LDS_TILES + sr.LDS_CAPPED + sr.BOUNDARY + sr.BUFFER_TILES + sr.GENERATED + sr.NOT_PD:
        assert sr.sweep_plan(S, T, n) == (lds, tile) and sr.last_tile(S, tile) == last, (T, n, S)


def test_sample_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "sample_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "sample_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
