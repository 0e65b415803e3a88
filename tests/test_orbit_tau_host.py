"""Host side of the odd part of psi on the sign-orbit route (gaussianvi_amd/csrc/orbits.hpp, kernels_orbit.hpp: m1[c] =
tau2[c] a_c): build_orbits' tau2 against math.fsum over the oracle's full table, as a plain build and under
AddressSanitizer / UndefinedBehaviorSanitizer (tests/stubs/orbit_tau.cpp, a stand-alone program), and the per-orbit identity
the kernel rests on, restated in float64.

tau2 / 2 = sum_k w_k z_kc^2 cancels by ~1e4 at (12,5) (sum |w| = 1.2e4, the sum is 1): build_orbits forms the terms as
(w z) z -- as the reference sum below does, so both add the SAME float64 terms, 2^s equal ones per orbit -- and adds them
with Neumaier's compensated sum, whose error is one rounding of the result plus ~n^2 eps^2 sum |term| (n <= 2e4 terms: 4e-20
relative to sum |term| ~ 1e4, far below an ulp of 1).  Bound: 4 ulp; a plain sum misses it (checked below at (12,5))."""
import math
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "orbit_tau.cpp")
CASES = [(2, 3), (4, 5), (6, 5), (12, 5), (8, 6), (24, 4)]
BUILDS = {"plain": ["g++", "-O2", "-std=c++17"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def reference_tau(Z, w):
    """-> [d] correctly rounded sum_k (w_k z_kc) z_kc"""
    terms = (w[:, None] * Z) * Z
    return np.array([math.fsum(terms[:, c]) for c in range(Z.shape[1])])


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_tau2_against_fsum_over_the_oracle_table(tmp_path, build):
    exe = str(tmp_path / "orbit_tau")
    r = subprocess.run(BUILDS[build] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for d, p in CASES:
        Z, w = o.nwspgr_cached(d, p)
        Z, w = np.ascontiguousarray(Z, dtype="<f8"), np.ascontiguousarray(w, dtype="<f8")
        path = tmp_path / f"table_{d}_{p}.bin"
        path.write_bytes(Z.tobytes() + w.tobytes())
        r = subprocess.run([exe, str(path), str(d), str(len(w))], capture_output=True, text=True, env=ENV, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith(f"ok {d} {len(w)} "), r.stdout[-2000:] + r.stderr[-4000:]
        got = np.array([float.fromhex(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("tau2 ")]) / 2.0
        ref = reference_tau(Z, w)
        assert got.shape == ref.shape == (d,)
        ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
        plain = np.abs(((w[:, None] * Z) * Z).sum(axis=0) - ref) / np.spacing(np.abs(ref))
        print(f"({d},{p}) {build}: tau2 / 2 within {ulps.max():.1f} ulp of fsum; tau - 1 up to {np.abs(ref - 1).max():.1e}; "
              f"numpy's own sum {plain.max():.0f} ulp; sum |w| {np.abs(w).sum():.1e}")
        assert ulps.max() <= 4.0, (d, p, ulps)


def test_a_plain_sum_in_table_order_misses_the_bound():
    """what the compensation is for: the same terms added one after the other at (12,5)"""
    Z, w = o.nwspgr_cached(12, 5)
    terms = (w[:, None] * Z) * Z
    ref = reference_tau(Z, w)
    s = np.zeros(12)
    for row in terms:
        s = s + row
    ulps = np.abs(s - ref) / np.spacing(np.abs(ref))
    print(f"plain sum: {ulps.max():.0f} ulp")
    assert ulps.max() > 4.0


def test_half_orbit_identity_in_float64():
    """sum over the walked half orbit (sigma_{s-1} = +1, the others free) of sigma_i l(sigma) = 2^(s-1) m_i a_{c_i}, with
    l = sum_r su0_r v_r, v = sum_j sigma_j m_j H[:, c_j], a_c = sum_r su0_r H[r][c] -- for every support size of the tables
    above, every i including the fixed coordinate i = s - 1.  Bound: both sides are sums of at most n = M s 2^(s-1)
    products whose absolute values add up to B = 2^(s-1) sum_r |su0_r| sum_j m_j |H[r][c_j]|: n eps B (the first-order bound
    of a recursive sum, every product rounded once)."""
    rng = np.random.default_rng(5)
    eps = np.finfo(np.float64).eps
    seen = set()
    for d, p in CASES:
        Z, _ = o.nwspgr_cached(d, p)
        M = max(d // 2, 1)
        support = (Z != 0).sum(axis=1)
        for s in sorted(set(int(v) for v in support) - {0}):
            seen.add(s)
            row = Z[np.flatnonzero((support == s) & (Z >= 0).all(axis=1))[-1]]
            c = np.flatnonzero(row)
            m = row[c]
            H = rng.normal(size=(M, d))
            su0 = rng.normal(size=M) * rng.choice([-1.0, 1.0], size=M)
            a = np.array([sum(su0[r] * H[r, cc] for r in range(M)) for cc in c])
            odd = np.zeros(s)
            for bits in range(1 << (s - 1)):
                sigma = np.array([1.0 if (bits >> j) & 1 else -1.0 for j in range(s - 1)] + [1.0])
                v = (H[:, c] * (sigma * m)).sum(axis=1)
                odd += sigma * float(su0 @ v)
            want = 2.0 ** (s - 1) * m * a
            bound = M * s * 2 ** (s - 1) * eps * 2.0 ** (s - 1) * float(np.abs(su0) @ (np.abs(H[:, c]) @ m))
            gap = np.abs(odd - want).max()
            print(f"({d},{p}) s = {s}: |sum sigma_i l - 2^(s-1) m_i a_c| <= {gap:.2e} (bound {bound:.2e})")
            assert gap <= bound, (d, p, s, odd, want)
    assert seen == {1, 2, 3, 4, 5}, seen
