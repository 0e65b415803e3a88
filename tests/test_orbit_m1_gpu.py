"""The odd part of psi on the sign-orbit route (kernels_orbit.hpp, orbit_wave): m1[c] = tau2[c] a_c, a_c = sum_r s_r u0_r H[r][c],
formed once per factor behind the walk by chunk 0 -- the walk itself evaluates the even scalar only.

Per shape (every body of the walk runs: grouped s <= 3, the register-column and the LDS-column s = 4 bodies at m = 2 / 6,
orbit_walk_split at m = 12, m = 12 with s <= 3, and the SIGNED instances; K is no multiple of 4):
  * Vdmu against the lane-per-point kernels (option orbit 0) and against oracle.batched_moments, at the tolerances of
    test_gpu_parity.py::test_sign_orbit_kernel_vs_lane_per_point_and_oracle (1e-10 at p <= 5, 1e-8 above);
  * Vdmu BIT-identical under orbit_copies 1 / 8 / 16 and orbit_waves 64 / 100000: m1 depends on neither any more, so a value
    written by the wrong chunk, written twice or left in an accumulator is a differing word;
  * mu = mu0 on the fixed-prior kind with u0 = 0: Vdmu is exactly 0.0.  The prep forms u0 = b + A mu with b = -A mu0 stored
    per factor, which is zero only up to rounding for a general mu0 (1e-17 in Vdmu, measured); mu0 = mu = 0 makes it the
    exact zero the check is about, so the fixed-prior shapes run a second set with mu0 = 0;
  * E_phi, Vddmu and the costs run-to-run bit-identical.
The one-launch factor pass (factor_fused_kernel) against the three launches on the T = 9, n = 6 chain: three NGD steps, the
tolerances of test_ngd_schedule_gpu.py for these two routes."""
import numpy as np
import pytest

import gvi_oracle as o
import test_gpu_parity as parity
from chains import make_chain, oracle_table
from gaussianvi_amd import api, synthetic as syn

pytestmark = pytest.mark.gpu

SHAPES = [("fixed", 2, 2, 3, 5), ("quad", 4, 2, 5, 7), ("fixed", 6, 6, 5, 7), ("quad", 12, 6, 5, 5), ("fixed", 12, 12, 5, 3),
          ("quad", 24, 12, 4, 3), ("indef", 12, 6, 4, 5), ("indef", 24, 12, 5, 3)]
ALTERNATIVES = [("orbit_copies", 1), ("orbit_copies", 8), ("orbit_copies", 16), ("orbit_waves", 64), ("orbit_waves", 100000)]


def problem(kind, d, m, p, K):
    """-> (psi kind, state dimension, parameters, oracle psi, the parameters with mu0 = 0 (fixed prior) or None, mu, Sigma)"""
    rng = np.random.default_rng(9100 + 10 * d + p)
    at_zero = None
    if kind == "fixed":
        mu0 = rng.normal(size=(K, d))
        Kh = rng.normal(size=(K, d, d))
        Kinv = Kh @ np.transpose(Kh, (0, 2, 1)) / d + 0.3 * np.eye(d)
        psi_kind, n, params, psi = api.PSI_FIXED_PRIOR, d, np.concatenate([mu0, Kinv.reshape(K, -1)], axis=1), o.psi_batch_fixed_prior(mu0, Kinv)
        at_zero = np.concatenate([np.zeros((K, d)), Kinv.reshape(K, -1)], axis=1)
    else:
        n = d // 2
        Phi, Qinv = parity.quad_params(rng, K, n)
        if kind == "indef":
            Qh = rng.normal(size=(K, n, n))
            Qinv = 0.5 * (Qh + np.transpose(Qh, (0, 2, 1)))
            ev = np.linalg.eigvalsh(Qinv)
            assert (ev.min(axis=1) < 0).all() and (ev.max(axis=1) > 0).all()
        psi_kind, params, psi = api.PSI_QUAD_PRIOR, np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1), o.psi_batch_quad_prior(Phi, Qinv)
    assert m == n
    mu, Sigma = syn.random_marginals(rng, K, d, 0.3)
    return psi_kind, n, params, psi, at_zero, mu, Sigma


@pytest.mark.parametrize("kind,d,m,p,K", SHAPES)
def test_m1_of_the_orbit_route(kind, d, m, p, K):
    psi_kind, n, params, psi, at_zero, mu, Sigma = problem(kind, d, m, p, K)
    ctx, sid = parity.single_set_ctx(psi_kind, d, n, p, K, params)
    got = ctx.moments(sid, mu, Sigma)
    cost = ctx.costs(sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] == 6
    again = ctx.moments(sid, mu, Sigma)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)) and np.array_equal(cost, ctx.costs(sid, mu, Sigma))
    differing = {}
    for name, value in ALTERNATIVES:
        ctx.set_option(name, value)
        alt = ctx.moments(sid, mu, Sigma)
        assert ctx.profile_geometry(sid)["variant"] == 6
        differing[(name, value)] = int(np.count_nonzero(alt[1] != got[1]))
    print(f"{kind} d={d} m={m} p={p}: Vdmu words that differ from the default launch {differing}")
    ctx.set_option("orbit", 0)
    base = ctx.moments(sid, mu, Sigma)
    assert ctx.profile_geometry(sid)["variant"] != 6
    ctx.close()
    zero = None
    if at_zero is not None:
        ctx, sid = parity.single_set_ctx(psi_kind, d, n, p, K, at_zero)
        zero = ctx.moments(sid, np.zeros((K, d)), Sigma)[1]
        assert ctx.profile_geometry(sid)["variant"] == 6
        ctx.close()
    Z, w = oracle_table(d, p)
    ref = o.batched_moments(Z, w, mu, Sigma, psi, np.ones(K))
    tol = 1e-10 if p <= 5 else 1e-8
    gaps = parity.rel(got[1], base[1]), parity.rel(got[1], ref["Vdmu"])
    print(f"    Vdmu against the lane-per-point route {gaps[0]:.2e}, against the oracle {gaps[1]:.2e} (bound {tol:.0e})")
    assert not any(differing.values()), differing
    assert gaps[0] < tol and gaps[1] < tol, gaps
    if zero is not None:
        assert zero.shape == (K, d) and not zero.any(), zero


def run_steps(options):
    ch = make_chain("c3mini")
    assert (ch["T"], ch["n"]) == (9, 6) and [s["d"] for s in ch["specs"]] == [12, 6] and all(s["p"] == 5 for s in ch["specs"])
    ctx, _ = api.context_for_chain(ch)
    for name in options:
        ctx.set_option(name, 0)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    records = [ctx.ngd_step(0.55) for _ in range(3)]
    state = ctx.ngd_get_state()
    ctx.close()
    return records, state


def test_fused_pass_against_the_three_launches():
    (one, one_state), (three, three_state) = run_steps(()), run_steps(("fused",))
    for x, y in zip(one, three):
        print(f"    cost_iter {x['cost_iter']!r} / {y['cost_iter']!r}  new_cost {x['new_cost']!r} / {y['new_cost']!r}")
    for k in one_state:
        if one_state[k].size:
            print(f"    state {k}: {parity.rel(one_state[k], three_state[k]):.2e}")
    assert len(one) == len(three) == 3
    for x, y in zip(one, three):
        assert x["accepted"] == y["accepted"] and x["ntrials"] == y["ntrials"]
        assert np.isclose(x["cost_iter"], y["cost_iter"], rtol=1e-12, atol=0.0)
        assert np.isclose(x["new_cost"], y["new_cost"], rtol=1e-12, atol=0.0)
    for k in one_state:
        if one_state[k].size:
            assert parity.rel(one_state[k], three_state[k]) < 1e-10, k
