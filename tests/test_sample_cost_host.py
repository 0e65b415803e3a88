"""CPU checks of the boundary of "costs of sampled trajectories" (include/gvi_hip.h): the ctypes table, the shim methods and
the example compiling, and a numpy restatement of the clearance of every hinge-on-SDF kind that is consistent with the
oracle's psi (tests/test_sample_cost_gpu.py checks the device against it)."""
import os
import subprocess

import numpy as np
import pytest

import gvi_oracle as o
from chains import make_chain
from gaussianvi_amd import _lib, build, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gvi_sample_factor_costs", "gvi_sample_clearance", "gvi_sample_clearance_dev", "gvi_sample_costs", "gvi_sample_costs_dev",
         "gvi_ngd_sample_costs", "gvi_ngd_sample_costs_dev"]
OBSTACLE_CHAINS = ["planar", "quad2d", "pr3d", "arm7"]


def factor_slices(X, spec, n):
    """Xk [K][S][d]: Xk[k, s] = X[s].reshape(-1)[start_k n : start_k n + d], the slice gvi_gather_marginals takes."""
    S = X.shape[0]
    flat = X.reshape(S, -1)
    return np.stack([flat[:, int(st) * n:int(st) * n + spec["d"]] for st in spec["start"]])


def check_points(spec, Xk):
    """(sd [K][S][B], r [K][B] or [B]): signed distance at every check point b of every (factor, sample), and the radius of
    its ball -- the points of the kind's psi, from the oracle's look-ups and forward kinematics."""
    kind, P = spec["kind"], spec["params"]
    org, cell, field = spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"]
    if kind == syn.PSI_HINGE_SDF_2D:
        return o.planar_sdf_lookup(Xk[:, :, 0], Xk[:, :, 1], org, cell, field)[:, :, None], P[:, 2][:, None]
    if kind == syn.PSI_HINGE_SDF_3D:
        return o.sdf3d_lookup(Xk[:, :, 0], Xk[:, :, 1], Xk[:, :, 2], org, cell, field)[:, :, None], P[:, 2][:, None]
    if kind == syn.PSI_HINGE_SDF_2D_BODY:
        px, pz, phi = Xk[:, :, 0], Xk[:, :, 1], Xk[:, :, 2]
        r, nb, L = (P[:, j][:, None] for j in (2, 4, 5))
        lx = px - (L - r * 1.5) * np.cos(phi) / 2.0
        lz = pz - (L - r * 1.5) * np.sin(phi) / 2.0
        sd = [o.planar_sdf_lookup(lx + L * np.cos(phi) / nb * i, lz + L * np.sin(phi) / nb * i, org, cell, field)
              for i in range(int(P[0, 4]))]
        return np.stack(sd, axis=-1), np.repeat(P[:, 2][:, None], len(sd), axis=1)
    if kind == syn.PSI_HINGE_SDF_3D_ARM:
        arm = spec["arm"]
        nb = min(Xk.shape[-1], len(arm["radii"]))
        pts = o.arm_sphere_centers(Xk, arm["a"], arm["alpha"], arm["d"], arm["theta_bias"], arm["frames"][:nb], arm["centers"][:nb])
        sd = [o.sdf3d_lookup(pts[:, :, i, 0], pts[:, :, i, 1], pts[:, :, i, 2], org, cell, field) for i in range(nb)]
        return np.stack(sd, axis=-1), np.asarray(arm["radii"][:nb])
    raise ValueError(kind)


def clearance_ref(spec, Xk):
    """clr [K][S] = min_b sd_b - r_b."""
    sd, r = check_points(spec, Xk)
    r = r[:, None, :] if r.ndim == 2 else r[None, None, :]
    return (sd - r).min(axis=-1)


def psi_from_check_points(spec, Xk):
    """psi [K][S] = sigma sum_b hinge(eps + r_b - sd_b)^2 slope^2 from the SAME sd_b the clearance uses."""
    sd, r = check_points(spec, Xk)
    P = spec["params"]
    r = r[:, None, :] if r.ndim == 2 else r[None, None, :]
    sig, eps = P[:, 0][:, None, None], P[:, 1][:, None, None]
    slope = P[:, 3][:, None, None] if spec["kind"] == syn.PSI_HINGE_SDF_2D_BODY else 1.0
    thr = eps + r
    err = np.where(sd > thr, 0.0, (thr - sd) * slope)
    return (err * err * sig).sum(axis=-1)


def numpy_samples(ch, S, seed):
    """S draws [S][T][n] of N(mu0, (D0, U0)^-1) by a dense Cholesky factor (host only)."""
    T, n = ch["T"], ch["n"]
    Lam = np.zeros((T * n, T * n))
    for t in range(T):
        Lam[t * n:(t + 1) * n, t * n:(t + 1) * n] = ch["D0"][t]
        if t + 1 < T:
            Lam[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = ch["U0"][t]
            Lam[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = ch["U0"][t].T
    C = np.linalg.cholesky(np.linalg.inv(Lam))
    z = np.random.default_rng(seed).standard_normal((S, T * n))
    return (ch["mu0"].reshape(-1) + z @ C.T).reshape(S, T, n)


def test_signatures_are_bound():
    for name in NAMES:
        assert name in _lib.SIGNATURES, name


@pytest.mark.parametrize("name", OBSTACLE_CHAINS)
def test_clearance_restatement_is_consistent_with_the_oracle_psi(name):
    ch = make_chain(name)
    spec = ch["specs"][1]
    Xk = factor_slices(numpy_samples(ch, 64, 11), spec, ch["n"])
    ref = spec["psi_batch"](Xk)
    got = psi_from_check_points(spec, Xk)
    assert ref.max() > 0 and (ref == 0).any()                           # both hinge branches
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name}: psi from the clearance's check points vs psi_batch: {err:.3e}")
    assert err <= 1e-13, err
    clr = clearance_ref(spec, Xk)
    eps = spec["params"][:, 1][:, None]
    assert np.array_equal(ref > 0, clr < eps)                           # psi > 0 exactly where the clearance is below epsilon


def test_callsite_and_example_compile_against_the_shim(tmp_path):
    build.build_lib()
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    link = ["-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip", "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd")]
    exe = str(tmp_path / "sample_cost_callsite")
    r = subprocess.run(common + [os.path.join(ROOT, "tests", "stubs", "sample_cost_callsite.cpp")] + link + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run(common + [os.path.join(ROOT, "examples", "planar_example.cpp")] + link + ["-o", str(tmp_path / "planar_example")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
