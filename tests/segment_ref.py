"""Reference psi of the obstacle factors on a segment (GVI_PSI_HINGE_SDF_2D_SEG / _3D_SEG, include/gvi_hip.h): a numpy
restatement on the oracle's own grid look-ups.  The reference project has no such factor, so nothing in oracle/ restates it.

  psi(x) = sigma * sum_j max(0, eps + r - sdf(W_j x + c_j))^2        clearance(x) = min_j sdf(W_j x + c_j) - r

params [K][3 + J P (d + 1)] = [sigma, eps, r | W_0 (P x d) | c_0 (P) | ...], P = 2 (o.planar_sdf_lookup) or 3 (o.sdf3d_lookup).
The closures take (X [K][N][d], sel) like the oracle's psi_batch_* and plug into o.batched_moments / o.FactorSet."""
import numpy as np

import gvi_oracle as o
from gaussianvi_amd import synthetic as syn

NPOS = {syn.PSI_HINGE_SDF_2D_SEG: 2, syn.PSI_HINGE_SDF_3D_SEG: 3}


def unpack(params, P, d):
    """(sigma [K], eps [K], r [K], W [K][J][P][d], c [K][J][P])."""
    params = np.asarray(params, dtype=np.float64)
    K, per = params.shape[0], P * (d + 1)
    assert (params.shape[1] - 3) % per == 0 and params.shape[1] > 3, "ragged parameter block"
    J = (params.shape[1] - 3) // per
    body = params[:, 3:].reshape(K, J, per)
    return params[:, 0], params[:, 1], params[:, 2], body[:, :, :P * d].reshape(K, J, P, d), body[:, :, P * d:]


def check_point_distances(params, P, d, origin, cell, field, X, sel=slice(None)):
    """sd [K][J][N]: the signed distance at check point j of factor k at the slice X[k, i]."""
    _, _, _, W, c = unpack(np.asarray(params)[sel], P, d)
    q = np.einsum("kjpd,knd->kjnp", W, X) + c[:, :, None, :]
    if P == 2:
        return o.planar_sdf_lookup(q[..., 0], q[..., 1], origin, cell, field)
    return o.sdf3d_lookup(q[..., 0], q[..., 1], q[..., 2], origin, cell, field)


def psi_batch_hinge_seg(params, P, d, origin, cell, field):
    def f(X, sel=slice(None)):
        sig, eps, r, _, _ = unpack(np.asarray(params)[sel], P, d)
        sd = check_point_distances(params, P, d, origin, cell, field, X, sel)
        thr = (eps + r)[:, None, None]
        err = np.where(sd > thr, 0.0, thr - sd)
        return (err * err * sig[:, None, None]).sum(axis=1)
    return f


def clearance(params, P, d, origin, cell, field, X):
    """clr [K][N] = min_j sd_j - r."""
    sd = check_point_distances(params, P, d, origin, cell, field, X)
    return (sd - np.asarray(params)[:, 2][:, None, None]).min(axis=1)


def spec_psi_batch(spec):
    return psi_batch_hinge_seg(spec["params"], NPOS[spec["kind"]], spec["d"], spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])


def spec_clearance(spec, X):
    return clearance(spec["params"], NPOS[spec["kind"]], spec["d"], spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"], X)


def attach_oracle(ch):
    """make_chain's glue (tests/chains.py) for a chain that may hold segment sets: psi_batch on every spec and oracle_sets()."""
    from chains import oracle_psi_batch
    for spec in ch["specs"]:
        spec["psi_batch"] = spec_psi_batch(spec) if spec["kind"] in NPOS else oracle_psi_batch(spec)

    def oracle_sets():
        out = []
        for spec in ch["specs"]:
            fs = o.FactorSet(spec["start"], spec["d"], spec["p"], spec["psi_batch"])
            fs.temperature = np.asarray(spec["temperature"], dtype=np.float64)
            out.append(fs)
        return out
    ch["oracle_sets"] = oracle_sets
    return ch


def sigma_point_shares(ch, spec, taus_spec=None):
    """Per factor of `spec`, the share of sigma points with psi > 0 at the marginals of (mu0, (D0, U0)^-1)."""
    SigD, SigU = o.inverse_gbp(ch["D0"], ch["U0"])
    mk, Sk = o.gather_marginals(ch["mu0"], SigD, SigU, spec["start"], spec["d"])
    Z, _ = o.nwspgr_cached(spec["d"], spec["p"])
    S = np.stack([o.sym_sqrt(s) for s in Sk])
    X = np.einsum("na,kba->knb", Z, S) + mk[:, None, :]
    return (spec_psi_batch(spec)(X) > 0).mean(axis=1)
