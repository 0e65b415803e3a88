"""Reference psi and clearance of the moving-ball obstacle factors (GVI_PSI_HINGE_BALLS_2D / _3D, include/gvi_hip.h) in numpy
float64, written from the header's formulas and independently of gaussianvi_amd/csrc/balls_psi.hpp.  The reference project has
no such factor, so nothing in oracle/ restates it.

  q_j = W_j x + c_j       sd_j(x) = min over the slots with R_m != -inf of |q_j - (o_m + tau_j v_m)| - R_m   (+inf: every slot empty)
  psi(x) = sigma * sum_j max(0, eps + r - sd_j(x))^2        clearance(x) = min_j sd_j(x) - r

params [K][3 + J (P (d + 1) + 1) + 8 (2 P + 1)] = [sigma, eps, r | J x (W_j (P x d) | c_j (P) | tau_j) | 8 x (o_m (P) | v_m (P) | R_m)].
The closures take (X [K][N][d], sel) like the oracle's psi_batch_* and plug into o.batched_moments / o.FactorSet."""
import numpy as np

import gvi_oracle as o
from gaussianvi_amd import synthetic as syn

NPOS = {syn.PSI_HINGE_BALLS_2D: 2, syn.PSI_HINGE_BALLS_3D: 3}
SLOTS = 8


def block_size(P, d, J):
    return 3 + J * (P * (d + 1) + 1) + SLOTS * (2 * P + 1)


def unpack(params, P, d):
    """dict of sigma, eps, r [K]; W [K][J][P][d], c [K][J][P], tau [K][J]; o, v [K][8][P], R [K][8]."""
    params = np.asarray(params, dtype=np.float64)
    K, per, tail = params.shape[0], P * (d + 1) + 1, SLOTS * (2 * P + 1)
    body = params.shape[1] - 3 - tail
    assert body > 0 and body % per == 0, "ragged parameter block"
    J = body // per
    pts = params[:, 3:3 + body].reshape(K, J, per)
    slots = params[:, 3 + body:].reshape(K, SLOTS, 2 * P + 1)
    return dict(sigma=params[:, 0], eps=params[:, 1], r=params[:, 2], W=pts[:, :, :P * d].reshape(K, J, P, d), c=pts[:, :, P * d:P * d + P],
                tau=pts[:, :, P * d + P], o=slots[:, :, :P], v=slots[:, :, P:2 * P], R=slots[:, :, 2 * P])


def check_point_distances(params, P, d, X, sel=slice(None)):
    """sd [K][J][N]: the signed distance to the union of the balls at check point j of factor k at the slice X[k, i]."""
    u = unpack(np.asarray(params)[sel], P, d)
    q = np.einsum("kjpd,knd->kjnp", u["W"], X) + u["c"][:, :, None, :]                     # [K][J][N][P]
    sd = np.full(q.shape[:3], np.inf)
    for m in range(SLOTS):
        live = u["R"][:, m] != -np.inf                                                     # [K]
        with np.errstate(invalid="ignore", over="ignore"):
            centre = u["o"][:, None, m, :] + u["tau"][:, :, None] * u["v"][:, None, m, :]  # [K][J][P]
            dist = np.sqrt(((q - centre[:, :, None, :]) ** 2).sum(axis=-1)) - u["R"][:, m][:, None, None]
        sd = np.where(live[:, None, None], np.minimum(sd, dist), sd)
    return sd


def psi(params, P, d, X, sel=slice(None)):
    u = unpack(np.asarray(params)[sel], P, d)
    sd = check_point_distances(params, P, d, X, sel)
    thr = (u["eps"] + u["r"])[:, None, None]
    err = np.where(sd > thr, 0.0, thr - np.where(np.isinf(sd), thr, sd))
    return (err * err * u["sigma"][:, None, None]).sum(axis=1)


def psi_batch_hinge_balls(params, P, d):
    def f(X, sel=slice(None)):
        return psi(params, P, d, X, sel)
    return f


def clearance(params, P, d, X):
    """clr [K][N] = min_j sd_j - r."""
    sd = check_point_distances(params, P, d, X)
    return (sd - np.asarray(params)[:, 2][:, None, None]).min(axis=1)


def spec_psi_batch(spec):
    return psi_batch_hinge_balls(spec["params"], NPOS[spec["kind"]], spec["d"])


def spec_clearance(spec, X):
    return clearance(spec["params"], NPOS[spec["kind"]], spec["d"], X)


def attach_oracle(ch):
    """make_chain's glue (tests/chains.py) for a chain that may hold moving-ball sets: psi_batch on every spec and oracle_sets()."""
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
