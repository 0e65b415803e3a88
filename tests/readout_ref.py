"""Reference of the read-out-space quadrature (gvi_factors_set_readout_rule) in numpy float64, written from
the formulas and independently of gaussianvi_amd/csrc/readout_moments.hpp.  The 1-D rule is the in-tree one
(api.spgh_nodes(1, order)); the kinds' distances are those of segment_ref / balls_ref / the oracle's look-ups.

A set is a list over factors of lists over check points of (W [P][d], c [P], f), f(q [n][P]) -> [n].  Per check point, with
C = W Sigma W^T, L its lower Cholesky factor under the drop rule and T = "L^-1 W" on the kept coordinates (T Sigma T^T = I there):

  e0 = sum om f,  h = sum om xi f,  H = sum om (xi xi^T - I) f   at q = W mu + c + L xi over the tensor rule of the kept coordinates
  E[psi] = sum_j e0      E[(x - mu) psi] = Sigma sum_j T^T h      E[(x - mu)(x - mu)^T psi] = E[psi] Sigma + Sigma (sum_j T^T H T) Sigma
  Vdmu = sum_j T^T h / temperature      Vddmu = sum_j T^T H T / temperature

Nothing here takes a root of Sigma: the result depends on Sigma only."""
import functools

import numpy as np

import balls_ref
import gvi_oracle as o
import segment_ref
from gaussianvi_amd import api, synthetic as syn

NPOS = {syn.PSI_HINGE_SDF_2D: 2, syn.PSI_HINGE_SDF_3D: 3, syn.PSI_HINGE_SDF_2D_SEG: 2, syn.PSI_HINGE_SDF_3D_SEG: 3,
        syn.PSI_HINGE_BALLS_2D: 2, syn.PSI_HINGE_BALLS_3D: 3}
COND_MAX = 1e4


@functools.lru_cache(maxsize=None)
def rule(order):
    Z, w, _ = api.spgh_nodes(1, order)
    assert Z.shape == (order, 1)
    return Z[:, 0].copy(), w.copy()


def chol_drop(C):
    """(L, keep, ok) of the semidefinite rule: pivot p = C_kk - sum L_ki^2, thr = 64 2^-52 C_kk; |p| <= thr drops coordinate k,
    p NaN, p < -thr or C_kk < 0: not ok."""
    P = C.shape[0]
    L, keep = np.zeros((P, P)), np.zeros(P, dtype=bool)
    for k in range(P):
        p = C[k, k] - (L[k, :k] ** 2).sum()
        thr = 64.0 * 2.0 ** -52 * C[k, k]
        if np.isnan(p) or p < -thr or C[k, k] < 0:
            return L, keep, False
        if abs(p) <= thr:
            continue
        keep[k] = True
        L[k, k] = np.sqrt(p)
        for r in range(k + 1, P):
            L[r, k] = (C[r, k] - L[r, :k] @ L[k, :k]) / L[k, k]
    return L, keep, True


def kept_cond(C, keep):
    """Condition number of C on the kept coordinates (1 when none is kept)."""
    if not keep.any():
        return 1.0
    ev = np.linalg.eigvalsh(C[np.ix_(keep, keep)])
    return ev[-1] / ev[0]


def tensor_nodes(order, keep):
    """xi [n][P] (0 on dropped coordinates), om [n]: the first kept coordinate runs fastest."""
    x, w = rule(order)
    P = len(keep)
    xi, om = np.zeros((1, P)), np.ones(1)
    for k in reversed(range(P)):
        if keep[k]:
            base = np.repeat(xi, order, axis=0)
            base[:, k] = np.tile(x, len(xi))
            xi, om = base, np.repeat(om, order) * np.tile(w, len(om))
    return xi, om


def check_point(W, c, mu, Sigma, order, f, diag=None):
    """(e0, a [d], B [d][d]) with a = T^T h, B = T^T H T; None when the covariance of the read-out is not positive semidefinite."""
    P, d = W.shape
    C = W @ Sigma @ W.T
    C = (C + C.T) / 2
    L, keep, ok = chol_drop(C)
    if not ok:
        return None
    assert kept_cond(C, keep) <= COND_MAX, ("read-out covariance too ill-conditioned for the bounds of the tests", kept_cond(C, keep))
    T = np.zeros((P, d))
    for k in range(P):
        if keep[k]:
            T[k] = (W[k] - L[k, :k] @ T[:k]) / L[k, k]
    xi, om = tensor_nodes(order, keep)
    q = (W @ mu + c)[None, :] + xi @ L.T
    fv = f(q)
    if diag is not None:
        diag.append(dict(q=q, f=fv, keep=keep.copy(), om=om))
    with np.errstate(invalid="ignore"):                               # f = -inf at every node: spec_gaps of a scene without balls
        wf = om * fv
        e0 = wf.sum()
        h = wf @ xi
        H = np.einsum("n,na,nb->ab", wf, xi, xi) - e0 * np.diag(keep.astype(float))
    return e0, T.T @ h, T.T @ H @ T


def moments(factors, mu, Sigma, order, temperature=1.0, diag=None):
    """factors[k] = [(W, c, f), ...].  Returns the dict of o.batched_moments (E_phi, E_xmuphi, E_xxphi, Vdmu, Vddmu, cost); a factor
    whose read-out covariance is not positive semidefinite is NaN."""
    K, d = mu.shape
    T = np.broadcast_to(np.asarray(temperature, dtype=np.float64).reshape(-1), (K,))
    out = dict(E_phi=np.zeros(K), E_xmuphi=np.zeros((K, d)), E_xxphi=np.zeros((K, d, d)), Vdmu=np.zeros((K, d)), Vddmu=np.zeros((K, d, d)))
    for k in range(K):
        e0, a, B = 0.0, np.zeros(d), np.zeros((d, d))
        dk = [] if diag is not None else None
        for W, c, f in factors[k]:
            r = check_point(np.asarray(W, dtype=np.float64), np.asarray(c, dtype=np.float64), mu[k], Sigma[k], order, f, dk)
            if r is None:
                e0, a, B = np.nan, np.full(d, np.nan), np.full((d, d), np.nan)
                break
            e0, a, B = e0 + r[0], a + r[1], B + r[2]
        if diag is not None:
            diag.append(dk)
        out["E_phi"][k] = e0
        out["E_xmuphi"][k] = Sigma[k] @ a
        out["E_xxphi"][k] = e0 * Sigma[k] + Sigma[k] @ B @ Sigma[k]
        out["Vdmu"][k] = a / T[k]
        out["Vddmu"][k] = B / T[k]
    out["cost"] = out["E_phi"] / T
    return out


# ---- the kinds ----
def hinge(sd, thr, sigma):
    err = np.where(sd > thr, 0.0, thr - np.where(np.isinf(sd), thr, sd))
    return err * err * sigma


def grid_distance(P, origin, cell, field):
    if P == 2:
        return lambda q: o.planar_sdf_lookup(q[:, 0], q[:, 1], origin, cell, field)
    return lambda q: o.sdf3d_lookup(q[:, 0], q[:, 1], q[:, 2], origin, cell, field)


def balls_distance(P, tau, slots):
    """q [n][P] -> sd [n] through balls_ref on a block whose read-out is the identity on a P-dimensional slice."""
    blk = np.concatenate([[1.0, 0.0, 0.0], np.eye(P).ravel(), np.zeros(P), [tau], np.ravel(slots)])[None]
    return lambda q: balls_ref.check_point_distances(blk, P, P, q[None])[0, 0]


def spec_distances(spec):
    """dist[k][j]: q [n][P] -> sd [n], and (sigma, thr) [K], (W, c) [K][J] of a set's spec (kind, d, params and the grid)."""
    kind, d, prm = spec["kind"], spec["d"], np.asarray(spec["params"], dtype=np.float64)
    P, K = NPOS[kind], len(prm)
    if kind in balls_ref.NPOS:
        u = balls_ref.unpack(prm, P, d)
        slots = np.concatenate([u["o"], u["v"], u["R"][:, :, None]], axis=2)
        J = u["W"].shape[1]
        dist = [[balls_distance(P, u["tau"][k, j], slots[k]) for j in range(J)] for k in range(K)]
        return dist, u["sigma"], u["eps"] + u["r"], u["W"], u["c"]
    g = grid_distance(P, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    if kind in segment_ref.NPOS:
        sig, eps, r, W, c = segment_ref.unpack(prm, P, d)
        return [[g] * W.shape[1]] * K, sig, eps + r, W, c
    W = np.tile(np.eye(P, d)[None, None], (K, 1, 1, 1))
    return [[g]] * K, prm[:, 0], prm[:, 1] + prm[:, 2], W, np.zeros((K, 1, P))


def spec_factors(spec, sel=slice(None)):
    dist, sigma, thr, W, c = spec_distances(spec)
    ks = range(len(sigma))[sel]
    return [[(W[k, j], c[k, j], (lambda q, fn=dist[k][j], t=thr[k], s=sigma[k]: hinge(fn(q), t, s))) for j in range(W.shape[1])] for k in ks]


def spec_moments(spec, mu, Sigma, order, temperature=None, diag=None):
    T = spec["temperature"] if temperature is None else temperature
    return moments(spec_factors(spec), mu, Sigma, order, T, diag)


def spec_gaps(spec, mu, Sigma, order):
    """Per factor: thr - sd at every node of every check point (positive: inside the hinge), and the nodes themselves."""
    dist, sigma, thr, W, c = spec_distances(spec)
    fac = [[(W[k, j], c[k, j], (lambda q, fn=dist[k][j], t=thr[k]: t - fn(q))) for j in range(W.shape[1])] for k in range(len(sigma))]
    diag = []
    moments(fac, mu, Sigma, order, 1.0, diag)
    return [np.concatenate([e["f"] for e in dk]) for dk in diag], [np.concatenate([e["q"] for e in dk]) for dk in diag]


def fast_moments(spec, order):
    """The hook of o.FactorSet.fast_moments: (mk, Sk, temperature) -> (E_phi, Vdmu, Vddmu)."""
    def f(mk, Sk, temperature):
        r = spec_moments(spec, mk, Sk, order, temperature)
        return r["E_phi"], r["Vdmu"], r["Vddmu"]
    return f
