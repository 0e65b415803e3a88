"""Reference of the limit factors (GVI_PSI_HINGE_BOX, include/gvi_hip.h): a numpy restatement.  The
reference project has no such factor, so nothing in oracle/ restates it.

  psi(x) = sum_i sigma_i [max(0, x_i - (hi_i - eps_i))^2 + max(0, (lo_i + eps_i) - x_i)^2]
  margin(x) = min_i min(hi_i - x_i, x_i - lo_i)

params [K][4 d] = [sigma (d) | eps (d) | lo (d) | hi (d)]; lo = -inf / hi = +inf switches a side off.
psi_batch takes (X [K][N][d], sel) like the oracle's psi_batch_* and plugs into o.batched_moments / o.FactorSet;
closed_form(params) is a FactorSet.fast_moments: the exact Gaussian moments from Phi and phi of the 1-D marginals."""
import math

import numpy as np

_erfc = np.vectorize(math.erfc, otypes=[np.float64])
_exp = np.vectorize(math.exp, otypes=[np.float64])


def unpack(params, d):
    """(sigma, eps, lo, hi), each [K][d]."""
    params = np.asarray(params, dtype=np.float64)
    assert params.ndim == 2 and params.shape[1] == 4 * d, "parameter block is not [sigma | eps | lo | hi]"
    return params[:, :d], params[:, d:2 * d], params[:, 2 * d:3 * d], params[:, 3 * d:]


def psi_batch(params, d):
    def f(X, sel=slice(None)):
        sig, eps, lo, hi = (v[:, None, :] for v in unpack(np.asarray(params)[sel], d))
        with np.errstate(invalid="ignore"):
            up = np.where(np.isfinite(hi), np.maximum(0.0, X - (hi - eps)), 0.0)
            dn = np.where(np.isfinite(lo), np.maximum(0.0, (lo + eps) - X), 0.0)
        return (sig * up * up + sig * dn * dn).sum(axis=2)
    return f


def margin(params, d, X):
    """[K][N] for X [K][N][d]; +inf for a factor without a finite limit."""
    _, _, lo, hi = (v[:, None, :] for v in unpack(params, d))
    return np.minimum(hi - X, X - lo).min(axis=2)


def side_expectations(sigma, sd, gap, sgn):
    """(e0, e1, e2) = (E[h], E[h'], E[h'']) of h(x) = sigma max(0, sgn (x - a))^2 at x ~ N(m, sd^2), gap = sgn (m - a):
    e0 = sigma sd^2 [(1 + t^2) Phi(t) + t phi(t)], e1 = sgn 2 sigma sd [t Phi(t) + phi(t)], e2 = 2 sigma Phi(t), t = gap / sd.
    Phi through erfc; for t <= -3 the brackets through a continued fraction (below).  Arrays broadcast; every entry must be finite (the caller skips an infinite side)."""
    sigma, sd, gap = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (sigma, sd, gap)))
    t = gap / sd
    phi = 0.39894228040143267794 * _exp(-0.5 * t * t)
    b0 = 0.5 * _erfc(-t * 0.70710678118654752440)
    b1, b2 = t * b0 + phi, (1.0 + t * t) * b0 + t * phi
    tail = t <= -3.0
    if tail.any():
        # the brackets cancel for t < 0 (to t^4 / 2 of their size): repeated integrals of erfc at x = -t / sqrt 2 through the
        # continued fraction of their ratios r_n = 1 / (2 x + 2 (n + 1) r_(n+1)), backwards from r_65 = 0 -- products only
        x = -t[tail] * 0.70710678118654752440
        rn, keep = np.zeros(x.shape), {}
        for n in range(64, -1, -1):
            rn = 1.0 / (2.0 * x + 2.0 * (n + 1) * rn)
            if n <= 2:
                keep[n] = rn
        i0 = keep[0] * (1.12837916709551257390 * _exp(-x * x))
        i1 = keep[1] * i0
        b0, b1, b2 = b0.copy(), b1.copy(), b2.copy()
        b0[tail], b1[tail], b2[tail] = 0.5 * i0, 0.70710678118654752440 * i1, 2.0 * (keep[2] * i1)
    return sigma * sd * sd * b2, sgn * 2.0 * sigma * sd * b1, 2.0 * sigma * b0


def coordinate_expectations(params, d, m, sd):
    """(e0, e1, e2) [K][d] summed over the finite sides of every coordinate; m, sd [K][d]."""
    sig, eps, lo, hi = unpack(params, d)
    out = [np.zeros(m.shape) for _ in range(3)]
    for fin, gap, sgn in ((np.isfinite(hi), m - (hi - eps), 1.0), (np.isfinite(lo), (lo + eps) - m, -1.0)):
        if fin.any():
            e = side_expectations(sig[fin], sd[fin], gap[fin], sgn)
            for acc, v in zip(out, e):
                acc[fin] += v
    return out


def t_values(params, d, mu, Sigma):
    """t [K][d][2] (upper, lower): how far the mean is inside each hinge in standard deviations; NaN for a side that is off."""
    sig, eps, lo, hi = unpack(params, d)
    sd = np.sqrt(np.einsum("kii->ki", Sigma))
    with np.errstate(invalid="ignore"):
        t = np.stack([(mu - (hi - eps)) / sd, ((lo + eps) - mu) / sd], axis=2)
    t[~np.isfinite(np.stack([hi, lo], axis=2))] = np.nan
    return t


def closed_moments(params, d, mu, Sigma, temperature):
    """The exact moments: dict with E_phi, cost, Vdmu, Vddmu, E_xmuphi, E_xxphi (the keys of o.batched_moments).
    E[(x - mu) psi] = Sigma E[grad psi], E[(x - mu)(x - mu)^T psi] = E[psi] Sigma + Sigma diag(E[d^2 psi / dx_i^2]) Sigma
    (Stein), hence Vdmu = E[grad psi] / T and Vddmu = diag(E[d^2 psi / dx_i^2]) / T."""
    mu, Sigma = np.asarray(mu, dtype=np.float64), np.asarray(Sigma, dtype=np.float64)
    T = np.broadcast_to(np.asarray(temperature, dtype=np.float64).reshape(-1), (mu.shape[0],))
    with np.errstate(invalid="ignore"):                      # a trial state of a line search need not be positive definite: NaN
        sd = np.sqrt(np.einsum("kii->ki", Sigma))
    e0, e1, e2 = coordinate_expectations(params, d, mu, sd)
    E = e0.sum(axis=1)
    Vddmu = np.einsum("ki,ij->kij", e2, np.eye(d)) / T[:, None, None]
    Ex = np.einsum("kab,kb->ka", Sigma, e1)
    Exx = E[:, None, None] * Sigma + np.einsum("kai,ki,kib->kab", Sigma, e2, Sigma)
    return dict(E_phi=E, cost=E / T, Vdmu=e1 / T[:, None], Vddmu=Vddmu, E_xmuphi=Ex, E_xxphi=Exx)


def closed_form(params, d):
    """FactorSet.fast_moments of a box set: (mk, Sk, temperature) -> (E_phi, Vdmu, Vddmu)."""
    def f(mk, Sk, temperature):
        r = closed_moments(params, d, mk, Sk, temperature)
        return r["E_phi"], r["Vdmu"], r["Vddmu"]
    return f
