"""Reference of the half-space and corridor limit factors (GVI_PSI_HINGE_HALFSPACE, include/gvi_hip.h): a
numpy restatement.  The reference project has no such factor, so nothing in oracle/ restates it.

  psi(x)    = sum_j sigma_j max(0, a_j^T x - (b_j - eps_j))^2
  margin(x) = min over rows with sigma_j > 0 of (b_j - a_j^T x) / |a_j|

params [K][J (d + 3)] = [sigma (J) | eps (J) | b (J) | A (J x d, row-major)]; a row with sigma_j = 0 is off.
psi_batch takes (X [K][N][d], sel) like the oracle's psi_batch_* and plugs into o.batched_moments / o.FactorSet;
closed_form(params) is a FactorSet.fast_moments: the scalar a_j^T x is a 1-D Gaussian N(a_j^T mu, a_j^T Sigma a_j), its hinge has
the expectations of box_ref.side_expectations, and Stein's lemma along a_j gives the rest.  Nothing here takes a root of Sigma."""
import numpy as np

from box_ref import side_expectations


def unpack(params, d):
    """(sigma [K][J], eps [K][J], b [K][J], A [K][J][d])."""
    params = np.asarray(params, dtype=np.float64)
    assert params.ndim == 2 and params.shape[1] % (d + 3) == 0 and params.shape[1] >= d + 3, "parameter block is not [sigma | eps | b | A]"
    J = params.shape[1] // (d + 3)
    return params[:, :J], params[:, J:2 * J], params[:, 2 * J:3 * J], params[:, 3 * J:].reshape(-1, J, d)


def psi_batch(params, d):
    def f(X, sel=slice(None)):
        sig, eps, b, A = unpack(np.asarray(params)[sel], d)
        with np.errstate(invalid="ignore"):
            e = np.einsum("kjd,knd->knj", A, X) - (b - eps)[:, None, :]
            h = np.where(sig[:, None, :] > 0, np.maximum(0.0, e), 0.0)
        return (sig[:, None, :] * h * h).sum(axis=2)
    return f


def margin(params, d, X):
    """[K][N] for X [K][N][d]; +inf for a factor whose rows are all off."""
    sig, _, b, A = unpack(params, d)
    norm = np.sqrt((A * A).sum(axis=2))
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = (b[:, None, :] - np.einsum("kjd,knd->knj", A, X)) / norm[:, None, :]
    return np.where(sig[:, None, :] > 0, dist, np.inf).min(axis=2)


def row_gaussians(params, d, mu, Sigma):
    """(mean, sd) [K][J] of the scalars a_j^T x."""
    _, _, _, A = unpack(params, d)
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.einsum("kja,kab,kjb->kj", A, Sigma, A))
    return np.einsum("kjd,kd->kj", A, mu), sd


def t_values(params, d, mu, Sigma):
    """t [K][J]: how far the mean is inside each row's hinge in standard deviations; NaN for a row that is off."""
    sig, eps, b, _ = unpack(params, d)
    m, sd = row_gaussians(params, d, mu, Sigma)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (m - (b - eps)) / sd
    return np.where(sig > 0, t, np.nan)


def row_expectations(params, d, mu, Sigma):
    """(e0, e1, e2) [K][J]: E[h], E[h'], E[h''] of the rows' hinges, zeros for a row that is off.  sd = 0: the hinge at the mean."""
    sig, eps, b, _ = unpack(params, d)
    m, sd = row_gaussians(params, d, mu, Sigma)
    gap = m - (b - eps)
    out = [np.zeros(sig.shape) for _ in range(3)]
    on = sig > 0
    rnd, det = on & (sd > 0), on & ~(sd > 0)
    if rnd.any():
        for acc, v in zip(out, side_expectations(sig[rnd], sd[rnd], gap[rnd], 1.0)):
            acc[rnd] = v
    if det.any():
        g = np.maximum(gap[det], 0.0)
        out[0][det], out[1][det], out[2][det] = sig[det] * g * g, 2.0 * sig[det] * g, np.where(gap[det] > 0, 2.0 * sig[det], 0.0)
    return out


def closed_moments(params, d, mu, Sigma, temperature):
    """The exact moments: dict with E_phi, cost, Vdmu, Vddmu, E_xmuphi, E_xxphi (the keys of o.batched_moments).
    E[grad psi] = sum_j a_j e1_j and E[hess psi] = sum_j a_j a_j^T e2_j; by Stein E[(x - mu) psi] = Sigma E[grad psi] and
    E[(x - mu)(x - mu)^T psi] = E[psi] Sigma + Sigma E[hess psi] Sigma, hence Vdmu = E[grad psi] / T, Vddmu = E[hess psi] / T."""
    mu, Sigma = np.asarray(mu, dtype=np.float64), np.asarray(Sigma, dtype=np.float64)
    T = np.broadcast_to(np.asarray(temperature, dtype=np.float64).reshape(-1), (mu.shape[0],))
    A = unpack(params, d)[3]
    e0, e1, e2 = row_expectations(params, d, mu, Sigma)
    E = e0.sum(axis=1)
    grad = np.einsum("kj,kjd->kd", e1, A)
    hess = np.einsum("kj,kja,kjb->kab", e2, A, A)
    Ex = np.einsum("kab,kb->ka", Sigma, grad)
    Exx = E[:, None, None] * Sigma + np.einsum("kai,kij,kjb->kab", Sigma, hess, Sigma)
    return dict(E_phi=E, cost=E / T, Vdmu=grad / T[:, None], Vddmu=hess / T[:, None, None], E_xmuphi=Ex, E_xxphi=Exx)


def closed_form(params, d):
    """FactorSet.fast_moments of a half-space set: (mk, Sk, temperature) -> (E_phi, Vdmu, Vddmu)."""
    def f(mk, Sk, temperature):
        r = closed_moments(params, d, mk, Sk, temperature)
        return r["E_phi"], r["Vdmu"], r["Vddmu"]
    return f
