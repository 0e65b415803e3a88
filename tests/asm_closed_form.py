"""Quadrature-free reference of the assembled NGD system for chains of QUAD_PRIOR / FIXED_PRIOR factor sets with ANY start
list (repeated, unsorted, sparse): psi is quadratic, so a degree-3 rule integrates the moments exactly and
  V = sum over the factors of Hessian_k / temperature_k, placed on the block(s) start[k] (and start[k] + 1),
  g = sum of the factor gradients at the mean / temperature_k,    dmu = solve(dense(V), -g),
  E[psi_k] = psi_k(mu_k) + tr(Hessian_k Sigma_k) / 2.
Plain numpy, no GPU.  A set is a dict: kind "b" (binary, d = 2n: Phi [K,n,n], Q [K,n,n]; psi = (Phi x0 - x1)^T Q (Phi x0 - x1) / 2)
or "u" (unary, d = n: mu_u [K,n], Kinv [K,n,n]; psi = (x - mu_u)^T Kinv (x - mu_u)), start [K], and optionally temp [K]."""
import numpy as np

import gvi_oracle as o


def _temp(s):
    return np.broadcast_to(np.asarray(s.get("temp", 1.0), dtype=np.float64), (len(s["start"]),))


def _hessian(s, k, n):
    if s["kind"] == "b":
        J = np.hstack([s["Phi"][k], -np.eye(n)])
        return J.T @ s["Q"][k] @ J                                # psi = (J x)^T Q (J x) / 2
    return 2.0 * s["Kinv"][k]                                     # psi = (x - mu_k)^T Kinv (x - mu_k)


def closed_form(T, n, sets, mu, solve=True):
    """g, V_D, V_U as the sums above, set after set and factor after factor; parts[i]: set i's share of V_D; dmu from the dense
    system (None with solve = False: a singular V)"""
    g, VD, VU = np.zeros((T, n)), np.zeros((T, n, n)), np.zeros((max(T - 1, 0), n, n))
    parts = []
    for s in sets:
        part, temp = np.zeros((T, n, n)), _temp(s)
        for k, t in enumerate(np.asarray(s["start"], dtype=np.int64)):
            H = _hessian(s, k, n) / temp[k]
            if s["kind"] == "b":
                gr = H @ np.concatenate([mu[t], mu[t + 1]])
                g[t] += gr[:n]; g[t + 1] += gr[n:]
                part[t] += H[:n, :n]; part[t + 1] += H[n:, n:]; VU[t] += H[:n, n:]
            else:
                g[t] += H @ (mu[t] - s["mu_u"][k]); part[t] += H
        VD += part
        parts.append(part)
    dmu = np.linalg.solve(o.bt_to_dense(VD, VU), -g.reshape(-1)).reshape(T, n) if solve else None
    return dict(g=g, VD=VD, VU=VU, parts=parts, dmu=dmu)


def closed_form_cost(T, n, sets, mu, D, U):
    """sum_k E[psi_k] / temperature_k + log det(Lambda) / 2 of q = N(mu, Lambda^-1), Lambda = the chain (D, U)"""
    Lam = o.bt_to_dense(D, U)
    Sig = np.linalg.inv(Lam)
    value = 0.0
    for s in sets:
        temp, d = _temp(s), (2 * n if s["kind"] == "b" else n)
        for k, t in enumerate(np.asarray(s["start"], dtype=np.int64)):
            H, x = _hessian(s, k, n), mu[t:t + d // n].reshape(-1)
            if s["kind"] == "u":
                x = x - s["mu_u"][k]
            value += (x @ H @ x / 2 + np.trace(H @ Sig[t * n:t * n + d, t * n:t * n + d]) / 2) / temp[k]
    sign, logdet = np.linalg.slogdet(Lam)
    assert sign > 0
    return value + logdet / 2
