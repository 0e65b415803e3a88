"""CPU helpers of the spectral-stage tests (tests/test_spectral_host.py, tests/test_spectral_prep_gpu.py): the input classes,
the problems of the JKO rows, the rows themselves, 50-digit references (mpmath, imported only inside the functions that need
it) and the recorded error of the float64 restatements the GPU tests compare with (tests/golden/spectral_ref_err.json).

The GPU module never imports mpmath: it compares the device with oracle/gvi_oracle.py (sym_sqrt, batched_moments, bw_jko on the
oracle's moments, as ChainProx.gradients calls it) and takes, per row, bound = max(floor, 32 * ref_err), ref_err being the recorded max-abs error of that float64
restatement against the 50-digit reference, relative to the max-abs entry.  `PYTHONPATH=oracle python tests/spectral_ref.py`
rewrites the file (about two and a half minutes: mpmath's eigsy takes 1.3 s at d = 32).

Scaling of the seeded inputs (the bounds are relative, so the inputs must not hide the quantity under test):
  * nodes: X = mu + S z is rounded at |mu|, the error is measured against max |X - mu|; mu_k is therefore drawn at the scale of
    the marginal's own standard deviation sd_k = sqrt(lambda_max(Sigma_k)) (for `tiny`, a mean of O(1) would leave 1e-10).
  * moments: psi(x) = log(1 + |x - c|^2) + sin(a . x) with c_k = mu_k + sd_k u, a_k = v / sd_k, so psi varies by O(1) over
    the nodes of every class.

What ref_err measures on a JKO row: o.bw_jko against mp_jko on the SAME float64 inputs, the oracle's marginal Sigma and its
S = Lam E2 Lam - Lam E0 (jko_oracle returns both).  Taking the chain's (D, U) as the exact input instead would measure the
conditioning of precision -> marginal -> inverse (cond^2 eps = 1e-8 for cond1e4, whatever the arithmetic), not the restatement:
8.6e-9 at unary d = 16, h = 1e-4 that way, against 7.8e-12 for the map.
"""
import functools
import json
import os

import numpy as np

import gvi_oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_FILE = os.path.join(HERE, "golden", "spectral_ref_err.json")
DPS = 50

D_ALL = tuple(range(1, 18)) + (20, 24, 28, 31, 32)
CLASSES = ("well", "cond1e8", "cond1e4", "clustered", "identity", "diagonal", "near_diag", "tiny", "huge")
NEEDS_2 = ("cond1e8", "cond1e4", "clustered", "near_diag")
MOMENT_CLASSES = ("well", "clustered", "tiny", "cond1e4")
H_ALL = (0.55, 1e-2, 1e-4)
JKO_D = {"u": (1, 2, 3, 5, 6, 7, 8, 9, 12, 13, 16), "b": (2, 4, 6, 8, 12, 16, 18, 24, 32)}
JKO_CLASSES = ("well", "cond1e4")
MARGIN = 32.0


def _sym(A):
    return 0.5 * (A + A.T)


def spectrum(name, d):
    """The eigenvalues the class `name` claims at size d (ascending); None where it only bounds them (near_diag)"""
    lin = np.linspace(0.3, 2.0, d)
    return {"well": lin, "cond1e8": np.geomspace(1e-4, 1e4, d), "cond1e4": np.geomspace(1e-2, 1e2, d),
            "clustered": np.concatenate([np.ones(d // 2), np.full(d - d // 2, 4.0)]), "identity": np.full(d, 0.7), "diagonal": lin,
            "near_diag": None, "tiny": 1e-12 * lin, "huge": 1e12 * lin}[name]


def classes_of(d):
    return tuple(c for c in CLASSES if d >= 2 or c not in NEEDS_2)


def sigma_cases(d, rng):
    """{class: SPD [d, d]}, Q diag(spec) Q^T with Q from the QR of a seeded normal matrix, symmetrised exactly"""
    Q = np.linalg.qr(rng.normal(size=(d, d)))[0]
    E = _sym(rng.normal(size=(d, d)))
    np.fill_diagonal(E, 0.0)
    out = {}
    for name in classes_of(d):
        if name == "identity":
            out[name] = 0.7 * np.eye(d)
        elif name == "diagonal":
            out[name] = np.diag(spectrum(name, d))
        elif name == "near_diag":
            out[name] = np.diag(spectrum("diagonal", d)) + 1e-9 * E
        elif name in ("tiny", "huge"):
            out[name] = (1e-12 if name == "tiny" else 1e12) * out["well"]
        else:
            out[name] = _sym((Q * spectrum(name, d)) @ Q.T)
    return out


# ---- the operator rows (parts 3): one context per d, factor k carries class k ----
@functools.lru_cache(maxsize=None)
def operator_case(d):
    """classes, Sigma [K, d, d], mu [K, d] (at the marginal's scale), and the psi of the moment rows"""
    rng = np.random.default_rng(31000 + d)
    cases = sigma_cases(d, rng)
    names = tuple(cases)
    Sigma = np.stack([cases[c] for c in names])
    sd = np.sqrt(np.array([np.linalg.eigvalsh(S).max() for S in Sigma]))
    mu = rng.normal(size=(len(names), d)) * sd[:, None]
    c = mu + sd[:, None] * rng.normal(size=mu.shape)
    a = rng.normal(size=mu.shape) / sd[:, None] / np.sqrt(d)
    for arr in (Sigma, mu, a, c):
        arr.setflags(write=False)
    return dict(d=d, names=names, Sigma=Sigma, mu=mu, a=a, c=c, sd=sd)


def psi_smooth(a, c):
    """psi_k(x) = log(1 + |x - c_k|^2) + sin(a_k . x) on X [K, N, d] -> [K, N] (the closure batched_moments takes)"""
    def f(X, sel=slice(None)):
        E = X - c[sel][:, None, :]
        return np.log1p(np.einsum("knd,knd->kn", E, E)) + np.sin(np.einsum("knd,kd->kn", X, a[sel]))
    return f


# ---- the JKO rows (part 5): a chain with ONE factor, whose marginal is a Sigma of the class ----
@functools.lru_cache(maxsize=None)
def jko_case(kind, d, cls):
    """kind "u": T = 1, one FIXED_PRIOR factor, d = n;  "b": T = 2, one QUAD_PRIOR factor, d = 2 n.  (D, U) are the blocks of
    the float64 inverse of the class's Sigma (symmetrised): THEY are the inputs, the references invert them again.
    hess: the factor's Hessian, which is its unit-temperature Vddmu in exact arithmetic (psi is quadratic)"""
    rng = np.random.default_rng(52000 + 1000 * (kind == "b") + 10 * d + JKO_CLASSES.index(cls))
    n, T = (d, 1) if kind == "u" else (d // 2, 2)
    P = _sym(np.linalg.inv(sigma_cases(d, rng)[cls]))
    D = np.stack([P[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    U = np.stack([P[:n, n:]]) if T == 2 else np.zeros((0, n, n))
    mu0 = rng.normal(size=(T, n))
    if kind == "u":
        mu_u = rng.normal(size=(1, d))
        G = rng.normal(size=(1, d, d))
        Kinv = G @ G.transpose(0, 2, 1) / d + 0.3 * np.eye(d)
        params, psi, hess = np.concatenate([mu_u, Kinv.reshape(1, -1)], axis=1), o.psi_batch_fixed_prior(mu_u, Kinv), 2.0 * Kinv[0]
    else:
        Phi = np.eye(n)[None] + 0.1 * rng.normal(size=(1, n, n))
        G = rng.normal(size=(1, n, n))
        Qinv = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        J = np.concatenate([Phi[0], -np.eye(n)], axis=1)
        params, psi, hess = np.concatenate([Phi.reshape(1, -1), Qinv.reshape(1, -1)], axis=1), o.psi_batch_quad_prior(Phi, Qinv), J.T @ Qinv[0] @ J
    for arr in (D, U, mu0, params, hess):
        arr.setflags(write=False)
    return dict(kind=kind, d=d, n=n, T=T, cls=cls, D=D, U=U, mu0=mu0, params=params, psi=psi, hess=hess)


def jko_oracle(case, h):
    """The float64 restatement, as o.ChainProx.gradients forms it for this one factor: o.bw_jko on the oracle's unit-temperature
    moments at the oracle's own marginal.  dict(g [T, n], V dense [d, d], Sigma, S): the marginal and S = Lam E2 Lam - Lam E0
    (bw_jko's own expression) are what the 50-digit reference of the MAP takes as its inputs."""
    n, T, d = case["n"], case["T"], case["d"]
    SigD, SigU = o.inverse_gbp(case["D"], case["U"])
    mk, Sk = o.gather_marginals(case["mu0"], SigD, SigU, np.zeros(1, dtype=np.int64), d)
    Z, w = o.nwspgr_cached(d, 3)
    r = o.batched_moments(Z, w, mk, Sk, case["psi"], 1.0)
    Lam = np.linalg.inv(Sk[0])
    Vd, Vdd = o.bw_jko(mk[0], Sk[0], Lam, r["E_phi"][0], r["E_xmuphi"][0], r["E_xxphi"][0], h)
    return dict(g=Vd.reshape(T, n), V=Vdd, Sigma=Sk[0], S=Lam @ r["E_xxphi"][0] @ Lam - Lam * r["E_phi"][0])


def dense_of(VD, VU):
    """[d, d] of the factor from the chain's blocks (T = 1: VD[0];  T = 2: [[VD0, VU0], [VU0^T, VD1]])"""
    if len(VD) == 1:
        return VD[0].copy()
    return np.block([[VD[0], VU[0]], [VU[0].T, VD[1]]])


# ---- the rows ----
def node_rows():
    return [("nodes", d, c) for d in D_ALL for c in classes_of(d)]


def moment_rows():
    return [("moments", d, c) for d in D_ALL for c in MOMENT_CLASSES if c in classes_of(d)]


def jko_rows():
    return [("jko", kind, d, c, h) for kind in ("u", "b") for d in JKO_D[kind] for c in JKO_CLASSES if c in classes_of(d) for h in H_ALL]


def all_rows():
    return node_rows() + moment_rows() + jko_rows()


def key(row):
    return "/".join(f"{v:g}" if isinstance(v, float) else str(v) for v in row)


@functools.lru_cache(maxsize=None)
def recorded():
    with open(ERR_FILE) as f:
        return json.load(f)


def bound(row, floor):
    return max(floor, MARGIN * recorded()[key(row)])


# ---- 50-digit references ----
def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _eigsy(mp, A):
    """(eigenvalues, eigenvector matrix) of a symmetric mp matrix; 1 x 1 by hand (eigsy needs n > 1 rotations)"""
    if A.rows == 1:
        return mp.matrix([A[0, 0]]), mp.matrix([[1]])
    return mp.eigsy(A)


def _mp_spectral(mp, A, fn):
    E, Q = _eigsy(mp, A)
    return Q * mp.diag([fn(E[i]) for i in range(A.rows)]) * Q.T


def mp_sym_sqrt(Sigma):
    mp = _mp()
    return _mp_spectral(mp, mp.matrix(np.asarray(Sigma).tolist()), mp.sqrt)


def mp_jko(Sigma, S, h):
    """oracle/gvi_oracle.py::bw_jko in mpmath: M = I - h S, Sig_half = M Sigma M^T, Sigma_new = f(Sig_half) with
    f(l) = l/2 + h + sqrt(l (l + 4h))/2, Vddmu = (Sigma_new^-1 - Sigma^-1) / h.  Sigma, S: mp matrices."""
    mp = _mp()
    h = mp.mpf(h)
    M = mp.eye(Sigma.rows) - h * S
    Sh = M * Sigma * M.T
    Sh = (Sh + Sh.T) / 2
    Lam_new = _mp_spectral(mp, Sh, lambda l: 1 / (l / 2 + h + mp.sqrt(l * (l + 4 * h)) / 2))
    return (Lam_new - Sigma ** -1) / h


def jko_scalar(sigma, s, h):
    """The 1-D closed form of the map, in mpmath"""
    mp = _mp()
    sigma, s, h = mp.mpf(sigma), mp.mpf(s), mp.mpf(h)
    l = (1 - h * s) ** 2 * sigma
    return (1 / (l / 2 + h + mp.sqrt(l * (l + 4 * h)) / 2) - 1 / sigma) / h


def mp_moments(Z, w, mu, Sigma, a, c):
    """(E_phi, Vdmu, Vddmu) of one factor at unit temperature for psi = log(1 + |x - c|^2) + sin(a . x), as
    oracle/gvi_oracle.py::batched_moments forms them, in mpmath"""
    mp = _mp()
    d = len(mu)
    Sg = mp.matrix(np.asarray(Sigma).tolist())
    S, Lam = _mp_spectral(mp, Sg, mp.sqrt), Sg ** -1
    muv, av, cv = (mp.matrix(np.asarray(v).tolist()) for v in (mu, a, c))
    E0, E1, E2 = mp.mpf(0), mp.zeros(d, 1), mp.zeros(d, d)
    for zn, wn in zip(np.asarray(Z), np.asarray(w)):
        y = S * mp.matrix(zn.tolist())
        x = y + muv
        e = x - cv
        v = (mp.log(1 + (e.T * e)[0, 0]) + mp.sin((av.T * x)[0, 0])) * mp.mpf(float(wn))
        E0 += v
        E1 += v * y
        E2 += v * (y * y.T)
    return E0, Lam * E1, Lam * E2 * Lam - Lam * E0


def _rel_mp(a, ref, scale=None):
    """max-abs error of the float64 array a against the mp matrix (or scalar) ref, relative to ref's max-abs entry"""
    mp = _mp()
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    if not isinstance(ref, mp.matrix):
        ref = mp.matrix([[ref]])
    if a.shape != (ref.rows, ref.cols):
        a = a.reshape(ref.rows, ref.cols)
    if not np.isfinite(a).all():
        return float("inf")
    err = max(abs(mp.mpf(float(a[i, j])) - ref[i, j]) for i in range(ref.rows) for j in range(ref.cols))
    if scale is None:
        scale = max(abs(ref[i, j]) for i in range(ref.rows) for j in range(ref.cols))
    return float(err / scale)


def vddmu_scale_1d(Sigma, E_phi):
    """d = 1 at p = 2: the rule's nodes are +-1, so Vddmu = Lam (z^2 - 1) E_phi vanishes identically and what any arithmetic
    returns is rounding of its two terms; it is measured against their size |Lam E_phi|"""
    return abs(float(E_phi) / float(np.asarray(Sigma).reshape(-1)[0]))


def ref_err(row):
    """The number recorded for the row: the float64 restatement against the 50-digit reference"""
    if row[0] == "nodes":
        _, d, cls = row
        C = operator_case(d)
        k = C["names"].index(cls)
        return _rel_mp(o.sym_sqrt(C["Sigma"][k]), mp_sym_sqrt(C["Sigma"][k]))
    if row[0] == "moments":
        _, d, cls = row
        C = operator_case(d)
        k = C["names"].index(cls)
        Z, w = o.nwspgr_cached(d, 2)
        sl = slice(k, k + 1)
        r = o.batched_moments(Z, w, C["mu"][sl], C["Sigma"][sl], psi_smooth(C["a"][sl], C["c"][sl]), 1.0)
        E0, V1, V2 = mp_moments(Z, w, C["mu"][k], C["Sigma"][k], C["a"][k], C["c"][k])
        scale = vddmu_scale_1d(C["Sigma"][k], r["E_phi"][0]) if d == 1 else None
        return max(_rel_mp(r["E_phi"][0], E0), _rel_mp(r["Vdmu"][0], V1), _rel_mp(r["Vddmu"][0], V2, scale))
    _, kind, d, cls, h = row
    mp = _mp()
    R = jko_oracle(jko_case(kind, d, cls), h)
    return _rel_mp(R["V"], mp_jko(mp.matrix(R["Sigma"].tolist()), mp.matrix(R["S"].tolist()), h))


def write_err_file(path=ERR_FILE):
    out = {key(r): float(f"{ref_err(r):.3e}") for r in all_rows()}
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    return out


if __name__ == "__main__":
    vals = write_err_file()                                           # PYTHONPATH=oracle python tests/spectral_ref.py
    for part in ("nodes", "moments", "jko"):
        v = [x for k, x in vals.items() if k.startswith(part)]
        print(f"{part}: {len(v)} rows, ref_err {min(v):.1e} .. {max(v):.1e}")
