"""Deterministic synthetic factor chains for tests and bench.py.

Pure numpy/scipy input generation -- no oracle, no device code.  A chain is T states of size n with
block-tridiagonal precision; factors come in homogeneous *sets* (same kind, d, GH degree), the unit
the C-ABI works on.  psi parameter blocks use the C-ABI layouts of include/gvi_hip.h:

  QUAD_PRIOR  [Phi (n x n, row-major) | Qinv (n x n)]          d = 2n   (gp/minimum_acc_prior.h, gp/LTV_prior.h)
  FIXED_PRIOR [mu0 (d) | Kinv (d x d)]                         d = n    (gp/fixed_prior.h)
  RANGE_1D    [y, mu_p, f*b, sig_r_sq, sig_p_sq]               d = 1    (src/1d_example.cpp:25-35)
  HINGE_SDF_2D_SEG / _3D_SEG  [sigma, eps, r | W_0 (P x d) | c_0 (P) | ... ]   d = n or 2n   (segment_params)
  HINGE_BOX   [sigma (d) | eps (d) | lo (d) | hi (d)]          d = n or 2n   (box_params)
  HINGE_HALFSPACE  [sigma (J) | eps (J) | b (J) | A (J x d)]   d = n or 2n   (halfspace_params)
  HINGE_BALLS_2D / _3D  [sigma, eps, r | J x (W_j | c_j | tau_j) | 8 x (o_m | v_m | R_m)]   d = n or 2n   (balls_params)
"""
from __future__ import annotations

import numpy as np

PSI_RANGE_1D, PSI_QUAD_PRIOR, PSI_FIXED_PRIOR, PSI_HOST_CALLBACK, PSI_HINGE_SDF_2D = 0, 1, 2, 3, 4
PSI_HINGE_SDF_2D_BODY, PSI_HINGE_SDF_3D, PSI_HINGE_SDF_3D_ARM = 5, 6, 7
PSI_HINGE_SDF_2D_SEG, PSI_HINGE_SDF_3D_SEG = 8, 9
PSI_HINGE_BOX = 10
PSI_HINGE_HALFSPACE = 11
PSI_HINGE_BALLS_2D, PSI_HINGE_BALLS_3D = 13, 14       # 12 is not a kind
BALLS_MAX_M = 8           # ball slots of one HINGE_BALLS_* factor

CONFIGS = {
    # name: (cfg#, T, n, p, prior kind)
    "tiny": (0, 5, 2, 3, "minacc"),
    "c2": (2, 65, 2, 3, "minacc"),          # BASELINE.json configs[1]
    "c3mini": (31, 9, 6, 5, "ltv"),
    "c3small": (32, 33, 6, 5, "ltv"),
    "c3t2": (33, 2, 6, 5, "ltv"),           # shortest chains: one / two prior factors (tail blocks of the fused launches)
    "c3t3": (34, 3, 6, 5, "ltv"),
    "c3": (3, 1025, 6, 5, "ltv"),           # BASELINE.json configs[2] (headline)
    # the LITERAL SURVEY 8(d) C3 chain: dt = 0.05, seeded stable A_k (6 x 6) / B_k (6 x 3), two end anchors only.
    # cond(Hessian) ~ 1e7: kept for parity at operator level and for the checked conditioning bound (tests), not benched
    "c3lit": (36, 1025, 6, 5, "ltvlit"),
    "c3litmini": (37, 17, 6, 5, "ltvlit"),
    "c5mini": (51, 5, 12, 5, "ltv"),        # d = 24 slice (split kernel), N(24,5) = 243 905
    "c5small": (52, 33, 12, 6, "ltv", 5),   # d = 24, p = 6: N = 2 438 801; unary factors at p = 5
    "c5": (5, 4097, 12, 7, "ltv", 5),       # BASELINE.json configs[4]: N(24,7) = 20 557 057 (fp64, coded table)
}

# Physical scales.  They are chosen so that the joint Hessian is well conditioned (cond ~ 5e2 at
# T = 1025): a pure prior chain pinned only at its two ends has cond ~ 2e7 at T = 1025, dt = 0.05,
# and then NO two fp64 implementations of the reference algorithm (including the reference against
# itself under a different OpenMP schedule) agree to 1e-6 on the NGD iterate -- the solve
# amplifies the ~1e-11..1e-8 rounding of the GH sums (|w|_1 ~ 5e3 at (12,5)) by cond.  Hence every
# state also carries a unary Gaussian "measurement" factor (the batch-estimation graph of Barfoot
# et al. that src/1d_example.cpp cites): binary motion priors + unary factors on every state.
DT = {"minacc": 0.25, "ltv": 0.2}
QC = 0.8                  # minimum-acceleration power spectral density
B_SCALE = 3.0             # LTV input gain
KAPPA_UNARY, KAPPA_ANCHOR = 1.0, 50.0


def _minacc(nd, qc, dt):
    I = np.eye(nd)
    Phi = np.block([[I, dt * I], [np.zeros((nd, nd)), I]])
    iQc = np.eye(nd) / qc
    Qinv = np.block([[12 * iQc / dt ** 3, -6 * iQc / dt ** 2], [-6 * iQc / dt ** 2, 4 * iQc / dt]])
    return Phi, Qinv


def minacc_interpolation(nd, qc, dt, tau):
    """(A, B, Qt) of the constant-velocity prior of _minacc at time tau in [0, dt] between two support states:
    x(tau) | x_i, x_i+1 ~ N(A x_i + B x_i+1, Qt) with Psi = Q(tau) Phi(dt - tau)^T Q(dt)^-1, A = Phi(tau) - Psi Phi(dt), B = Psi,
    Qt = Q(tau) - Psi Phi(dt - tau) Q(tau) (Barfoot, Tong, Sarkka, RSS 2014).  The end points return exactly (I, 0, 0) and
    (0, I, 0): evaluated numerically Qt is rounding noise of either sign there."""
    n = 2 * nd
    if tau == 0:
        return np.eye(n), np.zeros((n, n)), np.zeros((n, n))
    if tau == dt:
        return np.zeros((n, n)), np.eye(n), np.zeros((n, n))
    assert 0 < tau < dt, "tau outside [0, dt]"
    I, Z = np.eye(nd), np.zeros((nd, nd))

    def Phi(t):
        return np.block([[I, t * I], [Z, I]])

    def Q(t):
        return qc * np.block([[t ** 3 / 3 * I, t ** 2 / 2 * I], [t ** 2 / 2 * I, t * I]])

    Psi = Q(tau) @ Phi(dt - tau).T @ _minacc(nd, qc, dt)[1]
    A = Phi(tau) - Psi @ Phi(dt)
    Qt = Q(tau) - Psi @ Phi(dt - tau) @ Q(tau)
    return A, Psi, (Qt + Qt.T) / 2


def minacc_segment_readout(nd, qc, dt, taus, npos):
    """(W [J][npos][2n], c [J][npos]) of the HINGE_SDF_*_SEG kinds for the constant-velocity prior of _minacc: check point j is
    the first npos rows (the position) of x(tau_j) = A(tau_j) x_i + B(tau_j) x_i+1, so W_j = [A rows | B rows] of
    minacc_interpolation and c_j = 0 (the prior has no input term)."""
    n = 2 * nd
    assert 1 <= npos <= n
    W = np.zeros((len(taus), npos, 2 * n))
    for j, tau in enumerate(taus):
        A, B, _ = minacc_interpolation(nd, qc, dt, tau)
        W[j, :, :n], W[j, :, n:] = A[:npos], B[:npos]
    return W, np.zeros((len(taus), npos))


def segment_params(sigma, eps, radius, W, c):
    """Parameter blocks [K][3 + J P (d + 1)] of a HINGE_SDF_*_SEG set: [sigma, eps, r | W_0 | c_0 | ... | W_{J-1} | c_{J-1}].
    W [J][P][d] and c [J][P] shared by the set, or [K][J][P][d] and [K][J][P] per factor; sigma, eps, radius scalars or [K]."""
    W, c = np.asarray(W, dtype=np.float64), np.asarray(c, dtype=np.float64)
    sig, eps, radius = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (sigma, eps, radius))
    K = max(sig.size, eps.size, radius.size, W.shape[0] if W.ndim == 4 else 1)
    if W.ndim == 3:
        W = np.broadcast_to(W, (K,) + W.shape)
    if c.ndim == 2:
        c = np.broadcast_to(c, (K,) + c.shape)
    assert W.ndim == 4 and c.shape == W.shape[:3] and W.shape[0] == K
    head = np.stack([np.broadcast_to(v, (K,)) for v in (sig, eps, radius)], axis=1)
    body = np.concatenate([W.reshape(K, W.shape[1], -1), c], axis=2).reshape(K, -1)
    return np.ascontiguousarray(np.concatenate([head, body], axis=1))


def _segment_spec(obstacle, kind, T, n, nd, dt, taus, npos, p=None, readout_order=0):
    """The segment set beside the obstacle set `obstacle`: one factor per pair of neighbouring states (K = T - 1, start =
    arange, d = 2n), check points at the times taus inside the segment, the obstacle set's sigma, eps, r and field; GH degree p
    (default: the obstacle set's).  readout_order > 0: the set takes the read-out-space rule of that order
    (gvi_factors_set_readout_rule; api.context_for_chain sets it)."""
    W, c = minacc_segment_readout(nd, QC, dt, taus, npos)
    P = obstacle["params"]
    spec = dict(kind=kind, d=2 * n, p=obstacle["p"] if p is None else p, start=np.arange(T - 1, dtype=np.int32),
                params=segment_params(P[:T - 1, 0], P[:T - 1, 1], P[:T - 1, 2], W, c), temperature=np.ones(T - 1),
                seg_W=W, seg_c=c, sdf_origin=obstacle["sdf_origin"], sdf_cell=obstacle["sdf_cell"], sdf_field=obstacle["sdf_field"])
    if readout_order:
        spec["readout_order"] = int(readout_order)
    return spec


def box_params(sigma, eps, lo, hi):
    """Parameter blocks [K][4 d] of a HINGE_BOX set: [sigma (d) | eps (d) | lo (d) | hi (d)].  Each argument is a scalar, [d]
    (shared by the set) or [K][d]; lo = -inf / hi = +inf switches a side off."""
    parts = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (sigma, eps, lo, hi)]
    d = max(v.shape[-1] for v in parts)
    K = max([v.shape[0] for v in parts if v.ndim == 2] + [1])
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(v, (K, d)) for v in parts], axis=1))


def add_box_set(chain, lo, hi, sigma=10.0, eps=0.05, p=3, pair=False, temperature=1.0):
    """A copy of `chain` (the arrays are shared) with a HINGE_BOX set appended behind its sets: one factor per state (d = n) or,
    pair = True, per pair of neighbouring states (d = 2n), limits lo / hi [d] with -inf / +inf for the coordinates and sides
    without one.  Velocity limits on make_planar_chain: lo = [-inf, -inf, -v, -v], hi = [inf, inf, v, v]; joint-angle and
    joint-rate limits on make_obstacle_chain("arm7"): lo = [q_min (7) | -w (7)], hi = [q_max (7) | w (7)]."""
    T, n = chain["T"], chain["n"]
    K, d = (T - 1, 2 * n) if pair else (T, n)
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,))
    spec = dict(kind=PSI_HINGE_BOX, d=d, p=p, start=np.arange(K, dtype=np.int32), params=np.tile(box_params(sigma, eps, lo, hi), (K, 1)),
                temperature=np.full(K, float(temperature)))
    return dict(chain, specs=list(chain["specs"]) + [spec])


def halfspace_params(sigma, eps, b, A, J=None):
    """Parameter blocks [K][J (d + 3)] of a HINGE_HALFSPACE set: [sigma (J) | eps (J) | b (J) | A (J x d, row-major)], rows
    a_j^T x <= b_j.  A is [J][d] (shared by the set), [K][J][d], or a list of K arrays [J_k][d] with their own row counts;
    sigma, eps, b are scalars, [J], [K][J] or, beside a list A, lists of [J_k].  Every factor is padded to J rows (default:
    the largest row count) with rows that are off: sigma = 0, eps = b = 0, a = 0."""
    ragged = isinstance(A, (list, tuple)) and all(np.ndim(a) == 2 for a in A)
    if ragged:
        blocks = [np.asarray(a, dtype=np.float64) for a in A]
        K = len(blocks)

        def per(v, k):
            v = v[k] if isinstance(v, (list, tuple)) else v
            return np.broadcast_to(np.asarray(v, dtype=np.float64), (blocks[k].shape[0],))
        rows = [[per(v, k) for k in range(K)] for v in (sigma, eps, b)]
    else:
        A = np.asarray(A, dtype=np.float64)
        assert A.ndim in (2, 3), "A is [J][d] or [K][J][d]"
        parts = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (sigma, eps, b)]
        K = max([v.shape[0] for v in parts if v.ndim == 2] + [A.shape[0] if A.ndim == 3 else 1])
        blocks = list(np.broadcast_to(A, (K,) + A.shape[-2:]))
        rows = [list(np.broadcast_to(v, (K, A.shape[-2]))) for v in parts]
    d = blocks[0].shape[1]
    Jmax = max(a.shape[0] for a in blocks)
    J = Jmax if J is None else int(J)
    assert J >= Jmax and all(a.shape[1] == d for a in blocks), "J below a factor's row count, or rows of different dimension"
    out = np.zeros((K, J * (d + 3)))
    for k in range(K):
        Jk = blocks[k].shape[0]
        for slot in range(3):
            out[k, slot * J:slot * J + Jk] = rows[slot][k]
        out[k, 3 * J:3 * J + Jk * d] = blocks[k].reshape(-1)
    return out


def add_corridor_set(chain, normals, offsets, sigma=10.0, eps=0.05, p=3, pair=False, taus=None, dt=0.25, qc=QC, temperature=1.0):
    """A copy of `chain` (the arrays are shared) with a HINGE_HALFSPACE set appended behind its sets: a convex corridor
    n_j^T pos <= b_j on the first npos coordinates (the position) of the state, normals [Jn][npos] and offsets [Jn] shared by
    the set, or [K][Jn][npos] and [K][Jn] with one polygon per factor.
    pair = False: one factor per state (K = T, d = n), rows [n_j | 0].
    pair = True: one factor per pair of neighbouring states (K = T - 1, d = 2n) that holds the corridor at the times taus
    (default: the midpoint dt / 2) INSIDE the segment: the position there is W(tau) [x_i | x_i+1] + c(tau) (minacc_segment_readout
    for the chain's constant-velocity prior with step dt and spectral density qc), so the rows are W(tau)^T n_j with offsets
    b_j - n_j^T c(tau): J = len(taus) Jn rows, tau-major."""
    T, n = chain["T"], chain["n"]
    K, d = (T - 1, 2 * n) if pair else (T, n)
    normals, offsets = np.asarray(normals, dtype=np.float64), np.asarray(offsets, dtype=np.float64)
    Jn, npos = normals.shape[-2:]
    N = np.broadcast_to(normals, (K, Jn, npos))
    B = np.broadcast_to(offsets, (K, Jn))
    if pair:
        taus = [0.5 * dt] if taus is None else list(taus)
        W, c = minacc_segment_readout(n // 2, qc, dt, taus, npos)                 # [L][npos][2n], [L][npos]
        A = np.einsum("kjp,lpe->klje", N, W).reshape(K, len(taus) * Jn, d)
        b = (B[:, None, :] - np.einsum("kjp,lp->klj", N, c)).reshape(K, len(taus) * Jn)
    else:
        A = np.zeros((K, Jn, d))
        A[:, :, :npos] = N
        b = B
    spec = dict(kind=PSI_HINGE_HALFSPACE, d=d, p=p, start=np.arange(K, dtype=np.int32), params=halfspace_params(sigma, eps, b, A),
                temperature=np.full(K, float(temperature)))
    return dict(chain, specs=list(chain["specs"]) + [spec])


def balls_params(sigma, eps, r, W, c, tau, centres, velocities, radii):
    """Parameter blocks [K][3 + J (P (d + 1) + 1) + 8 (2 P + 1)] of a HINGE_BALLS_2D / _3D set:
    [sigma, eps, r | J x (W_j | c_j | tau_j) | 8 x (o_m | v_m | R_m)].  W [J][P][d], c [J][P] and tau [J] shared by the set, or
    [K][J][P][d], [K][J][P], [K][J] per factor; centres [M][P], velocities [M][P] and radii [M] one scene for every factor, or
    [K][M][P], [K][M][P], [K][M] per factor, M <= 8: the remaining slots are empty (radius -inf, centre and velocity 0).
    sigma, eps, r scalars or [K]."""
    W, c, tau = (np.asarray(v, dtype=np.float64) for v in (W, c, tau))
    o, v, R = (np.asarray(x, dtype=np.float64) for x in (centres, velocities, radii))
    sig, eps, r = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (sigma, eps, r))
    K = max(sig.size, eps.size, r.size, W.shape[0] if W.ndim == 4 else 1, o.shape[0] if o.ndim == 3 else 1,
            v.shape[0] if v.ndim == 3 else 1, R.shape[0] if R.ndim == 2 else 1)
    J, P = W.shape[-3], W.shape[-2]
    W = np.broadcast_to(W, (K,) + W.shape[-3:])
    c = np.broadcast_to(c, (K, J, P))
    tau = np.broadcast_to(tau, (K, J))
    M = R.shape[-1] if R.ndim else 0
    assert M <= BALLS_MAX_M, "a factor has 8 ball slots"
    slots = np.zeros((K, BALLS_MAX_M, 2 * P + 1))
    slots[:, :, 2 * P] = -np.inf
    if M:
        slots[:, :M, :P] = np.broadcast_to(o, (K, M, P))
        slots[:, :M, P:2 * P] = np.broadcast_to(v, (K, M, P))
        slots[:, :M, 2 * P] = np.broadcast_to(R, (K, M))
    head = np.stack([np.broadcast_to(x, (K,)) for x in (sig, eps, r)], axis=1)
    body = np.concatenate([W.reshape(K, J, -1), c, tau[:, :, None]], axis=2).reshape(K, -1)
    return np.ascontiguousarray(np.concatenate([head, body, slots.reshape(K, -1)], axis=1))


def add_moving_obstacle_set(chain, centres0, velocities, radii, sigma=15.0, eps=0.2, r=0.1, p=3, taus=None, dt=0.25, qc=QC,
                            temperature=1.0, readout_order=0):
    """A copy of `chain` (the arrays are shared) with a HINGE_BALLS_2D / _3D set appended behind its sets: balls m with centres
    centres0 [M][P] at time 0, constant velocities [M][P] and radii [M] (M <= 8; P = 2 or 3 picks the kind).  State i has the
    time t_i = i dt, and factor i of the set carries ball m at centres0_m + t_i v_m with velocity v_m.
    taus = None: one factor per state (K = T, d = n) on the state's position, J = 1, tau = 0.
    taus given: one factor per pair of neighbouring states (K = T - 1, d = 2n) on the GP-interpolated positions at the times
    taus inside the segment (minacc_segment_readout for the chain's constant-velocity prior with step dt and spectral density
    qc), tau_j = taus[j]: check point j meets the balls where they are at t_i + taus[j]."""
    T, n = chain["T"], chain["n"]
    o0, v = np.atleast_2d(np.asarray(centres0, dtype=np.float64)), np.atleast_2d(np.asarray(velocities, dtype=np.float64))
    P = o0.shape[1]
    assert P in (2, 3) and v.shape == o0.shape
    if taus is None:
        K, d = T, n
        W = np.zeros((1, P, n))
        W[0, :, :P] = np.eye(P)
        c, tau = np.zeros((1, P)), np.zeros(1)
    else:
        K, d = T - 1, 2 * n
        W, c = minacc_segment_readout(n // 2, qc, dt, list(taus), P)
        tau = np.asarray(taus, dtype=np.float64)
    t = dt * np.arange(K)
    centres = o0[None, :, :] + t[:, None, None] * v[None, :, :]
    params = balls_params(sigma, eps, r, W, c, tau, centres, np.broadcast_to(v, centres.shape), np.broadcast_to(radii, (K, o0.shape[0])))
    spec = dict(kind=PSI_HINGE_BALLS_2D if P == 2 else PSI_HINGE_BALLS_3D, d=d, p=p, start=np.arange(K, dtype=np.int32), params=params,
                temperature=np.full(K, float(temperature)))
    if readout_order:                   # the read-out-space rule of that order (gvi_factors_set_readout_rule; api.context_for_chain sets it)
        spec["readout_order"] = int(readout_order)
    return dict(chain, specs=list(chain["specs"]) + [spec])


def _ltv_system(rng, nd):
    """Four (A, B) pairs -- one per piece-wise-constant sub-interval -- of a seeded stable second-order system
    x'' = -Kp x - Kd x' + B2 u (state [x, x']): the hA / hB entries LTV_GP reads (gp/LTV_prior.h:57-61)."""
    out = []
    for _ in range(4):
        Kp = np.diag(rng.uniform(0.5, 2.0, nd)) + 0.1 * rng.normal(size=(nd, nd))
        Kd = np.diag(rng.uniform(0.5, 1.5, nd)) + 0.1 * rng.normal(size=(nd, nd))
        A = np.block([[np.zeros((nd, nd)), np.eye(nd)], [-Kp, -Kd]])
        B = np.vstack([np.zeros((nd, nd)), B_SCALE * (np.eye(nd) + 0.1 * rng.normal(size=(nd, nd)))])
        out.append((A, B))
    return out


def _ltv_from_system(system, dt):
    """Exact discretisation over the 4 sub-intervals (product of matrix exponentials, Van Loan block form for the Gramian):
    the maths of gp/LTV_prior.h:123-197."""
    from scipy.linalg import expm
    n = system[0][0].shape[0]
    Phi, Q = np.eye(n), np.zeros((n, n))
    h = dt / 4
    for A, B in system:
        M = np.zeros((2 * n, 2 * n))
        M[:n, :n], M[:n, n:], M[n:, n:] = -A, B @ B.T, A.T
        E = expm(M * h)
        Ad = E[n:, n:].T
        Qd = Ad @ E[:n, n:]
        Phi = Ad @ Phi
        Q = Ad @ Q @ Ad.T + (Qd + Qd.T) / 2
    return Phi, np.linalg.inv(Q)


def _ltv(rng, nd, dt):
    """(Phi, Q^-1) of one seeded LTV prior factor."""
    return _ltv_from_system(_ltv_system(rng, nd), dt)


def ltv_chain_system(name: str):
    """The (hA, hB) lists behind make_chain(name)'s LTV priors, in LTV_GP's layout: 4 (T - 1) + 1 matrices each, factor k
    reading entries 4k .. 4k + 4 (the 5th is only touched at t = delta_t exactly; here the next factor's first)."""
    cfg, T, n, p, kind = CONFIGS[name][:5]
    assert kind == "ltv"
    rng = np.random.default_rng(0x5EED + cfg)
    hA, hB = [], []
    for k in range(T - 1):
        for A, B in _ltv_system(rng, n // 2):
            hA.append(A); hB.append(B)
    hA.append(hA[-1].copy()); hB.append(hB[-1].copy())
    return np.stack(hA), np.stack(hB)


def _ltv_literal(rng, n, dt):
    """SURVEY 8(d) C3 as written: (Phi_k, Q_k^-1) = exact discretisation over 4 piece-wise-constant sub-intervals (product of
    matrix exponentials / Van Loan) of a seeded STABLE A_k (n x n, spectral radius <= 1) and B_k (n x n/2) -- the maths of
    gp/LTV_prior.h:123-197 without GSL."""
    from scipy.linalg import expm
    Phi, Q = np.eye(n), np.zeros((n, n))
    h = dt / 4
    for _ in range(4):
        G = rng.normal(size=(n, n))
        G = G - (np.linalg.eigvals(G).real.max() + 0.1) * np.eye(n)            # stable: Re(lambda) < 0
        A = G / max(1.0, np.abs(np.linalg.eigvals(G)).max())                   # spectral radius <= 1
        B = rng.normal(size=(n, n // 2))
        M = np.zeros((2 * n, 2 * n))
        M[:n, :n], M[:n, n:], M[n:, n:] = -A, B @ B.T, A.T
        E = expm(M * h)
        Ad = E[n:, n:].T
        Qd = Ad @ E[:n, n:]
        Phi = Ad @ Phi
        Q = Ad @ Q @ Ad.T + (Qd + Qd.T) / 2
    return Phi, np.linalg.inv(Q)


def make_literal_chain(name: str):
    """The literal BASELINE configs[2] chain of SURVEY 8(d): T - 1 LTV-form priors (d = 2n) and TWO FixedPriorGP end anchors
    (K0 = 1e-2 I) -- no unary factor on the interior states; start state = straight line + N(0, 0.05^2) jitter, initial
    precision = sum of the factor Hessians."""
    cfg, T, n, p, kind = CONFIGS[name][:5]
    rng = np.random.default_rng(0x5EED + cfg)
    K, dt = T - 1, 0.05
    Phi = np.zeros((K, n, n))
    Qinv = np.zeros((K, n, n))
    for k in range(K):
        Phi[k], Qinv[k] = _ltv_literal(rng, n, dt)
    goal = rng.uniform(1.0, 2.0, n)
    t = np.arange(T)[:, None] / (T - 1)
    nominal = goal[None, :] * t
    mu0 = nominal + 0.05 * rng.normal(size=nominal.shape)
    anchors = np.stack([nominal[0], nominal[-1]])
    Kinv = np.stack([np.eye(n) / 1e-2] * 2)
    D0 = np.zeros((T, n, n))
    U0 = np.zeros((T - 1, n, n))
    for k in range(K):
        Lam = np.hstack([-Phi[k], np.eye(n)])
        M = Lam.T @ Qinv[k] @ Lam
        D0[k] += M[:n, :n]
        D0[k + 1] += M[n:, n:]
        U0[k] += M[:n, n:]
    D0[0] += 2 * Kinv[0]
    D0[-1] += 2 * Kinv[1]
    specs = [
        dict(kind=PSI_QUAD_PRIOR, d=2 * n, p=p, start=np.arange(K, dtype=np.int32),
             params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1),
             temperature=np.ones(K), Phi=Phi, Qinv=Qinv),
        dict(kind=PSI_FIXED_PRIOR, d=n, p=p, start=np.array([0, T - 1], dtype=np.int32),
             params=np.concatenate([anchors, Kinv.reshape(2, -1)], axis=1), temperature=np.ones(2), mu0=anchors, Kinv=Kinv),
    ]
    return dict(name=name, T=T, n=n, specs=specs, mu0=mu0, D0=D0, U0=U0)


def make_chain(name: str):
    """Returns dict(T, n, specs, mu0, D0, U0).  specs[0]: the T-1 binary prior factors (d = 2n,
    QUAD_PRIOR); specs[1]: T unary measurement factors (d = n, FIXED_PRIOR), the first and the last
    being the strong end anchors.  "planar1k" / "planar": the planning graph with hinge-on-SDF obstacle factors
    (make_planar_chain); "arm7x": the 7-DOF arm graph (make_obstacle_chain) at T = 129."""
    if name == "planar1k":          # bench.py --config planar1k: 1025 states, 1025 obstacle factors d = 4 at p = 7 (2145 points)
        ch = make_planar_chain(T=1025, p=3, p_obstacle=7)
        ch["name"] = name
        # obstacle factors at the reference's HIGH temperature (gvibase/GVI-GH-impl.h:104-117 switches to it when the line search
        # is exhausted; its planar experiments start there): at T_k = 1 the hinge rejects every step after two iterations
        ch["specs"][1]["temperature"] = np.full(len(ch["specs"][1]["start"]), 30.0)
        return ch
    if name == "planar":
        return make_planar_chain()
    if name == "arm7x":
        ch = make_obstacle_chain("arm7", T=129)
        ch["name"] = name
        ch["specs"][1]["temperature"] = np.full(len(ch["specs"][1]["start"]), 30.0)
        return ch
    if name not in CONFIGS and name.startswith("c3x") and name[3:].isdigit():
        CONFIGS[name] = (3, 1024 * int(name[3:]) + 1, 6, 5, "ltv")      # weak-scaling family: 1024 factors per GPU
    if CONFIGS[name][4] == "ltvlit":
        return make_literal_chain(name)
    cfg, T, n, p, kind = CONFIGS[name][:5]
    p_unary = CONFIGS[name][5] if len(CONFIGS[name]) > 5 else p
    rng = np.random.default_rng(0x5EED + cfg)
    nd, K = n // 2, T - 1
    dt = DT[kind]
    Phi = np.zeros((K, n, n))
    Qinv = np.zeros((K, n, n))
    for k in range(K):
        Phi[k], Qinv[k] = _minacc(nd, QC, dt) if kind == "minacc" else _ltv(rng, nd, dt)
    # nominal trajectory: straight line with constant velocity; start state = nominal + jitter
    goal = rng.uniform(1.0, 2.0, nd)
    t = np.arange(T)[:, None] * dt
    horizon = (T - 1) * dt
    nominal = np.hstack([goal[None, :] * t / horizon, np.tile(goal / horizon, (T, 1))])
    mu0 = nominal + 0.05 * rng.normal(size=nominal.shape)
    meas = nominal + 0.1 * rng.normal(size=nominal.shape)     # unary factor means
    meas[0], meas[-1] = nominal[0], nominal[-1]
    kappa = np.full(T, KAPPA_UNARY)
    kappa[0] = kappa[-1] = KAPPA_ANCHOR
    Kinv = kappa[:, None, None] * np.eye(n)[None]
    # initial precision: 0.7 x (sum of factor Hessians) -- PD block-tridiagonal
    D0 = np.zeros((T, n, n))
    U0 = np.zeros((T - 1, n, n))
    for k in range(K):
        Lam = np.hstack([-Phi[k], np.eye(n)])
        M = Lam.T @ Qinv[k] @ Lam
        D0[k] += M[:n, :n]
        D0[k + 1] += M[n:, n:]
        U0[k] += M[:n, n:]
    D0 += 2 * Kinv
    D0, U0 = 0.7 * D0, 0.7 * U0
    specs = [
        dict(kind=PSI_QUAD_PRIOR, d=2 * n, p=p, start=np.arange(K, dtype=np.int32),
             params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1),
             temperature=np.ones(K), Phi=Phi, Qinv=Qinv),
        dict(kind=PSI_FIXED_PRIOR, d=n, p=p_unary, start=np.arange(T, dtype=np.int32),
             params=np.concatenate([meas, Kinv.reshape(T, -1)], axis=1),
             temperature=np.ones(T), mu0=meas, Kinv=Kinv),
    ]
    return dict(name=name, T=T, n=n, specs=specs, mu0=mu0, D0=D0, U0=U0)


def circle_sdf(origin, cell, rows, cols, centers, radii):
    """Signed distance to a union of discs on a grid: field[r, c] at (origin + (c, r) * cell)."""
    xs = origin[0] + np.arange(cols) * cell
    ys = origin[1] + np.arange(rows) * cell
    X, Y = np.meshgrid(xs, ys)
    f = np.full((rows, cols), np.inf)
    for (cx, cy), r in zip(centers, radii):
        f = np.minimum(f, np.hypot(X - cx, Y - cy) - r)
    return f


def make_planar_chain(T=17, p=3, seed=0x5EED + 40, jitter=0.02, p_obstacle=None, horizon=None, segment_taus=None, segment_p=None,
                      readout_order=0):
    """Planar point-robot planning graph of the reference's own GPU workload: states
    [x, y, vx, vy] (n = 4), T-1 minimum-acceleration priors (d = 8), T hinge-on-SDF obstacle factors on
    every state (d = 4, helpers/CudaOperation.h:491-523) and two fixed-prior end anchors.  p_obstacle: GH degree of the
    obstacle factors (default p + 1); horizon: total time (default (T - 1) / 4, i.e. dt = 0.25).  segment_taus: times in [0, dt]
    of the check points of an additional HINGE_SDF_2D_SEG set on every pair of neighbouring states (d = 8), inserted behind the
    obstacle set (specs = priors, obstacles, segments, anchors), at GH degree segment_p (default: the obstacle factors');
    readout_order > 0 puts that segment set on the read-out-space rule of that order."""
    rng = np.random.default_rng(seed)
    n, nd, K = 4, 2, T - 1
    dt = 0.25 if horizon is None else horizon / (T - 1)
    Phi1, Qinv1 = _minacc(nd, QC, dt)
    Phi, Qinv = np.stack([Phi1] * K), np.stack([Qinv1] * K)
    start_xy, goal_xy = np.array([-3.0, -0.4]), np.array([3.0, 0.4])
    horizon = (T - 1) * dt
    vel = (goal_xy - start_xy) / horizon
    t = np.arange(T)[:, None] * dt
    nominal = np.hstack([start_xy[None] + vel[None] * t, np.tile(vel, (T, 1))])
    mu0 = nominal + jitter * rng.normal(size=nominal.shape)
    origin, cell, rows, cols = (-5.0, -4.0), 0.1, 81, 101
    field = circle_sdf(origin, cell, rows, cols, [(0.0, 1.6), (-1.0, -2.2)], [1.2, 0.9])
    anchors = np.stack([nominal[0], nominal[-1]])
    Kinv = np.stack([np.eye(n) / 1e-2] * 2)
    D0 = np.zeros((T, n, n)); U0 = np.zeros((T - 1, n, n))
    for k in range(K):
        Lam = np.hstack([-Phi[k], np.eye(n)])
        M = Lam.T @ Qinv[k] @ Lam
        D0[k] += M[:n, :n]; D0[k + 1] += M[n:, n:]; U0[k] += M[:n, n:]
    D0[0] += 2 * Kinv[0]; D0[-1] += 2 * Kinv[1]
    D0 += 0.5 * np.eye(n)
    specs = [
        dict(kind=PSI_QUAD_PRIOR, d=2 * n, p=p, start=np.arange(K, dtype=np.int32),
             params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1), temperature=np.ones(K), Phi=Phi, Qinv=Qinv),
        dict(kind=PSI_HINGE_SDF_2D, d=n, p=p + 1 if p_obstacle is None else p_obstacle, start=np.arange(T, dtype=np.int32),
             params=np.tile(np.array([[15.5, 0.5, 0.3]]), (T, 1)), temperature=np.ones(T),
             sdf_origin=origin, sdf_cell=cell, sdf_field=field),
        dict(kind=PSI_FIXED_PRIOR, d=n, p=p, start=np.array([0, T - 1], dtype=np.int32),
             params=np.concatenate([anchors, Kinv.reshape(2, -1)], axis=1), temperature=np.ones(2), mu0=anchors, Kinv=Kinv),
    ]
    if segment_taus is not None:
        specs.insert(2, _segment_spec(specs[1], PSI_HINGE_SDF_2D_SEG, T, n, nd, dt, segment_taus, 2, segment_p, readout_order))
    return dict(name="planar", T=T, n=n, specs=specs, mu0=mu0, D0=D0, U0=U0)


def sphere_sdf3d(origin, cell, rows, cols, nz, centers, radii):
    """Signed distance to a union of balls: field[r, c, z] at origin + (c, r, z) * cell."""
    xs = origin[0] + np.arange(cols) * cell
    ys = origin[1] + np.arange(rows) * cell
    zs = origin[2] + np.arange(nz) * cell
    Y, X, Zz = np.meshgrid(ys, xs, zs, indexing="ij")
    f = np.full((rows, cols, nz), np.inf)
    for (cx, cy, cz), r in zip(centers, radii):
        f = np.minimum(f, np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Zz - cz) ** 2) - r)
    return f


def make_obstacle_chain(kind: str, T=9, p=3, seed=0x5EED + 41, segment_taus=None, segment_p=None, readout_order=0):
    """n = 6 planning graphs of the reference's other two obstacle workloads: "quad2d" (planar quadrotor,
    state [x, z, phi, vx, vz, w], body of 5 check points, helpers/CudaOperation.h:565-606) and "pr3d" (3-D point
    robot, state [x, y, z, v], trilinear field, :650-683): minimum-acceleration priors (d = 12), one obstacle
    factor per state (d = 6) and two end anchors.  segment_taus ("pr3d" only): as for make_planar_chain, a HINGE_SDF_3D_SEG set
    (d = 12) behind the obstacle set, on the read-out-space rule where readout_order > 0."""
    rng = np.random.default_rng(seed + {"quad2d": 0, "pr3d": 1, "arm7": 2}[kind])
    nd = 7 if kind == "arm7" else 3
    n, K = 2 * nd, T - 1
    if kind == "arm7":
        p = 3                                    # d = 28 priors: N(28,3) = 1625 sigma points (p = 2 is not exact for Vddmu)
    dt = 0.25
    Phi1, Qinv1 = _minacc(nd, QC, dt)
    Phi, Qinv = np.stack([Phi1] * K), np.stack([Qinv1] * K)
    horizon = (T - 1) * dt
    if kind == "quad2d":
        start, goal = np.array([-3.0, -0.5, 0.2]), np.array([3.0, 0.6, -0.1])
        origin, cell = (-6.0, -5.0), 0.1
        field = circle_sdf(origin, cell, 101, 121, [(0.0, 2.2), (-1.0, -3.0)], [1.2, 0.9])
        obst = dict(kind=PSI_HINGE_SDF_2D_BODY, params=np.tile(np.array([[15.5, 0.5, 0.3, 5.0, 5.0, 1.0]]), (T, 1)))
    elif kind == "arm7":
        start = np.array([-0.8, 0.5, 0.3, 1.2, -0.4, 0.6, 0.0])
        goal = np.array([0.7, 0.9, -0.2, 0.8, 0.3, 0.2, 0.4])
        origin, cell = (-1.5, -1.5, -0.5), 0.05
        field = sphere_sdf3d(origin, cell, 61, 61, 41, [(0.4, 0.2, 0.5), (-0.3, -0.4, 0.3)], [0.25, 0.2])
        obst = dict(kind=PSI_HINGE_SDF_3D_ARM, params=np.tile(np.array([[15.5, 0.1]]), (T, 1)), arm=wam_like_arm())
    else:
        start, goal = np.array([-2.0, -0.5, 0.0]), np.array([2.0, 0.5, 0.6])
        origin, cell = (-4.0, -3.0, -2.0), 0.2
        field = sphere_sdf3d(origin, cell, 31, 41, 21, [(0.0, 1.4, 0.3), (-0.5, -1.8, 0.0)], [1.0, 0.8])
        obst = dict(kind=PSI_HINGE_SDF_3D, params=np.tile(np.array([[15.5, 0.5, 0.3]]), (T, 1)))
    vel = (goal - start) / horizon
    t = np.arange(T)[:, None] * dt
    nominal = np.hstack([start[None] + vel[None] * t, np.tile(vel, (T, 1))])
    mu0 = nominal + 0.02 * rng.normal(size=nominal.shape)
    anchors = np.stack([nominal[0], nominal[-1]])
    Kinv = np.stack([np.eye(n) / 1e-2] * 2)
    D0 = np.zeros((T, n, n)); U0 = np.zeros((T - 1, n, n))
    for k in range(K):
        Lam = np.hstack([-Phi[k], np.eye(n)])
        M = Lam.T @ Qinv[k] @ Lam
        D0[k] += M[:n, :n]; D0[k + 1] += M[n:, n:]; U0[k] += M[:n, n:]
    D0[0] += 2 * Kinv[0]; D0[-1] += 2 * Kinv[1]
    D0 += 0.5 * np.eye(n)
    specs = [
        dict(kind=PSI_QUAD_PRIOR, d=2 * n, p=p, start=np.arange(K, dtype=np.int32),
             params=np.concatenate([Phi.reshape(K, -1), Qinv.reshape(K, -1)], axis=1), temperature=np.ones(K), Phi=Phi, Qinv=Qinv),
        dict(d=n, p=p if kind == "arm7" else p + 1, start=np.arange(T, dtype=np.int32), temperature=np.ones(T),
             sdf_origin=origin, sdf_cell=cell, sdf_field=field, **obst),
        dict(kind=PSI_FIXED_PRIOR, d=n, p=p, start=np.array([0, T - 1], dtype=np.int32),
             params=np.concatenate([anchors, Kinv.reshape(2, -1)], axis=1), temperature=np.ones(2), mu0=anchors, Kinv=Kinv),
    ]
    if segment_taus is not None:
        assert kind == "pr3d", "segment factors are built for the point robots"
        specs.insert(2, _segment_spec(specs[1], PSI_HINGE_SDF_3D_SEG, T, n, nd, dt, segment_taus, 3, segment_p, readout_order))
    return dict(name=kind, T=T, n=n, specs=specs, mu0=mu0, D0=D0, U0=U0)


def wam_like_arm(nspheres=16):
    """A 7-DOF arm in DH form (Barrett-WAM-like link lengths) with collision spheres on its frames -- the inputs of
    the reference's CudaOperation_3dArm / ForwardKinematics (helpers/CudaOperation.h:325-399, 686-716)."""
    rng = np.random.default_rng(0x5EED + 60)
    h = np.pi / 2
    frames = np.array([0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6][:nspheres], dtype=np.int32)
    return dict(a=np.array([0.0, 0.0, 0.045, -0.045, 0.0, 0.0, 0.0]), alpha=np.array([-h, h, -h, h, -h, h, 0.0]),
                d=np.array([0.0, 0.0, 0.55, 0.0, 0.3, 0.0, 0.06]), theta_bias=np.zeros(7), frames=frames,
                centers=0.05 * rng.normal(size=(len(frames), 3)), radii=rng.uniform(0.05, 0.12, len(frames)))


def random_marginals(rng, K, d, scale=1.0):
    """Seeded (mu_k, Sigma_k) with SPD Sigma_k, for operator-level parity tests."""
    mu = rng.normal(size=(K, d))
    B = rng.normal(size=(K, d, d))
    Sigma = scale * (B @ np.transpose(B, (0, 2, 1)) / d + 0.2 * np.eye(d))
    return mu, Sigma
