"""Inputs and references for the tests of the FACTORISATION half of the chain kernels -- half log-determinant and selected
inverse (test_chain_selinv_host.py, test_chain_selinv_gpu.py); numpy only, no GPU.

selinv is the textbook sequential recursion over the chain, one node after the other from the left: an algorithm that shares
nothing with the kernels' segmented cyclic reduction (no levels, no passes, no parity buffers, no padding), generic over float64
and np.longdouble.  A is the symmetric block-tridiagonal matrix with diagonal blocks D[t] and A[t, t + 1] = U[t]:
  S_0 = D_0,  S_t = D_t - U_{t-1}^T S_{t-1}^-1 U_{t-1};            1/2 log det A = 1/2 sum_t sum(log(pivots of S_t));
  (pivots of S_t: the natural pivots of the hand-written Gauss-Jordan in longdouble; in float64 the squares of the diagonal of
  numpy's Cholesky factor, which are the same numbers)
  SD_{T-1} = S_{T-1}^-1,  G_t = S_t^-1 U_t,  SU_t = -G_t SD_{t+1},  SD_t = S_t^-1 + G_t SD_{t+1} G_t^T,
SD[t] = (A^-1)[t, t], SU[t] = (A^-1)[t, t + 1].

The case table reuses chain_pivot_ref's plan restatement and lengths (the lengths where the pass plan changes, per block size)
and adds what the solve's table lacks: a fourth pass at every N >= 6 (n = 5, 6: T = 49153, one past the largest three-pass
length 49152 -- chain_passes gives FOUR passes, (0, 5) (5, 5) (10, 5) and the top pass from level 15; n = 7, 8: T = 6145;
n = 12, 16: T = 513, the first four-pass length) and a third pass at N = 1 (T = 4097).  Ten short rows have a FULL last
segment in their earlier passes (see LENGTHS below).  The padded sizes n = 9, 11, 13 have
their three-pass length 130 and n = 7 its 385 in the solve's table already."""
import functools

import numpy as np

import chain_pivot_ref as P
from chain_pivot_ref import chain_levels, chain_passes, node_level, padded, pass_of  # noqa: F401  (the tests' one import)


# ---- the sequential recursion ----
def _gauss_jordan(S):
    """(S^-1, pivots) of a symmetric positive definite block by Gauss-Jordan with the natural pivots, in S's own dtype"""
    n = S.shape[0]
    M = np.concatenate([S, np.eye(n, dtype=S.dtype)], axis=1)
    piv = np.empty(n, dtype=S.dtype)
    for p in range(n):
        piv[p] = M[p, p]
        M[p] = M[p] / M[p, p]
        f = M[:, p].copy()
        f[p] = 0
        M -= f[:, None] * M[p][None, :]
    return M[:, n:], piv


def _inverse_logpiv(S):
    """(S^-1, sum(log(pivots)) / 2; NaN where a pivot is not positive)"""
    if S.dtype == np.float64:
        try:
            L = np.linalg.cholesky(S)                                 # pivots of the LDL^T form = diag(L)^2
        except np.linalg.LinAlgError:
            return np.linalg.inv(S), np.float64(np.nan)
        return np.linalg.inv(S), np.log(np.diagonal(L)).sum()
    Si, piv = _gauss_jordan(S)
    if not (piv > 0).all():
        return Si, S.dtype.type(np.nan)
    return Si, np.log(piv).sum() / 2


def selinv(D, U, dtype=np.float64):
    """(SD [T, n, n], SU [T - 1, n, n], half log-det) in dtype (float64 or np.longdouble)"""
    D, U = np.asarray(D, dtype=dtype), np.asarray(U, dtype=dtype)
    T, n = D.shape[:2]
    Sinv, G = np.empty((T, n, n), dtype=dtype), np.empty((max(T - 1, 0), n, n), dtype=dtype)
    hld = dtype(0)
    S = D[0]
    for t in range(T):
        Sinv[t], lp = _inverse_logpiv(S)
        hld = hld + lp
        if t + 1 < T:
            G[t] = Sinv[t] @ U[t]
            S = D[t + 1] - U[t].T @ G[t]
    SD, SU = np.empty((T, n, n), dtype=dtype), np.empty((max(T - 1, 0), n, n), dtype=dtype)
    SD[T - 1] = Sinv[T - 1]
    for t in range(T - 2, -1, -1):
        SU[t] = -G[t] @ SD[t + 1]
        SD[t] = Sinv[t] - SU[t] @ G[t].T
    return SD, SU, hld


def solve(D, U, rhs):
    """A^-1 rhs in float64 by the same left-to-right recursion (block Thomas); rhs [T, n]"""
    T, n = rhs.shape
    Sinv, y = np.empty((T, n, n)), np.empty((T, n))
    S, r = D[0], rhs[0]
    for t in range(T):
        Sinv[t] = np.linalg.inv(S)
        y[t] = r
        if t + 1 < T:
            G = Sinv[t] @ U[t]
            S, r = D[t + 1] - U[t].T @ G, rhs[t + 1] - G.T @ y[t]
    x = np.empty((T, n))
    x[T - 1] = Sinv[T - 1] @ y[T - 1]
    for t in range(T - 2, -1, -1):
        x[t] = Sinv[t] @ (y[t] - U[t] @ x[t + 1])
    return x


def dense_selinv(D, U):
    """the same three results from numpy's dense inverse and slogdet"""
    T, n = D.shape[:2]
    A = P.dense(D, U)
    Ai = np.linalg.inv(A)
    SD = np.stack([Ai[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    SU = np.stack([Ai[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] for t in range(T - 1)]) if T > 1 else np.zeros((0, n, n))
    sign, logdet = np.linalg.slogdet(A)
    assert sign > 0
    return SD, SU, logdet / 2


def rel(a, b):
    """max |a - b| relative to the largest entry of b (test_gpu_parity.rel), in the operands' dtype"""
    s = np.abs(b).max() if np.size(b) else 0
    return float(np.abs(a - b).max() / (s if s > 0 else 1)) if np.size(b) else 0.0


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- generators: read-only arrays, computed once ----
@functools.lru_cache(maxsize=None)
def well(T, n, seed):
    """test_gpu_parity._spd_chain: per link a random 2n x 2n matrix B B^T / 2n + 0.3 I, overlapped; condition about 17"""
    from test_gpu_parity import _spd_chain
    return _frozen(*_spd_chain(T, n, np.random.default_rng(seed)))


@functools.lru_cache(maxsize=None)
def stiff(T, n, seed):
    """per link M = B B^T / n + 1e-6 I with B of shape (2n, n) -- rank n of 2n, the rest at 1e-6 -- overlapped as in _spd_chain;
    condition about 1e7"""
    rng = np.random.default_rng(seed)
    D, U = np.zeros((T, n, n)), np.zeros((T - 1, n, n))
    for i in range(T - 1):
        B = rng.normal(size=(2 * n, n))
        M = B @ B.T / n + 1e-6 * np.eye(2 * n)
        D[i] += M[:n, :n]
        D[i + 1] += M[n:, n:]
        U[i] += M[:n, n:]
    return _frozen(D, U)


# ---- the case tables ----
LENGTHS = {n: tuple(Ts) for n, Ts in P.LENGTHS.items()}
LENGTHS[1] += (4097,)
for _n, _T in ((5, 49153), (6, 49153), (7, 6145), (8, 6145), (12, 513), (16, 513)):
    LENGTHS[_n] += (_T,)
# chains whose LAST segment of an earlier pass is full: every other multi-pass length here is 2^k + 1 or close to it, so its last
# workgroup eliminates nothing and leaves neutral log-pivot entries (mantissa 1, exponent 0) at the end of the entry list -- a
# top-pass fold that stops short of lp_off goes unnoticed (two passes each; T = 128, n = 12: three, both full).  The rows of
# N <= 6 see that break (test_chain_selinv_gpu.py, B2); at N >= 8 a workgroup has more waves than a segment has level-0 nodes and
# the last entry is neutral at any length: those rows only keep the full-segment shape in the table
for _n, _T in ((1, 160), (2, 160), (3, 96), (4, 96), (5, 64), (6, 64), (8, 32), (12, 16), (12, 128), (16, 16)):
    LENGTHS[_n] += (_T,)
WELL_CASES = [(T, n) for n in LENGTHS for T in LENGTHS[n]]
STIFF_CASES = [(65, 2), (65, 3), (97, 4), (49, 6), (40, 8), (65, 11), (65, 12), (65, 16)]     # (T, n); all dense-checkable
# one case per padded N at its deepest plan, on a padded block wherever one size is padded to N (only the generator is needed:
# the scaled results are compared with the unscaled ones)
SCALE_CASES = [(4097, 1), (4097, 2), (2049, 3), (2049, 4), (49153, 5), (6145, 7), (513, 11), (513, 13)]
# one case per padded N on a plan of three passes
NOT_PD_CASES = [(4097, 1), (4097, 2), (2049, 3), (2049, 4), (1537, 5), (385, 7), (130, 11), (130, 13)]


def case_seed(T, n):
    return 9000 * n + T


def state_b(T, n):
    """the chain a well case is measured on"""
    return well(T, n, case_seed(T, n))


def state_a(T, n):
    """another positive definite chain of the shape, factorised first in the same context"""
    return well(T, n, case_seed(T, n) + 500000)


def stiff_state(T, n):
    return stiff(T, n, case_seed(T, n))


@functools.lru_cache(maxsize=None)
def reference(T, n):
    """float64 selinv of state_b(T, n); read-only"""
    SD, SU, hld = selinv(*state_b(T, n))
    _frozen(SD, SU)
    return SD, SU, float(hld)


@functools.lru_cache(maxsize=None)
def stiff_reference(T, n):
    """dict: the longdouble selinv of stiff_state(T, n), the dense condition number, and the float64 recursion's own deviation
    from it -- dev (SD / SU, test_gpu_parity.rel form) and dev_hld (relative)"""
    D, U = stiff_state(T, n)
    SDl, SUl, hl = selinv(D, U, np.longdouble)
    SD, SU, h = selinv(D, U)
    _frozen(SDl, SUl)
    return dict(SD=SDl, SU=SUl, hld=hl, cond=float(np.linalg.cond(P.dense(D, U))), dev=max(rel(SD, SDl), rel(SU, SUl)),
                dev_hld=float(abs(h - hl) / abs(hl)))


@functools.lru_cache(maxsize=None)
def stiff_logdet_yardstick():
    """largest relative deviation of the float64 recursion's half log-det from the longdouble one over the stiff cases"""
    return max(stiff_reference(T, n)["dev_hld"] for T, n in STIFF_CASES)


# ---- a chain that is not positive definite, found out only by the last pass ----
def cr_not_pd_nodes(D, U):
    """The kernels' elimination ORDER without pivoting, in float64: level l eliminates the odd multiples of 2^l, the root last.
    Returns the nodes whose effective block is not positive definite at its elimination (the factorisation's 'bad' pivots: the
    natural pivots of a symmetric block are all positive exactly when it is positive definite)."""
    T = D.shape[0]
    Dw = np.array(D, dtype=np.float64)
    A = {(t, t + 1): np.asarray(U[t], dtype=np.float64) for t in range(T - 1)}
    bad = []

    def check(e):
        if np.linalg.eigvalsh(0.5 * (Dw[e] + Dw[e].T)).min() <= 0.0:
            bad.append(e)

    for l in range(chain_levels(T)):
        h = 1 << l
        for e in range(h, T, 2 * h):
            a, b = e - h, (e + h if e + h < T else None)
            check(e)
            E = np.linalg.inv(Dw[e])
            Ua = A[(a, e)]
            Dw[a] -= Ua @ E @ Ua.T
            if b is not None:
                Ub = A[(e, b)]
                Dw[b] -= Ub.T @ E @ Ub
                A[(a, b)] = -Ua @ E @ Ub
    check(0)
    return bad


@functools.lru_cache(maxsize=None)
def not_pd_state(T, n):
    """(D, U, e, h, c): state_b(T, n) with c I subtracted from D[e].  h = 2^level0 of the top pass is the first node the LAST
    pass eliminates that is no root, e = h + 1 its right neighbour, a level-0 node of the first pass.  Every node eliminated
    before the last pass lies strictly between two last-pass nodes, so what it sees of e is the principal submatrix WITHOUT h.
    With SD_e the marginal of e in the full chain and SD'_e the one in the chain cut off at h (both by the float64 recursion),
    A - c E_e stays positive definite up to c_lo = 1 / lambda_max(SD_e) and the cut-off chain up
    to c_hi = 1 / lambda_max(SD'_e) > c_lo (e loses the neighbour h); c is their mean: e itself and every node of the earlier
    passes keep positive pivots, and the first non-positive one appears in the last pass (test_chain_selinv_host.py replays the
    elimination order and asserts it)."""
    D, U = state_b(T, n)
    h = 1 << chain_passes(T, n)[-1][0]
    assert len(chain_passes(T, n)) >= 3 and h + 1 < T
    e = h + 1
    c_lo = 1.0 / np.linalg.eigvalsh(reference(T, n)[0][e]).max()
    c_hi = 1.0 / np.linalg.eigvalsh(selinv(D[e:], U[e:])[0][0]).max()
    c = 0.5 * (c_lo + c_hi)
    Dn = np.array(D)
    Dn[e] -= c * np.eye(n)
    return _frozen(Dn)[0], U, e, h, (c_lo, c, c_hi)
