"""Option "chol_rowb": the register Cholesky of the per-pass products (kernels_prep.hpp, prep_chol_body) with DPP row-broadcast
multipliers against its v_readlane form, through the prep launch of the three-launch route (option "fused" 0), which holds
both forms as instances of its own.  Same products with the same signs: S = L, S^-T, Sigma^-1, H = A L and u0 must agree bit
for bit; where a pivot is not positive the NaNs must sit in exactly the same entries and every other entry must still agree
bit for bit.

Shapes: one binary prior set of d = 2 n = 2, 4, 6, 8, 12 with K = 1, 3, 5 factors on a chain of K + 1 states.  The state has
a block-diagonal precision (no coupling), so the marginal of factor k is blkdiag(Sigma_k, Sigma_k+1) with Sigma_t the inverse
of the state's precision block, which the test chooses: Sigma_t = L_t S_t L_t^T, L_t lower triangular with a positive diagonal
and S_t = I, or with one -1 to put a negative pivot at step 0 (first), d / 2 (middle) or d - 1 (last) of factor K // 2.  The
test checks on the v_readlane result that the NaNs are where such a pivot puts them (entries (r, c) of L with j <= c <= r), so
the inputs do what they claim."""
import numpy as np
import pytest

from gaussianvi_amd import api

pytestmark = pytest.mark.gpu
P_DEG = 3                                     # smallest degree that takes the Cholesky route
NEG = ("none", "first", "middle", "last")


def _state(n, K, neg, rng):
    """(mu, D, U) of the chain, the factor with the negative pivot and its step (None without one)"""
    T, d = K + 1, 2 * n
    kf, step = K // 2, {"none": None, "first": 0, "middle": d // 2, "last": d - 1}[neg]
    D = np.zeros((T, n, n))
    for t in range(T):
        L = np.tril(0.3 * rng.normal(size=(n, n)), -1) + np.diag(rng.uniform(0.8, 1.6, n))
        S = np.ones(n)
        if step is not None and t == kf + (step >= n):
            S[step % n] = -1.0
        Sig = (L * S) @ L.T
        Dt = np.linalg.inv(Sig)
        D[t] = 0.5 * (Dt + Dt.T)
    return rng.normal(size=(T, n)), D, np.zeros((T - 1, n, n)), kf, step


def _bits_equal_outside_nan(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("d", [2, 4, 6, 8, 12])
def test_row_broadcast_cholesky_matches_the_readlane_form_bit_for_bit(d, K):
    n = d // 2
    rng = np.random.default_rng(100 * d + K)
    G = rng.normal(size=(K, n, n))
    Phi = np.eye(n)[None] + 0.05 * rng.normal(size=(K, n, n))
    Q = G @ G.transpose(0, 2, 1) / n + 2.0 * np.eye(n)
    ctx = api.Context(0)
    try:
        ctx.set_option("fused", 0)
        ctx.chain_set(K + 1, n)
        sid = ctx.factors_add(d, P_DEG, np.arange(K, dtype=np.int32), api.PSI_QUAD_PRIOR,
                              np.concatenate([Phi.reshape(K, -1), Q.reshape(K, -1)], 1), rng.uniform(0.5, 2.0, K))
        for neg in NEG:
            mu, D, U, kf, step = _state(n, K, neg, rng)
            got = {}
            for rowb in (1, 0):
                ctx.set_option("chol_rowb", rowb)               # (drops the products: the next pass runs its prep)
                ctx.ngd_init(mu, D, U)
                ctx.ngd_gradients()
                got[rowb] = ctx.debug_products(sid, K, d, n)
            S0 = got[0]["S"]
            want_nan = np.zeros((K, d, d), dtype=bool)
            if step is not None:
                r, c = np.indices((d, d))
                want_nan[kf] = (c >= step) & (r >= c)
                # (a neighbour of factor kf shares the state with the -1: its own NaNs are not pinned here, only compared)
                assert np.array_equal(np.isnan(S0[kf]), want_nan[kf]), (neg, np.isnan(S0[kf]).astype(int))
            else:
                assert not np.isnan(S0).any()
                Sig = S0 @ S0.transpose(0, 2, 1)                 # the factor of the marginal it was given
                for k in range(K):
                    ref = np.zeros((d, d))
                    ref[:n, :n], ref[n:, n:] = np.linalg.inv(D[k]), np.linalg.inv(D[k + 1])
                    assert np.abs(Sig[k] - ref).max() <= 1e-10 * np.abs(ref).max(), (k, np.abs(Sig[k] - ref).max())
            for name in ("S", "Sinv", "Lam", "H", "u0"):
                a, b = got[1][name], got[0][name]
                nn = int(np.isnan(b).sum())
                same = _bits_equal_outside_nan(a, b)
                print(f"d {d} K {K} {neg}: {name} NaN entries {nn} of {b.size}, row-broadcast == v_readlane outside them: {same}")
                assert same, (neg, name)
    finally:
        ctx.close()
