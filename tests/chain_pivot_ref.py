"""Inputs and float64 references for the tests of the PIVOTED chain solve (test_chain_pivot_host.py, test_chain_pivot_gpu.py);
numpy only, no GPU.

indefinite_chain / zero_diagonal_chain build block-tridiagonal systems that are well conditioned but on which the threshold
partial pivoting of the chain kernels (kernels_chain.hpp eliminate / gj_rowb, kernels_chain_wave.hpp gauss_jordan: rows are
swapped when |natural pivot| * 8 < column maximum) does swap rows.  census restates the kernels' elimination order with that
rule in float64 and records, per node, what was swapped and how close every decision was to the threshold: the host test holds
every input to a margin that rounding in another order of summation cannot cross, so the census describes what the device does.

Nodes: level l eliminates the alive nodes that are odd multiples of 2^l, neighbours e -+ 2^l; node 0 is the root and is given
the level chain_levels(T)."""
import functools

import numpy as np

# ---- chain_plan.hpp::chain_passes, restated: padded block size N -> (cap = longest top pass, m_seg = levels of a segmented pass)
# (test_chain_pivot_host.py compares the two expressions with the header's text)
PADDED = (1, 2, 3, 4, 6, 8, 12, 16)
CAP_EXPR = "n <= 2 ? 128 : (n <= 4 ? 64 : (n <= 6 ? 48 : (n <= 8 ? 24 : 8)))"
MSEG_EXPR = "n <= 6 ? 5 : (n <= 8 ? 4 : 3)"


def padded(n):
    return next(N for N in PADDED if n <= N)


def chain_levels(T):
    L = 0
    while (1 << L) < T:
        L += 1
    return L


def chain_passes(T, n):
    """[(level0, levels, top)] of the chain's plan; the last pass is the top pass (it also eliminates the root)."""
    N = padded(n)
    m_seg = 5 if N <= 6 else (4 if N <= 8 else 3)
    cap = 128 if N <= 2 else (64 if N <= 4 else (48 if N <= 6 else (24 if N <= 8 else 8)))
    alive = lambda l: (T + (1 << l) - 1) >> l
    passes, level0 = [], 0
    while alive(level0) > cap:
        passes.append((level0, m_seg, False))
        level0 += m_seg
    passes.append((level0, chain_levels(T) - level0, True))
    return passes


def pass_of(level, passes):
    """index of the pass that eliminates the nodes of a level"""
    return max(i for i, ps in enumerate(passes) if ps[0] <= level)


def node_level(e, T):
    return chain_levels(T) if e == 0 else (e & -e).bit_length() - 1


# ---- generators ----
def _indefinite(T, n, seed):
    rng = np.random.default_rng(seed)
    D = np.empty((T, n, n))
    for t in range(T):
        S = rng.normal(size=(n, n))
        w, V = np.linalg.eigh(0.5 * (S + S.T))
        D[t] = 2.0 * (V * (np.sign(w) * (1.0 + np.abs(w)))) @ V.T
        D[t] = 0.5 * (D[t] + D[t].T)
    U = 0.3 * rng.normal(size=(max(T - 1, 0), n, n)) / np.sqrt(n)
    rhs = rng.normal(size=(T, n))
    return D, U, rhs


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def indefinite_chain(T, n, seed):
    """D_t = 2 V diag(sign(w) (1 + |w|)) V^T from the eigendecomposition of a random symmetric matrix (symmetric, indefinite,
    condition <= ~8), U_t = 0.3 N(0, 1) / sqrt(n), rhs ~ N(0, 1).  Read-only arrays, computed once."""
    return _frozen(*_indefinite(T, n, seed))


def zero_nodes(T):
    """Nodes the zero-diagonal generator changes: level-0 nodes whose leading diagonal entry becomes exactly 0.0 (node 1; the
    last node when it is odd -- no right neighbour; an odd node near 3T/4 -- with two nodes per wave it sits in the other half
    of a wave than node 1), and higher-level nodes whose EFFECTIVE leading entry becomes 1e-3 of its column maximum, in the order
    they are made (node 2: both neighbours; the largest power of two below T; node 0, the root)."""
    exact = {1}
    if (T - 1) % 2 == 1:
        exact.add(T - 1)
    if T >= 8:
        exact.add((3 * T // 4) | 1)
    high = [e for e in dict.fromkeys((2, 1 << (chain_levels(T) - 1))) if 2 <= e < T] + [0]
    return sorted(exact), high


@functools.lru_cache(maxsize=None)
def zero_diagonal_chain(T, n, seed):
    """indefinite_chain with zero natural pivots at step 0 (n >= 2): an unpivoted elimination divides by zero in the level-0
    nodes of zero_nodes(T) and by (nearly) zero in the higher-level ones.  A higher-level node's Schur updates do not depend on
    its own D: they are taken from the census, D[e][0, 0] := -update[0, 0] makes the effective entry zero to rounding, and it is
    then put at 1e-3 of the effective column maximum so that the decision is no tie."""
    assert n >= 2 and T >= 2
    D, U, rhs = _indefinite(T, n, seed)
    exact, high = zero_nodes(T)
    for e in exact:
        D[e, 0, 0] = 0.0
        a = np.copysign(max(abs(D[e, 1, 0]), 1.5), D[e, 1, 0])       # [[0, a], [a, d]] in the leading corner, |a| not small
        D[e, 1, 0] = D[e, 0, 1] = a
    for e in high:                                                   # (the root last: its updates depend on every other node)
        eff = census(D, U, rhs)[1][e]["block"]
        D[e, 0, 0] += -eff[0, 0] + 1e-3 * np.abs(eff[1:, 0]).max()
    return _frozen(D, U, rhs)


# ---- the kernels' elimination in float64 ----
def _gauss_jordan(M, n):
    """[D | ...] -> [I | D^-1 ...] in place with the kernels' threshold rule; returns (swaps [(p, rs)], closest margin, a pivot
    was not positive)"""
    swaps, margin, neg = [], np.inf, False
    for p in range(n):
        col = np.abs(M[p:n, p])
        k = int(np.argmax(col))                                      # the first maximum, as the kernels' strict '>' search
        with np.errstate(divide="ignore"):
            margin = min(margin, abs(np.log(8.0 * col[0] / col[k])))
        if col[0] * 8.0 < col[k]:
            M[[p, p + k]] = M[[p + k, p]]
            swaps.append((p, p + k))
        neg |= not M[p, p] > 0.0
        M[p] /= M[p, p]
        for r in range(n):
            if r != p:
                M[r] -= M[r, p] * M[p]
    return swaps, margin, neg


def census(D, U, rhs):
    """x and, per node, dict(level, swaps [(p, rs)], cond and block (the matrix that was inverted), margin
    (min |log(8 |col_p| / best)| over its pivot decisions), neg (a pivot was not positive))."""
    T, n = rhs.shape
    Dw, y = np.array(D, dtype=np.float64), np.array(rhs, dtype=np.float64)
    A = {(t, t + 1): np.asarray(U[t], dtype=np.float64) for t in range(T - 1)}
    L = chain_levels(T)
    G, info = {}, [None] * T

    def eliminate(e, level, a, b):
        cols = [Dw[e]] + ([A[(a, e)].T] if a is not None else []) + ([A[(e, b)]] if b is not None else []) + [y[e][:, None]]
        M = np.concatenate(cols, axis=1)
        swaps, margin, neg = _gauss_jordan(M, n)
        info[e] = dict(level=level, swaps=swaps, cond=np.linalg.cond(Dw[e]), margin=margin, neg=neg, block=Dw[e].copy())
        GA = M[:, n:2 * n] if a is not None else None
        GB = M[:, M.shape[1] - 1 - n:M.shape[1] - 1] if b is not None else None
        return GA, GB, M[:, -1].copy()

    for l in range(L):
        h = 1 << l
        for e in range(h, T, 2 * h):
            a, b = e - h, (e + h if e + h < T else None)
            GA, GB, v = eliminate(e, l, a, b)
            Ua = A[(a, e)]
            Dw[a] -= Ua @ GA
            y[a] -= Ua @ v
            if b is not None:
                Ub = A[(e, b)]
                Dw[b] -= Ub.T @ GB
                y[b] -= Ub.T @ v
                A[(a, b)] = -Ua @ GB
            G[e] = (a, b, GA, GB, v)
    x = np.empty((T, n))
    x[0] = eliminate(0, L, None, None)[2]
    for l in range(L - 1, -1, -1):
        h = 1 << l
        for e in range(h, T, 2 * h):
            a, b, GA, GB, v = G[e]
            x[e] = v - GA @ x[a] - (GB @ x[b] if b is not None else 0.0)
    return x, info


def dense(D, U):
    T, n = D.shape[:2]
    M = np.zeros((T * n, T * n))
    for t in range(T):
        M[t * n:(t + 1) * n, t * n:(t + 1) * n] = D[t]
    for t in range(T - 1):
        M[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = U[t]
        M[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = U[t].T
    return M


def block_residual(D, U, x, rhs):
    """max |A x - rhs| without forming A"""
    Ax = np.einsum("tij,tj->ti", D, x)
    Ax[:-1] += np.einsum("tij,tj->ti", U, x[1:])
    Ax[1:] += np.einsum("tji,tj->ti", U, x[:-1])
    return np.abs(Ax - rhs).max()


# ---- the cases of test_chain_pivot_gpu.py ----
LENGTHS = {1: (3, 129), 2: (2, 3, 9, 65, 66, 128, 129, 4097), 3: (2, 3, 9, 64, 65, 97, 2049), 4: (2, 3, 9, 64, 65, 97, 2049),
           5: (3, 35, 48, 49, 70, 1537), 6: (3, 35, 48, 49, 70, 1537), 7: (2, 3, 24, 25, 40, 385), 8: (2, 3, 24, 25, 40, 385),
           9: (2, 3, 8, 9, 17, 65, 130), 11: (2, 3, 8, 9, 17, 65, 130), 12: (2, 3, 8, 9, 17, 65, 130),
           13: (3, 8, 9, 65, 130), 16: (3, 8, 9, 65, 130)}


def _zero_lengths(n):
    two_pass = next(T for T in LENGTHS[n] if len(chain_passes(T, n)) == 2)
    return LENGTHS[n][:2] + (two_pass,)


# (T, n, generator): every shape with the random generator; n >= 2: the zero-diagonal one at the two shortest chains and the
# first with two passes
CASES = [(T, n, "rand") for n in LENGTHS for T in LENGTHS[n]] + [(T, n, "zero") for n in LENGTHS if n >= 2 for T in _zero_lengths(n)]

# Seeds: the first of 0, 1, 2, ... for which the case meets the conditions of test_chain_pivot_host.py (margins, conditioning,
# swaps on the levels and in the passes it asks for: find_seed below); cases not listed use seed 0.  T = 2049, n = 3: the first
# that also has a node with TWO swaps, which a well-conditioned 3 x 3 block allows about once in 50000 nodes.
SEEDS = {(3, 1, "rand"): 5, (129, 1, "rand"): 10, (2, 2, "rand"): 362, (3, 2, "rand"): 289, (9, 2, "rand"): 3,
         (65, 2, "rand"): 3, (66, 2, "rand"): 3, (128, 2, "rand"): 1, (4097, 2, "rand"): 3, (2, 3, "rand"): 130,
         (3, 3, "rand"): 75, (9, 3, "rand"): 2, (65, 3, "rand"): 4, (97, 3, "rand"): 3, (2049, 3, "rand"): 29,
         (2, 4, "rand"): 13, (3, 4, "rand"): 13, (9, 4, "rand"): 1, (2049, 4, "rand"): 2, (49, 5, "rand"): 2,
         (70, 5, "rand"): 2, (1537, 5, "rand"): 2, (3, 6, "rand"): 7, (49, 6, "rand"): 2, (70, 6, "rand"): 2,
         (1537, 6, "rand"): 2, (2, 7, "rand"): 5, (3, 7, "rand"): 1, (40, 7, "rand"): 1, (385, 7, "rand"): 5,
         (2, 9, "rand"): 3, (3, 9, "rand"): 1, (8, 9, "rand"): 1, (9, 9, "rand"): 1, (2, 11, "rand"): 2}


def case_seed(T, n, gen):
    return SEEDS.get((T, n, gen), 0)


@functools.lru_cache(maxsize=None)
def case(T, n, gen):
    """(D, U, rhs, x of the census, per-node records) of a case; read-only, computed once"""
    D, U, rhs = (indefinite_chain if gen == "rand" else zero_diagonal_chain)(T, n, case_seed(T, n, gen))
    x, info = census(D, U, rhs)
    x.setflags(write=False)
    return D, U, rhs, x, info


def case_problems(T, n, info):
    """What keeps a case from being a test of the swap code (empty: nothing).  Conditions on one case."""
    out = []
    if min(r["margin"] for r in info) < 1e-6:
        out.append("a pivot decision within 1e-6 of the threshold")
    if max(r["cond"] for r in info) > 1e2:
        out.append("an inverted block with cond > 1e2")
    passes = chain_passes(T, n)
    if n == 1:
        if {r["level"] for r in info if r["neg"]} != set(range(chain_levels(T) + 1)):
            out.append("a level without a negative pivot")
        return out
    sw = [r for r in info if r["swaps"]]
    if not any(r["level"] == 0 for r in sw):
        out.append("no swap at level 0")
    if not any(r["level"] >= 1 for r in sw):
        out.append("no swap at a level >= 1")
    if {pass_of(r["level"], passes) for r in sw} != set(range(len(passes))):
        out.append("a pass without a swap")
    return out


def find_seed(T, n, gen, limit=20000):
    """first seed whose case has no problems (how SEEDS was made)"""
    for seed in range(limit):
        D, U, rhs = (_indefinite if gen == "rand" else zero_diagonal_chain.__wrapped__)(T, n, seed)
        if not case_problems(T, n, census(D, U, rhs)[1]):
            return seed
    raise ValueError((T, n, gen))
