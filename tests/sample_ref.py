"""Float64 restatement of the sampler's sweep (kernels_sample.hpp, sample_sweep_kernel) and of its launch plan
(posterior_host.inc, sweep_plan), numpy only.

A sample is a function of (D, U, eps) alone: the pivots are Cholesky factors with positive diagonal and the elimination order
is fixed, so cr_sample is a per-entry reference of gvi_bt_sample / gvi_ngd_sample, not just of its covariance.  It stands on
test_solve_host.cr_factor, which returns the R, GA, GB that sample_factor_kernel writes; tests/test_sample_host.py proves it
against the dense inverse (small shapes) and through y^T Lambda y = |eps|^2 (large shapes).

sweep_plan restates the rule by which the library picks the sweep's memory mode and tile length.  The library has no call that
reports either, so a GPU case can only assert the mode and tile it was written for against this restatement: if the constants
of the library's plan change, the restatement has to change with them, and the cases that then sit off their edge fail here
instead of silently testing something else.  It is the only check of that kind."""
import numpy as np

from test_solve_host import cr_factor, levels

LDS_BYTES = 80 * 1024      # SAMPLE_LDS_BYTES
TILE_MAX = 8               # SAMPLE_TILE_MAX
SWEEP_GROUPS = 512         # workgroups wanted before tiles grow (sweep_plan: (count + 511) / 512)


# ---- the shapes of tests/test_sample_sweep_gpu.py; tests/test_sample_host.py proves the reference at every one of them ----
# Sweep cases are (T, n, S, lds, tile, last): the mode, tile length and size of the last tile the case is written for.
N_ALL = tuple(range(1, 17))
GROW_SHRINK_T = (1, 2, 3, 6, 17, 4)                 # one context per n: the workspaces are carved again, larger and smaller
ENUM_T = tuple(range(1, 21)) + tuple(range(31, 35)) + tuple(range(63, 67)) + tuple(range(127, 131))
ENUM_N = (3, 16)
MANY_NODES = ((2051, 1), (700, 3), (131, 16))       # level 0 eliminates more nodes than the block has lane groups
LDS_TILES = ((7, 4, 513, True, 2, 1), (7, 4, 1100, True, 3, 2), (7, 4, 3585, True, 8, 1), (7, 4, 4096, True, 8, 8),
             (9, 6, 513, True, 2, 1), (9, 6, 3585, True, 8, 1), (5, 13, 513, True, 2, 1), (5, 13, 3585, True, 8, 1))
LDS_CAPPED = ((375, 8, 1537, True, 3, 1),)          # the count asks for 4, 81920 // 24000 allows 3
BOUNDARY = ((640, 16, 3, True, 1, 1), (641, 16, 3, False, 1, 1))
BUFFER_TILES = ((2561, 4, 513, False, 2, 1), (1281, 8, 513, False, 2, 1), (641, 16, 513, False, 2, 1),
                (1465, 7, 513, False, 2, 1), (789, 13, 513, False, 2, 1), (1281, 8, 1025, False, 3, 2))
GENERATED = ((9, 7, 513, True, 2, 1), (9, 7, 1100, True, 3, 2), (1465, 7, 513, False, 2, 1), (1465, 7, 1025, False, 3, 2))
NOT_PD = ((7, 4, 513, True, 2, 1), (641, 16, 2, False, 1, 1))
LOGPDF_T, LOGPDF_S = (1, 2, 3, 300), (1, 7)
SMALL_TN = 600                                       # up to here the host proof forms the dense inverse


def gpu_shapes():
    """Every (T, n) the GPU module samples or evaluates on, sorted."""
    s = {(T, n) for n in N_ALL for T in GROW_SHRINK_T + LOGPDF_T}
    s |= {(T, n) for n in ENUM_N for T in ENUM_T}
    s |= set(MANY_NODES)
    s |= {c[:2] for c in LDS_TILES + LDS_CAPPED + BOUNDARY + BUFFER_TILES + GENERATED + NOT_PD}
    return sorted(s)


def cr_sample(D, U, eps, factor=None):
    """y [S][T][n] of the back-sweep on eps [S][T][n]: y_root = R_0 eps_0, then, levels top-down,
    y_e = R_e eps_e - GA_e y_a - GB_e y_b with a = e - 2^l, b = e + 2^l (b absent when e + 2^l >= T).  x = mu + y.
    factor: a cr_factor(D, U) computed before (it is not written to)."""
    T = D.shape[0]
    R, GA, GB = cr_factor(D, U) if factor is None else factor
    Y = np.array(eps, dtype=float)
    assert Y.ndim == 3 and Y.shape[1:] == D.shape[:2]
    Y[:, 0] = Y[:, 0] @ R[0].T
    for l in range(levels(T) - 1, -1, -1):
        step = 1 << l
        for e in range(step, T, 2 * step):
            v = Y[:, e] @ R[e].T - Y[:, e - step] @ GA[e].T
            if e + step < T:
                v -= Y[:, e + step] @ GB[e].T
            Y[:, e] = v
    return Y


def half_logdet(D, U, factor=None):
    """1/2 log det of (D, U) from the Cholesky factors of the pivots: R_e = L_e^-T, so log diag L_e = -log diag R_e."""
    R = (cr_factor(D, U) if factor is None else factor)[0]
    return -float(np.log(np.einsum("tii->ti", R)).sum())


def block_matvec(D, U, X):
    """Lambda X for X [S][T][n], block by block: no dense matrix."""
    Y = np.einsum("tij,stj->sti", D, X)
    if D.shape[0] > 1:
        Y[:, :-1] += np.einsum("tij,stj->sti", U, X[:, 1:])
        Y[:, 1:] += np.einsum("tji,stj->sti", U, X[:, :-1])
    return Y


def sweep_plan(S, T, n):
    """(lds, tile) of the sampler's sweep for S samples of a (T, n) chain: posterior_host.inc::sweep_plan with LDS allowed.
    lds: the tile's y lives in LDS (else in the caller's output buffer); tile: samples per workgroup."""
    rowb = 8 * T * n
    lds = rowb <= LDS_BYTES
    cap = min(TILE_MAX, LDS_BYTES // rowb) if lds else TILE_MAX
    return lds, max(1, min(cap, (S + SWEEP_GROUPS - 1) // SWEEP_GROUPS))


def last_tile(S, tile):
    """Samples in the last workgroup's tile."""
    return S - (S - 1) // tile * tile
