"""Float64 reference of the covariance columns (kernels_solve.hpp, solve_sweep_kernel with a node list) and restatement of the
solve sweep's launch plan (posterior_host.inc, sweep_plan with the solve_lds option), numpy only; the case tables of
tests/test_solve_sweep_gpu.py.

The general solve's reference is test_solve_host.cr_solve, the float64 restatement of the kernel's up- and down-sweep on the
R, GA, GB of cr_factor.  columns() is cr_solve on the unit columns of a node list, returned in the layout of gvi_bt_cov_columns,
C[c][t][r][k] = x_(c n + k)[t][r].  tests/test_solve_shapes_host.py proves both at every shape the GPU module uses.

sweep_plan restates the rule by which the library picks the sweep's memory mode and tile length, with the constants of
tests/sample_ref.py (the library shares one plan between the sampler and the solve).  The library reports neither mode nor
tile, so a GPU case can only assert the (mode, tile, last tile) it was written for against this restatement: if the plan's
constants change, the rows below that then sit off their edge fail at the module's import and in the host test instead of
silently testing something else."""
import math

import numpy as np

import sample_ref as sr
from sample_ref import ENUM_N, ENUM_T, GROW_SHRINK_T, MANY_NODES, N_ALL, last_tile  # noqa: F401  (shared with the sampler's module)
from test_solve_host import cr_solve

SMALL_TN = 600                                       # up to here the host proof forms the dense inverse


def sweep_plan(R, T, n, lds_allowed=True):
    """(lds, tile) of the solve sweep for R right-hand sides of a (T, n) chain: posterior_host.inc::sweep_plan.
    lds_allowed: option solve_lds; with it the plan is the sampler's."""
    rowb = 8 * T * n
    lds = bool(lds_allowed) and rowb <= sr.LDS_BYTES
    cap = min(sr.TILE_MAX, sr.LDS_BYTES // rowb) if lds else sr.TILE_MAX
    return lds, max(1, min(cap, (R + sr.SWEEP_GROUPS - 1) // sr.SWEEP_GROUPS))


# ---- case tables: (T, n, count, lds, tile, last) with the default options; count = R right-hand sides or ncols nodes ----
GENERAL = ((7, 4, 513, True, 2, 1), (7, 4, 3585, True, 8, 1), (7, 4, 4096, True, 8, 8),
           (9, 6, 513, True, 2, 1), (9, 6, 3585, True, 8, 1), (5, 13, 513, True, 2, 1), (5, 13, 3585, True, 8, 1),
           (375, 8, 1537, True, 3, 1),                                        # the count asks for 4, 81920 // 24000 allows 3
           (640, 16, 3, True, 1, 1), (641, 16, 3, False, 1, 1),               # the 80 KB boundary
           (2561, 4, 513, False, 2, 1), (1281, 8, 513, False, 2, 1), (641, 16, 513, False, 2, 1),       # output buffer by size
           (1465, 7, 513, False, 2, 1), (789, 13, 513, False, 2, 1), (1281, 8, 1025, False, 3, 2))
COLUMNS = ((7, 4, 129, True, 2, 2), (7, 4, 275, True, 3, 2),                  # 275: tiles straddle two columns
           (7, 4, 897, True, 8, 4), (9, 7, 75, True, 2, 1),                   # odd n, ragged
           (5, 13, 41, True, 2, 1), (5, 13, 276, True, 8, 4),                 # 276: a straddle on the NM = 16 instance
           (375, 8, 193, True, 3, 2),                                         # capped by LDS
           (641, 16, 33, False, 2, 2), (1465, 7, 75, False, 2, 1), (2561, 4, 129, False, 2, 2))          # output buffer by size
# with solve_lds = 0 an LDS row keeps its tile and last tile, except where LDS capped the tile
NO_LDS_GENERAL = {(375, 8, 1537): (4, 1)}
NO_LDS_COLUMNS = {(375, 8, 193): (4, 4)}
STRADDLE = ((7, 4, 275), (5, 13, 276))               # bt_cov_columns against bt_solve_multi on explicit unit columns, bit for bit
NOT_PD_GENERAL = ((7, 4, 513, True, 2, 1), (641, 16, 2, False, 1, 1))
NOT_PD_COLUMNS = ((7, 4, 129, True, 2, 2),)
CONTIGUITY = ((9, 7, 1), (9, 7, 0), (1465, 7, 1))    # (T, n, solve_lds): R = 513 and the (., 7, 75) rows of COLUMNS


def with_modes(table, no_lds):
    """Every row as (T, n, count, solve_lds, lds, tile, last): as it stands, and every LDS row again with solve_lds = 0."""
    rows = [(T, n, c, 1, lds, tile, last) for T, n, c, lds, tile, last in table]
    for T, n, c, lds, tile, last in table:
        if lds:
            t0, l0 = no_lds.get((T, n, c), (tile, last))
            rows.append((T, n, c, 0, False, t0, l0))
    return tuple(rows)


GENERAL_ROWS = with_modes(GENERAL, NO_LDS_GENERAL)
COLUMN_ROWS = with_modes(COLUMNS, NO_LDS_COLUMNS)


def assert_plan(T, n, R, solve_lds, lds, tile, last):
    """R right-hand sides of a (T, n) chain reach the mode, tile length and last tile the case was written for."""
    got = sweep_plan(R, T, n, solve_lds)
    assert got == (lds, tile) and last_tile(R, tile) == last, (T, n, R, solve_lds, got, last_tile(R, tile))


def assert_tables():
    for T, n, R, opt, lds, tile, last in GENERAL_ROWS:
        assert_plan(T, n, R, opt, lds, tile, last)
    for T, n, nc, opt, lds, tile, last in COLUMN_ROWS:
        assert_plan(T, n, nc * n, opt, lds, tile, last)
    for T, n, R, lds, tile, last in NOT_PD_GENERAL:
        assert_plan(T, n, R, 1, lds, tile, last)
    for T, n, nc, lds, tile, last in NOT_PD_COLUMNS:
        assert_plan(T, n, nc * n, 1, lds, tile, last)
    assert len(GENERAL_ROWS) == 16 + 9 and len(COLUMN_ROWS) == 10 + 7


assert_tables()


def node_list(T, ncols):
    """nodes[c] = (3 + s c) % T with s = 5, or the next step coprime to T where 5 is not: neighbours in a tile are different
    nodes; where ncols s > T the list wraps, so it holds duplicates and is not sorted."""
    s = 5
    while math.gcd(s, T) != 1:
        s += 1
    return [(3 + s * c) % T for c in range(ncols)]


def gpu_shapes():
    """Every (T, n) tests/test_solve_sweep_gpu.py solves on, sorted."""
    s = {(T, n) for n in N_ALL for T in GROW_SHRINK_T}
    s |= {(T, n) for n in ENUM_N for T in ENUM_T}
    s |= set(MANY_NODES)
    s |= {c[:2] for c in GENERAL + COLUMNS + NOT_PD_GENERAL + NOT_PD_COLUMNS + CONTIGUITY}
    return sorted(s)


def unit_columns(T, n, nodes):
    """B [len(nodes) n][T][n]: right-hand side c n + k is the unit vector at (nodes[c], k)."""
    B = np.zeros((len(nodes) * n, T, n))
    for c, t in enumerate(nodes):
        for k in range(n):
            B[c * n + k, t, k] = 1.0
    return B


def columns(D, U, nodes, factor=None):
    """C [len(nodes)][T][n][n], C[c][t] = block (t, nodes[c]) of (D, U)^-1: cr_solve on the unit columns of the node list,
    C[c][t][r][k] = x_(c n + k)[t][r].  factor: a cr_factor(D, U) computed before (it is not written to)."""
    T, n = D.shape[0], D.shape[1]
    X = cr_solve(D, U, unit_columns(T, n, nodes), factor)            # [c n + k][t][r]
    return np.ascontiguousarray(X.reshape(len(nodes), n, T, n).transpose(0, 2, 3, 1))
