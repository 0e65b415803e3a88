"""CPU proof of the references tests/test_solve_sweep_gpu.py compares the device with -- test_solve_host.cr_solve and
solve_ref.columns -- at every (T, n) that module solves on, with its generator random_chain(T, n, 300 + T n), and of the
restated launch plan (solve_ref.sweep_plan) on every row of its case tables.

T n <= 600: cr_solve against numpy.linalg.solve and, on the unit columns, against the dense inverse; columns() of every node
against the dense inverse in the C[c][t][r][k] layout, and of a list with duplicates in descending order.
Above: the forward error |X - X_true| / |X_true| of cr_solve on B = Lambda X_true (the true solution is known, no dense
matrix), and for columns() the layout, entry by entry against cr_solve on single unit vectors, and Lambda C = the unit columns.
Bound 1e-13 everywhere, three orders inside the 1e-10 of the GPU module; cond <= 1e2 asserted wherever a dense matrix is formed.

Worst values measured (printed per shape by `pytest -s`): over the 148 shapes with T n <= 600, dense solve 9.0e-16, dense
inverse 9.7e-16, columns 9.7e-16, cond <= 11.9; over the 18 larger shapes, forward error 8.0e-16, unit-column residual 8.9e-16
(absolute; the entries of the columns are O(1))."""
import numpy as np
import pytest

import sample_ref as sr
import solve_ref as sv
from test_solve_host import SHAPES, cr_factor, cr_solve, dense, random_chain

_SHAPES = sorted(set(sv.gpu_shapes()) | set(SHAPES))
SMALL = [s for s in _SHAPES if s[0] * s[1] <= sv.SMALL_TN]
LARGE = [s for s in _SHAPES if s[0] * s[1] > sv.SMALL_TN]
REF_TOL = 1e-13
COND_MAX = 1e2


def rel(X, ref):
    return np.abs(X - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("T,n", SMALL)
def test_references_against_the_dense_inverse(T, n):
    D, U, _ = random_chain(T, n, 300 + T * n)
    fac = cr_factor(D, U)
    A = dense(D, U)
    w = np.linalg.eigvalsh(A)
    assert w[0] > 0 and w[-1] / w[0] <= COND_MAX
    N = T * n
    B = np.random.default_rng(T * n).standard_normal((5, T, n))
    e_solve = rel(cr_solve(D, U, B, fac), np.linalg.solve(A, B.reshape(5, -1).T).T.reshape(5, T, n))
    Sig = np.linalg.inv(A)
    e_inv = rel(cr_solve(D, U, np.eye(N).reshape(N, T, n), fac).reshape(N, N), Sig)
    ref = Sig.reshape(T, n, T, n).transpose(2, 0, 1, 3)                 # [c][t][r][k] = Sig[t n + r, c n + k]
    Cc = sv.columns(D, U, list(range(T)), fac)
    e_cols = rel(Cc, ref)
    print(f"    REF small T {T} n {n} cond {w[-1] / w[0]:.1f} solve {e_solve:.2e} inverse {e_inv:.2e} columns {e_cols:.2e}")
    assert max(e_solve, e_inv, e_cols) <= REF_TOL
    pick = [T - 1, T // 2, T // 2, 0]                                    # duplicates, descending
    Cp = sv.columns(D, U, pick)                                          # and the factorisation computed inside
    assert Cp.shape == (4, T, n, n)
    for c, t in enumerate(pick):
        assert rel(Cp[c], Cc[t]) <= REF_TOL, (c, t)


@pytest.mark.parametrize("T,n", LARGE)
def test_references_forward_error(T, n):
    D, U, _ = random_chain(T, n, 300 + T * n)
    fac = cr_factor(D, U)
    Xt = np.random.default_rng(T + n).standard_normal((3, T, n))
    e_fwd = rel(cr_solve(D, U, sr.block_matvec(D, U, Xt), fac), Xt)
    nodes = [T - 1, 0, T // 2, 1]
    Cc = sv.columns(D, U, nodes, fac)
    assert Cc.shape == (4, T, n, n)
    for c, t in enumerate(nodes):                                        # the layout, entry by entry
        for k in (0, n - 1):
            b = np.zeros((1, T, n))
            b[0, t, k] = 1.0
            assert rel(Cc[c, :, :, k], cr_solve(D, U, b, fac)[0]) <= REF_TOL, (c, k)     # not bit for bit: BLAS blocks by batch
    Xc = Cc.transpose(0, 3, 1, 2).reshape(4 * n, T, n)                   # back to [c n + k][t][r]
    e_res = np.abs(sr.block_matvec(D, U, Xc) - sv.unit_columns(T, n, nodes)).max()
    print(f"    REF large T {T} n {n} forward {e_fwd:.2e} unit-column residual {e_res:.2e}")
    assert max(e_fwd, e_res) <= REF_TOL


def test_restated_plan():
    """Every row of the case tables, the plan's own edges, and the sampler's plan where LDS is allowed."""
    sv.assert_tables()
    rows = {r[:4] for r in sv.GENERAL_ROWS}
    for T, n, R in ((7, 4, 513), (7, 4, 3585), (7, 4, 4096), (9, 6, 513), (9, 6, 3585), (5, 13, 513), (5, 13, 3585), (375, 8, 1537),
                    (640, 16, 3)):
        assert (T, n, R, 1) in rows and (T, n, R, 0) in rows
    for T, n, R in ((641, 16, 3), (2561, 4, 513), (1281, 8, 513), (641, 16, 513), (1465, 7, 513), (789, 13, 513), (1281, 8, 1025)):
        assert (T, n, R, 1) in rows and (T, n, R, 0) not in rows
    assert (375, 8, 1537, 0, False, 4, 1) in sv.GENERAL_ROWS and (375, 8, 193, 0, False, 4, 4) in sv.COLUMN_ROWS
    assert (7, 4, 275, 0, False, 3, 2) in sv.COLUMN_ROWS and (5, 13, 276, 0, False, 8, 4) in sv.COLUMN_ROWS
    for T, n in _SHAPES:
        for R in (1, 2, 3, 512, 513, 1024, 1025, 1537, 3585, 4096, 4097, 10 ** 6):
            assert sv.sweep_plan(R, T, n, True) == sr.sweep_plan(R, T, n)
            lds, tile = sv.sweep_plan(R, T, n, False)
            assert not lds and tile == min(8, (R + 511) // 512)
    assert sv.sweep_plan(3, 640, 16) == (True, 1) and sv.sweep_plan(3, 641, 16) == (False, 1)
    assert sv.sweep_plan(10 ** 6, 640, 16, False) == (False, 8)
    assert [sv.last_tile(R, t) for R, t in ((1, 1), (513, 2), (516, 2), (1100, 3), (3588, 8), (4096, 8))] == [1, 1, 2, 2, 4, 8]


def test_node_lists():
    """The node list of the column cases: neighbours are different nodes; where it wraps it has duplicates and is unsorted."""
    for T, n, nc, *_ in sv.COLUMNS:
        nodes = sv.node_list(T, nc)
        assert len(nodes) == nc and min(nodes) >= 0 and max(nodes) < T
        assert all(a != b for a, b in zip(nodes, nodes[1:]))
        if nc > T:
            assert len(set(nodes)) == T and nodes != sorted(nodes)
