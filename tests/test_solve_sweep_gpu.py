"""The multi-right-hand-side sweep (kernels_solve.hpp: solve_sweep_kernel<NM, LDSY>) per entry, at every state size, node
enumeration, tile length and memory mode, through gvi_bt_solve_multi, gvi_bt_cov_columns, gvi_ngd_cov_columns(_dev) (-m gpu).

Reference: test_solve_host.cr_solve, the float64 restatement of the up- and down-sweep, and solve_ref.columns, the same on the
unit columns of a node list in the C[c][t][r][k] layout; tests/test_solve_shapes_host.py proves both at every shape used here.
Bound: max |X - ref| <= 1e-10 max |ref| per case, the bound of test_solve_gpu and test_sample_sweep_gpu.  Every case first
asserts the mode (vectors in LDS / in the output buffer), the tile length and the size of the last tile it was written for
against solve_ref.sweep_plan -- the library reports neither, so the restated plan is the only check -- then prints
`ROW <case> T n count NM mode tile last err` (count = right-hand sides, or nodes for a `cols` case).
The rows measured on the MI355X are in profiles/solve_sweep_tests.txt.

test_every_state_size      n = 1 .. 16, one context per n, chain_set over T = 1, 2, 3, 6, 17, 4 (smp_ws / smp_io carved again,
                           larger and smaller), R = 3 and the columns of [T-1, 0, T//2], solve_lds 1 and 0: idle tail lanes when
                           64 % n != 0, both sides of 4|5 and 8|9, T = 1 with U = NULL at the C ABI.
test_every_node_enumeration  T = 1 .. 20, 31 .. 34, 63 .. 66, 127 .. 130 at n = 3 and 16, R = 2 and the columns of [0, T-1],
                           both modes: every last-survivor case of the up-sweep (a right neighbour missing on some levels only).
test_more_nodes_than_lane_groups  (2051, 1), (700, 3), (131, 16), R = 3 and one column: level 0 has more survivors and more
                           eliminated nodes than the block has lane groups (q += NG) on NM = 4 (G = 64, 21) and n = 16 (G = 4).
test_general_tiles         solve_ref.GENERAL: LDS (7, 4) at R = 513 / 3585 / 4096 (tile 2 / 8 / 8, last 1 / 1 / 8), (9, 6) and
                           (5, 13) at R = 513 / 3585; capped by LDS: (375, 8), R = 1537 (tile 3, last 1; with solve_lds 0 tile 4);
                           the 80 KB boundary (640, 16) / (641, 16); output buffer by size with tile 2, last 1 at (2561, 4),
                           (1281, 8), (641, 16), (1465, 7), (789, 13), and tile 3, last 2 at (1281, 8), R = 1025.  Every LDS row
                           again with solve_lds 0.
test_column_tiles          solve_ref.COLUMNS with nodes[c] = (3 + 5 c) % T (step coprime to T): (7, 4) at 129 / 275 / 897 nodes
                           (tile 2 / 3 / 8, last 2 / 2 / 4; at 275 a tile's right-hand sides belong to two nodes), (9, 7, 75)
                           odd n with a ragged last tile through the LDS write-out, (5, 13) at 41 / 276 (tile 2 / 8; a straddle
                           on NM = 16), (375, 8, 193) capped by LDS, output buffer by size at (641, 16, 33), (1465, 7, 75),
                           (2561, 4, 129).  Every LDS row again with solve_lds 0.  At the two straddle rows bt_cov_columns equals
                           bt_solve_multi on the explicit unit columns, transposed, bit for bit, in both modes.
test_contiguity_at_a_ragged_tile_edge  (9, 7) in both modes and (1465, 7): X[R-3:] and X[1:3] of an R = 513 call equal short
                           calls, columns 74 and 1 of the 75-node call equal one-node calls, bit for bit.
test_not_positive_definite one block of D = -I: every entry NaN at (7, 4, R = 513), the columns of (7, 4, 129 nodes), both modes,
                           and (641, 16, R = 2); the next call in the context with the good chain is within the bound.
test_callers_device_buffer ngd_cov_columns_dev on the resident c2 chain after two steps, 257 nodes (R = 514, tile 2), into a
                           torch buffer with 1024 sentinel doubles behind it: equal to ngd_cov_columns and to
                           bt_cov_columns(state), tail untouched, bit for bit.

Measured on the MI355X: all 70 tests pass on the unmodified library (6 s beside test_solve_gpu), so no source file changes.
Worst error per instance and mode over the 705 rows (general right-hand sides / columns):
    NM 4    LDS 7.8e-16 / 6.0e-16    output buffer 7.8e-16 / 6.0e-16
    NM 8    LDS 8.3e-16 / 7.7e-16    output buffer 1.0e-15 / 9.2e-16
    NM 16   LDS 1.4e-15 / 8.4e-16    output buffer 1.4e-15 / 8.4e-16

Sensitivity: four arithmetic-only edits to a scratch copy of kernels_solve.hpp (no address, loop bound, predicate, barrier or
wait count touched), each run once on this module and on test_solve_gpu (47 tests without the shim test, which links the
in-tree library):
  + for - on the GB term of the up-sweep   every per-entry test fails (69: every_state_size 16, every_node_enumeration 2,
                                           more_nodes 3, general_tiles 25, column_tiles 17, contiguity 3, not_positive_definite
                                           3); test_solve_gpu: 31 (dense_parity and columns at T >= 3, 14 each, forward_error 2,
                                           tiles)
  Ac for Bc in the up-sweep                the same 69 and the same 31
  Ar for Br in the down-sweep              the same 69 and the same 31
  Rc / Rr swapped in the down-sweep        68: all but n = 1 (every_state_size[1], more_nodes[2051-1]), where R is a scalar;
                                           test_solve_gpu: 39 (dense_parity and columns at every shape but (1, 1), 18 each)
No edit passes the per-entry tests of either module, so no case was added for one.  test_callers_device_buffer compares the
library with itself and passes under every edit, as it must.

What this cannot see: the results are right with the vmcnt drains of the output-buffer mode in place; that does not show the
drains are necessary (a run without them may pass by timing), and they are not to be removed to find out.  A mix-up of two
right-hand sides inside a tile would be seen (each has its own reference), but no such edit was tried: it would touch an
address.  Where 5 ncols < T (the three by-size column rows) the node list neither wraps nor repeats; duplicates and descending
order are on the LDS-sized rows, in both modes."""
import ctypes as C
import functools

import numpy as np
import pytest

import solve_ref as sv
from gaussianvi_amd import api, synthetic as syn
from test_solve_host import cr_factor, cr_solve, random_chain

pytestmark = pytest.mark.gpu
TOL = 1e-10
SWEEP_WAVES = 8                      # SOLVE_SWEEP_THREADS / 64, each wave with 64 // n lane groups


@functools.lru_cache(maxsize=None)
def problem(T, n):
    """(D, U, cr_factor(D, U)) of a shape, the chain tests/test_solve_shapes_host.py proves the references on: computed once,
    never written to.  U is None on a single-state chain."""
    D, U, _ = random_chain(T, n, 300 + T * n)
    fac = cr_factor(D, U)
    for a in (D, U) + fac:
        a.setflags(write=False)
    return D, (U if T > 1 else None), fac


def rhs(T, n, R):
    return np.random.default_rng(1000 * R + T * n).standard_normal((R, T, n))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def solve(ctx, D, U, B):
    """ctx.bt_solve_multi; a single-state chain goes to the C ABI with U = NULL."""
    if U is not None:
        return ctx.bt_solve_multi(D, U, B)
    X = np.empty(B.shape)
    ctx._ck(ctx.lib.gvi_bt_solve_multi(ctx.h, _p(D), None, B.shape[0], _p(B), _p(X)))
    return X


def cov_columns(ctx, D, U, nodes):
    if U is not None:
        return ctx.bt_cov_columns(D, U, nodes)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    Cc = np.empty((nd.size, ctx.T, ctx.n, ctx.n))
    ctx._ck(ctx.lib.gvi_bt_cov_columns(ctx.h, _p(D), None, nd.size, _p(nd), _p(Cc)))
    return Cc


def row(label, T, n, count, plan, err):
    print(f"    ROW {label} T {T} n {n} count {count} NM {4 if n <= 4 else 8 if n <= 8 else 16} mode {'lds' if plan[0] else 'buffer'} "
          f"tile {plan[1]} last {plan[2]} err {err:.2e}")


def check_solve(label, ctx, T, n, R, opt, plan, B=None):
    """One bt_solve_multi call under solve_lds = opt against cr_solve, per entry; prints the row, returns X."""
    sv.assert_plan(T, n, R, opt, *plan)
    D, U, fac = problem(T, n)
    B = rhs(T, n, R) if B is None else B
    ctx.set_option("solve_lds", opt)
    X = solve(ctx, D, U, B)
    ref = cr_solve(D, U if U is not None else np.zeros((0, n, n)), B, fac)
    err, scale = np.abs(X - ref).max(), np.abs(ref).max()
    row(label, T, n, R, plan, err / scale)
    assert X.shape == (R, T, n) and err <= TOL * scale, (label, T, n, R, opt, err / scale)
    return X


def check_columns(label, ctx, T, n, nodes, opt, plan):
    """One bt_cov_columns call under solve_lds = opt against solve_ref.columns, per entry; prints the row, returns C."""
    sv.assert_plan(T, n, len(nodes) * n, opt, *plan)
    D, U, fac = problem(T, n)
    ctx.set_option("solve_lds", opt)
    Cc = cov_columns(ctx, D, U, nodes)
    ref = sv.columns(D, U if U is not None else np.zeros((0, n, n)), nodes, fac)
    err, scale = np.abs(Cc - ref).max(), np.abs(ref).max()
    row(label + " cols", T, n, len(nodes), plan, err / scale)
    assert Cc.shape == ref.shape and err <= TOL * scale, (label, T, n, len(nodes), opt, err / scale)
    return Cc


def small_plan(T, n, opt):
    """A handful of right-hand sides: tile 1, in LDS when allowed (every such shape fits)."""
    assert 8 * T * n <= sv.sr.LDS_BYTES
    return (bool(opt), 1, 1)


def context(T, n):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    return ctx


@pytest.mark.parametrize("n", sv.N_ALL)
def test_every_state_size(n):
    ctx = api.Context(0)
    for T in sv.GROW_SHRINK_T:
        ctx.chain_set(T, n)
        for opt in (1, 0):
            check_solve("size", ctx, T, n, 3, opt, small_plan(T, n, opt))
            check_columns("size", ctx, T, n, [T - 1, 0, T // 2], opt, small_plan(T, n, opt))
    ctx.close()


@pytest.mark.parametrize("n", sv.ENUM_N)
def test_every_node_enumeration(n):
    ctx = api.Context(0)
    for T in sv.ENUM_T:
        ctx.chain_set(T, n)
        for opt in (1, 0):
            check_solve("enum", ctx, T, n, 2, opt, small_plan(T, n, opt))
            check_columns("enum", ctx, T, n, [0, T - 1], opt, small_plan(T, n, opt))
    ctx.close()


@pytest.mark.parametrize("T,n", sv.MANY_NODES)
def test_more_nodes_than_lane_groups(T, n):
    groups = SWEEP_WAVES * (64 // n)
    assert (T + 1) // 2 > groups and T // 2 > groups          # level 0, up and down: a lane group takes a second node
    ctx = context(T, n)
    for opt in (1, 0):
        check_solve("groups", ctx, T, n, 3, opt, small_plan(T, n, opt))
        check_columns("groups", ctx, T, n, [T // 3], opt, small_plan(T, n, opt))
    ctx.close()


@pytest.mark.parametrize("T,n,R,opt,lds,tile,last", sv.GENERAL_ROWS)
def test_general_tiles(T, n, R, opt, lds, tile, last):
    if (T, n, R) == (375, 8, 1537):
        assert (R + 511) // 512 == 4 and sv.sr.LDS_BYTES // (8 * T * n) == 3     # capped by LDS, not by the count
    if (T, n) == (640, 16):
        assert 8 * T * n == sv.sr.LDS_BYTES                                      # one vector takes the whole allocation
    ctx = context(T, n)
    check_solve("tiles", ctx, T, n, R, opt, (lds, tile, last))
    ctx.close()


@pytest.mark.parametrize("T,n,ncols,opt,lds,tile,last", sv.COLUMN_ROWS)
def test_column_tiles(T, n, ncols, opt, lds, tile, last):
    nodes = sv.node_list(T, ncols)
    if (T, n, ncols) in sv.STRADDLE:                           # tiles whose right-hand sides belong to two different nodes
        two = [j0 for j0 in range(0, ncols * n, tile) if j0 // n != (min(j0 + tile, ncols * n) - 1) // n]
        assert two and all(nodes[j0 // n] != nodes[j0 // n + 1] for j0 in two)
    ctx = context(T, n)
    Cc = check_columns("tiles", ctx, T, n, nodes, opt, (lds, tile, last))
    if (T, n, ncols) in sv.STRADDLE:
        # the same arithmetic on explicit unit columns, [c n + k][t][r]: only the layout differs
        X = ctx.bt_solve_multi(*problem(T, n)[:2], sv.unit_columns(T, n, nodes))
        assert np.array_equal(Cc, X.reshape(ncols, n, T, n).transpose(0, 2, 3, 1))
    ctx.close()


@pytest.mark.parametrize("T,n,opt", sv.CONTIGUITY)
def test_contiguity_at_a_ragged_tile_edge(T, n, opt):
    R, ncols = 513, 75
    lds = bool(opt) and 8 * T * n <= sv.sr.LDS_BYTES
    D, U, _ = problem(T, n)
    B = rhs(T, n, R)
    ctx = context(T, n)
    X = check_solve("contiguity", ctx, T, n, R, opt, (lds, 2, 1), B)
    sv.assert_plan(T, n, 3, opt, lds, 1, 1)
    assert np.array_equal(ctx.bt_solve_multi(D, U, B[R - 3:]), X[R - 3:])        # last full tile + the ragged one
    assert np.array_equal(ctx.bt_solve_multi(D, U, B[1:3]), X[1:3])              # across the first tile edge
    nodes = sv.node_list(T, ncols)
    Cc = check_columns("contiguity", ctx, T, n, nodes, opt, (lds, 2, 1))
    sv.assert_plan(T, n, n, opt, lds, 1, 1)
    for c in (ncols - 1, 1):                                                     # the ragged tile's column; one inside
        assert np.array_equal(ctx.bt_cov_columns(D, U, [nodes[c]])[0], Cc[c]), c
    ctx.close()


@pytest.mark.parametrize("cols,T,n,count,lds,tile,last",
                         [(False,) + c for c in sv.NOT_PD_GENERAL] + [(True,) + c for c in sv.NOT_PD_COLUMNS])
def test_not_positive_definite(cols, T, n, count, lds, tile, last):
    D, U, _ = problem(T, n)
    Dbad = D.copy()
    Dbad[T // 2] = -np.eye(n)
    B, nodes = (None, sv.node_list(T, count)) if cols else (rhs(T, n, count), None)
    ctx = context(T, n)
    for opt in (1, 0) if lds else (1,):
        plan = (lds and bool(opt), tile, last)
        sv.assert_plan(T, n, count * n if cols else count, opt, *plan)
        ctx.set_option("solve_lds", opt)
        X = ctx.bt_cov_columns(Dbad, U, nodes) if cols else ctx.bt_solve_multi(Dbad, U, B)
        assert X.shape == ((count, T, n, n) if cols else (count, T, n)) and np.all(np.isnan(X)), opt
        if cols:                                                    # nothing of the NaN state is left over
            check_columns("after nan", ctx, T, n, nodes, opt, plan)
        else:
            check_solve("after nan", ctx, T, n, count, opt, plan, B)
    ctx.close()


def test_callers_device_buffer():
    import torch
    ch = syn.make_chain("c2")
    ctx, _ = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    for _ in range(2):
        ctx.ngd_step(0.55, 10)
    T, n, pad = ctx.T, ctx.n, 1024
    ncols = (513 + n - 1) // n
    nodes = sv.node_list(T, ncols)
    plan = (True, 2, sv.last_tile(ncols * n, 2))
    sv.assert_plan(T, n, ncols * n, 1, *plan)
    Cc = ctx.ngd_cov_columns(nodes)
    st = ctx.ngd_get_state()
    assert np.all(np.isfinite(Cc)) and np.array_equal(Cc, ctx.bt_cov_columns(st["D"], st["U"], nodes))
    sentinel = -1.2345678901234567e300
    buf = torch.full((Cc.size + pad,), sentinel, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ngd_cov_columns_dev(nodes, buf.data_ptr())
    ctx.sync()
    out = buf.cpu().numpy()
    assert np.array_equal(out[:Cc.size].view(np.int64), Cc.reshape(-1).view(np.int64))
    assert np.array_equal(out[Cc.size:].view(np.int64), np.full(pad, sentinel).view(np.int64))
    print(f"    ROW device buffer cols T {T} n {n} count {ncols} NM 4 mode lds tile {plan[1]} last {plan[2]} bits equal, "
          f"{pad} doubles behind untouched")
    ctx.close()
