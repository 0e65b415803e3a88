"""The sampler's sweep (kernels_sample.hpp: sample_sweep_kernel<NM, LDSY>) per entry, at every state size, node enumeration,
tile length and memory mode, and gvi_bt_logpdf at every n (-m gpu).

Reference: tests/sample_ref.py::cr_sample, the float64 restatement of the back-sweep on the caller's eps.  A sample is a
function of (D, U, eps) alone (Cholesky pivots with positive diagonal, fixed elimination order), so every entry of X has one
right value; tests/test_sample_host.py proves the restatement at every shape used here (<= 8.6e-16 against the dense inverse,
<= 8.8e-16 on F^T Lambda F = I, cond <= 25).  Bound: max |X - ref| <= 1e-10 max |ref - mu| per case, the bound of
test_sample_gpu and test_solve_gpu; log-density 1e-10 relative to q / 2 + |hld| + T n log(2 pi) / 2, because log q itself may
cancel.  Every case first asserts the mode (y in LDS / in the caller's output buffer), the tile length and the size of the last
tile it was written for against sample_ref.sweep_plan -- the library reports neither, so the restated plan is the only check --
then prints `ROW <case> T n S NM mode tile last err`.  The figures measured on the MI355X are in profiles/sample_sweep_tests.txt.

test_every_state_size      n = 1 .. 16, one context per n, chain_set over T = 1, 2, 3, 6, 17, 4 (smp_ws / smp_io carved again, larger
                           and smaller), S = 3: idle tail lanes when 64 % n != 0, the instance boundaries 4|5 and 8|9, T = 1 with
                           U = NULL at the C ABI.
test_every_node_enumeration  T = 1 .. 20, 31 .. 34, 63 .. 66, 127 .. 130 at n = 3 and 16, S = 2, one context per n.
test_more_eliminations_than_lane_groups  (2051, 1), (700, 3), (131, 16): level 0 has more nodes than 8 (64 // n) groups (q += NG).
test_tiles                 LDS mode: (7, 4) at S = 513 / 1100 / 3585 / 4096 (tile 2 / 3 / 8 / 8, last 1 / 2 / 1 / 8), (9, 6) and (5, 13)
                           at S = 513 / 3585; tile capped by LDS: (375, 8), S = 1537 (count asks 4, LDS allows 3, last 1); the
                           80 KB boundary: (640, 16) LDS with one row = 81920 bytes, (641, 16) output buffer; output-buffer mode
                           with tile 2, last 1 at (2561, 4), (1281, 8), (641, 16), (1465, 7), (789, 13), S = 513, and tile 3, last 2
                           at (1281, 8), S = 1025.
test_generated_normals     (9, 7) at S = 513, 1100 and (1465, 7) at S = 513, 1025, first = 0 and 5: bt_sample(seed, first) is
                           bit-equal to bt_sample(eps = randn(seed, first T n, S T n)), and that is within the bound of cr_sample.
                           T n is odd; with tile 2 the pair base (first + j0) T n has the parity of `first` in every tile, so odd
                           and even bases inside ONE launch need an odd tile: the S = 1100 and S = 1025 rows (tile 3), asserted.
test_contiguity_at_a_ragged_tile_edge  X[S - 3:] and X[1:3] of an S = 513 call equal short calls with `first` advanced, bit for bit,
                           in both modes.
test_not_positive_definite one block of D = -I: every entry NaN at (7, 4, 513) and (641, 16, 2), given and generated normals; the
                           next call in the context with the good (D, U) is within the bound.
test_callers_device_buffer ngd_sample_dev on the c2 chain, S = 513, into a torch buffer with 1024 sentinel doubles behind it: the
                           samples equal ngd_sample and the tail is untouched, bit for bit.
test_logpdf_every_state_size  bt_logpdf for n = 1 .. 16 at T = 1, 2, 3, 300 (300 crosses the 256-thread reduction, S T = 2100 is no
                           multiple of 256), S = 1, 7, X = mu + 0.3 N(0, 1), against the block mat-vec and sample_ref.half_logdet.

Measured on the MI355X: all 63 tests pass on the unmodified library (4.3 s), so no source file changes.  Worst error per
instance and mode over the 190 sweep rows:
    NM 4    LDS 5.3e-16    output buffer 4.7e-16
    NM 8    LDS 7.4e-16    output buffer 6.3e-16
    NM 16   LDS 8.1e-16    output buffer 1.2e-15
and 2.0e-16 over the 128 log-density rows.

Sensitivity: five arithmetic-only edits to a scratch copy of kernels_sample.hpp (no address, loop bound, predicate, barrier or
wait count touched), each run once on this module and on test_sample_gpu (17 tests without the shim test, which links the
in-tree library):
  + for - on the GB term of the sweep      every per-entry test fails (44: every_state_size 16, every_node_enumeration 2,
                                           more_eliminations 3, tiles 17, generated_normals 4, not_positive_definite 2);
                                           test_sample_gpu: 8 (exact_covariance at T >= 7, sample_statistics, logpdf_of_samples)
  Ar for Br in the GB product              the same 44 and the same 8
  x = mu - y                               the same 44; test_sample_gpu: none -- F F^T, the 6-sigma statistics and |eps|^2 are
                                           all even in y
  z0 / z1 swapped in the sweep's generator generated_normals (4); test_sample_gpu: stream_properties
  0.5 dropped in logpdf_reduce_kernel      logpdf_every_state_size (16); test_sample_gpu: logpdf_matches_dense, logpdf_of_samples
The bit-equality tests (contiguity, device buffer) compare the library with itself and pass under every edit.

What this cannot see: the results are right with the vmcnt drains of the output-buffer mode in place; that does not show the
drains are necessary (a run without them may pass by timing), and they were not removed to find out.  A sample-to-sample
mix-up inside a tile would be seen (every sample has its own eps and reference), but no such edit was tried: it would touch an
address."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import sample_ref as sr
from gaussianvi_amd import api, synthetic as syn
from test_solve_host import cr_factor, random_chain

pytestmark = pytest.mark.gpu
TOL = 1e-10
LOG2PI = math.log(2.0 * math.pi)
SWEEP_GROUPS_PER_BLOCK = 8           # SAMPLE_SWEEP_THREADS / 64 waves, each with 64 // n lane groups


@functools.lru_cache(maxsize=None)
def problem(T, n):
    """(D, U, mu, cr_factor(D, U)) of a shape, the chain tests/test_sample_host.py proves the reference on: computed once,
    never written to.  U is None on a single-state chain."""
    D, U, mu = random_chain(T, n, 100 + T * n)
    fac = cr_factor(D, U)
    for a in (D, U, mu) + fac:
        a.setflags(write=False)
    return D, (U if T > 1 else None), mu, fac


def normals(T, n, S):
    return np.random.default_rng(1000 * S + T * n).standard_normal((S, T, n))


def sample(ctx, D, U, mu, S, seed=0, first=0, eps=None):
    """ctx.bt_sample; a single-state chain goes to the C ABI with U = NULL."""
    if U is not None:
        return ctx.bt_sample(D, U, mu, S, seed=seed, first=first, eps=eps)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    X = np.empty((S, ctx.T, ctx.n))
    ctx._ck(ctx.lib.gvi_bt_sample(ctx.h, p(D), None, p(mu), S, seed, first, p(eps), p(X)))
    return X


def assert_plan(T, n, S, lds, tile, last):
    """The case reaches the mode, tile length and last tile it was written for (sample_ref.sweep_plan: the only check)."""
    assert sr.sweep_plan(S, T, n) == (lds, tile), (T, n, S, sr.sweep_plan(S, T, n))
    assert sr.last_tile(S, tile) == last, (T, n, S)


def check(label, ctx, T, n, S, plan, eps):
    """One call with the caller's eps against cr_sample, per entry; prints the row, returns X."""
    assert_plan(T, n, S, *plan)
    D, U, mu, fac = problem(T, n)
    X = sample(ctx, D, U, mu, S, eps=eps)
    ref = mu + sr.cr_sample(D, U, eps, fac)
    err, scale = np.abs(X - ref).max(), np.abs(ref - mu).max()
    print(f"    ROW {label} T {T} n {n} S {S} NM {4 if n <= 4 else 8 if n <= 8 else 16} mode {'lds' if plan[0] else 'buffer'} "
          f"tile {plan[1]} last {plan[2]} err {err / scale:.2e}")
    assert err <= TOL * scale, (label, T, n, S, err / scale)
    return X


@pytest.mark.parametrize("n", sr.N_ALL)
def test_every_state_size(n):
    ctx = api.Context(0)
    for T in sr.GROW_SHRINK_T:
        ctx.chain_set(T, n)
        check("size", ctx, T, n, 3, (True, 1, 1), normals(T, n, 3))
    ctx.close()


@pytest.mark.parametrize("n", sr.ENUM_N)
def test_every_node_enumeration(n):
    ctx = api.Context(0)
    for T in sr.ENUM_T:
        ctx.chain_set(T, n)
        check("enum", ctx, T, n, 2, (True, 1, 1), normals(T, n, 2))
    ctx.close()


def context(T, n):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    return ctx


@pytest.mark.parametrize("T,n", sr.MANY_NODES)
def test_more_eliminations_than_lane_groups(T, n):
    assert T // 2 > SWEEP_GROUPS_PER_BLOCK * (64 // n)        # level 0: a lane group takes a second node
    ctx = context(T, n)
    check("groups", ctx, T, n, 2, (True, 1, 1), normals(T, n, 2))
    ctx.close()


@pytest.mark.parametrize("T,n,S,lds,tile,last", sr.LDS_TILES + sr.LDS_CAPPED + sr.BOUNDARY + sr.BUFFER_TILES)
def test_tiles(T, n, S, lds, tile, last):
    if (T, n, S) == sr.LDS_CAPPED[0][:3]:
        assert (S + 511) // 512 == 4 and sr.LDS_BYTES // (8 * T * n) == 3     # capped by LDS, not by the count
    if (T, n) == sr.BOUNDARY[0][:2]:
        assert 8 * T * n == sr.LDS_BYTES                                      # one row takes the whole allocation
    ctx = context(T, n)
    check("tiles", ctx, T, n, S, (lds, tile, last), normals(T, n, S))
    ctx.close()


@pytest.mark.parametrize("T,n,S,lds,tile,last", sr.GENERATED)
def test_generated_normals(T, n, S, lds, tile, last):
    seed = 20261019
    ctx = context(T, n)
    for first in (0, 5):
        bases = {(first + j0) * T * n % 2 for j0 in range(0, S, tile)}
        assert T * n % 2 == 1 and bases == ({0, 1} if tile % 2 else {first % 2})     # the pair base of the tiles: odd and even
        Xg = ctx.bt_sample(*problem(T, n)[:3], S, seed=seed, first=first)
        eps = ctx.randn(seed, first * T * n, S * T * n).reshape(S, T, n)
        Xe = check(f"generated first {first}", ctx, T, n, S, (lds, tile, last), eps)
        assert np.array_equal(Xg, Xe), first
    ctx.close()


@pytest.mark.parametrize("T,n,S,lds,tile,last", [sr.LDS_TILES[0], sr.BUFFER_TILES[3]])
def test_contiguity_at_a_ragged_tile_edge(T, n, S, lds, tile, last):
    assert_plan(T, n, S, lds, tile, last)
    assert tile == 2 and last == 1
    D, U, mu, _ = problem(T, n)
    ctx = context(T, n)
    X = ctx.bt_sample(D, U, mu, S, seed=7, first=3)
    assert_plan(T, n, 3, lds, 1, 1)
    assert np.array_equal(ctx.bt_sample(D, U, mu, 3, seed=7, first=3 + S - 3), X[S - 3:])     # last full tile + the ragged one
    assert np.array_equal(ctx.bt_sample(D, U, mu, 2, seed=7, first=4), X[1:3])                # across the first tile edge
    ctx.close()


@pytest.mark.parametrize("T,n,S,lds,tile,last", sr.NOT_PD)
def test_not_positive_definite(T, n, S, lds, tile, last):
    assert_plan(T, n, S, lds, tile, last)
    D, U, mu, _ = problem(T, n)
    Dbad = D.copy()
    Dbad[T // 2] = -np.eye(n)
    eps = normals(T, n, S)
    ctx = context(T, n)
    for kw in ({"eps": eps}, {"seed": 3}):
        assert np.all(np.isnan(ctx.bt_sample(Dbad, U, mu, S, **kw))), kw
    check("after nan", ctx, T, n, S, (lds, tile, last), eps)       # nothing of the NaN state is left over
    ctx.close()


def test_callers_device_buffer():
    import torch
    ch = syn.make_chain("c2")
    ctx, _ = api.context_for_chain(ch)
    ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    for _ in range(2):
        ctx.ngd_step(0.55, 10)
    T, n, S, seed, first, pad = ctx.T, ctx.n, 513, 99, 2, 1024
    assert_plan(T, n, S, True, 2, 1)
    X = ctx.ngd_sample(S, seed=seed, first=first)
    assert np.all(np.isfinite(X))
    sentinel = -1.2345678901234567e300
    buf = torch.full((S * T * n + pad,), sentinel, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ngd_sample_dev(S, buf.data_ptr(), seed=seed, first=first)
    ctx.sync()
    out = buf.cpu().numpy()
    assert np.array_equal(out[:S * T * n].view(np.int64), X.reshape(-1).view(np.int64))
    assert np.array_equal(out[S * T * n:].view(np.int64), np.full(pad, sentinel).view(np.int64))
    print(f"    ROW device buffer T {T} n {n} S {S} NM 4 mode lds tile 2 last 1 bits equal, {pad} doubles behind untouched")
    ctx.close()


@pytest.mark.parametrize("n", sr.N_ALL)
def test_logpdf_every_state_size(n):
    ctx = api.Context(0)
    for T in sr.LOGPDF_T:
        ctx.chain_set(T, n)
        D, U, mu, fac = problem(T, n)
        Uarg = U if U is not None else np.zeros((0, n, n))
        hld = sr.half_logdet(D, U, fac)
        for S in sr.LOGPDF_S:
            X = mu + 0.3 * np.random.default_rng(S * T + n).standard_normal((S, T, n))
            d = X - mu
            q = (d * sr.block_matvec(D, Uarg, d)).reshape(S, -1).sum(axis=1)
            ref = -0.5 * q + hld - 0.5 * T * n * LOG2PI
            scale = 0.5 * q + abs(hld) + 0.5 * T * n * LOG2PI          # log q itself may cancel
            lq = ctx.bt_logpdf(D, Uarg, mu, X)
            err = (np.abs(lq - ref) / scale).max()
            print(f"    ROW logpdf T {T} n {n} S {S} err {err:.2e}")
            assert err <= TOL, (T, n, S, err)
    ctx.close()
