"""Argument rules and staging of the posterior query calls (include/gvi_hip.h: sampling and log-density, many right-hand sides,
dense-time posterior, costs of sampled trajectories), through the raw C ABI.

Every query call checks its preconditions in one order:

    ctx null -> count < 0 -> chain not set -> NULL argument -> first < 0 -> bad set id -> ngd not initialised -> state_dim > 16
    -> node outside [0, T) -> interp set missing -> set not evaluable -> zero-count early return

test_error_table breaks one precondition at a time and then two at once (the earlier one is reported); the other tests pin
the zero-count no-ops, the single-state chain (U = NULL), that nothing staged by one call survives into the next, and that
the host and _dev variants of a call give the same bits.  Nothing here is larger than S = 64.

Bounds of test_single_state_chain: the 1e-10 relative of test_sample_gpu.test_exact_covariance_from_identity_eps for the
samples, rtol 1e-10 of test_sample_gpu.test_logpdf_matches_dense, TOL = 1e-10 of test_solve_gpu for the solves."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from gaussianvi_amd import api, synthetic as syn

pytestmark = pytest.mark.gpu
OK, ARG, UNSUP, STATE = 0, 1, 3, 5
CH, NG, IT = "call gvi_chain_set first", "call gvi_ngd_init first", "call gvi_interp_set first"
NU, FI, SD, ND, BS = "NULL argument", "first < 0", "state_dim > 16", "node outside [0, T)", "bad set id"
CB, CL = "a PSI_HOST_CALLBACK set has no device psi", "clearance needs a hinge-on-SDF set"
REGION = 2048                                # doubles per scratch region; the largest array of the table has 1734


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a


def raw(ctx, name, *args, h="own"):
    """(status, last error) of the C function `name`; numpy arrays go as pointers, ints as device pointers or values."""
    lib = ctx.lib
    hh = ctx.h if h == "own" else h
    assert lib.gvi_chain_set(ctx.h, 0, 0) == ARG             # a known last error: a stale message cannot pass for a new one
    st = getattr(lib, name)(hh, *[_p(a) for a in args])
    return st, lib.gvi_last_error(ctx.h).decode()


def run(ctx, name, *args):
    st, msg = raw(ctx, name, *args)
    assert st == OK, (name, st, msg)


# ---- contexts ----
def interp_queries(T, n, Q, seed=7):
    rng = np.random.default_rng(seed)
    idx = (np.arange(Q) % max(T - 1, 1)).astype(np.int32)
    A, B = rng.normal(size=(Q, n, n)) * 0.5, rng.normal(size=(Q, n, n)) * 0.5
    c = rng.normal(size=(Q, n))
    G = rng.normal(size=(Q, n, n))
    Qt = 0.1 * np.eye(n) + 0.05 * G @ G.transpose(0, 2, 1)
    return idx, A, B, c, Qt


@functools.lru_cache(maxsize=None)
def planar_chain():
    return syn.make_planar_chain(T=2)        # T - 1 priors: T = 2 is the smallest the generator makes


def planar(ngd=True, interp=True):
    """(ctx, set ids): the planar chain at T = 2, n = 4 (priors, hinge-on-SDF obstacles, anchors); Q = 3 queries with noise."""
    ch = planar_chain()
    ctx, ids = api.context_for_chain(ch)
    if ngd:
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
    if interp:
        ctx.interp_set(*interp_queries(ch["T"], ch["n"], 3))
    return ctx, ids


def bare(T, n, interp=False):
    ctx = api.Context(0)
    ctx.chain_set(T, n)
    if interp:
        ctx.interp_set(*interp_queries(T, n, 2))
    return ctx


@functools.lru_cache(maxsize=None)
def table_contexts():
    """The contexts of the table, made once; the tests change none of them.
    plan: everything in place.  noitp: plan without the query set.  bare3: T = 3, n = 2, a query set, two EMPTY sets (0: fixed
    prior, 1: hinge on a grid), no resident state.  cb: bare3's chain with one PSI_HOST_CALLBACK set.  wide: gvi_chain_set(2, 17),
    where neither a query set nor a resident state can exist.  nochain: no gvi_chain_set."""
    b3 = bare(3, 2, interp=True)
    assert b3.factors_add(2, 3, np.zeros(0, np.int32), syn.PSI_FIXED_PRIOR, np.zeros((0, 6)), np.zeros(0)) == 0
    assert b3.factors_add(2, 3, np.zeros(0, np.int32), syn.PSI_HINGE_SDF_2D, np.zeros((0, 3)), np.zeros(0)) == 1
    b3.factors_set_sdf2d(1, (-1.0, -1.0), 0.5, np.ones((5, 5)))
    cb = bare(3, 2)
    assert cb.factors_add(2, 3, np.zeros(2, np.int32), api.PSI_HOST_CALLBACK) == 0
    return dict(plan=planar()[0], noitp=planar(interp=False)[0], bare3=b3, cb=cb, wide=bare(2, 17), nochain=api.Context(0))


# ---- one argument list per entry: scratch regions stand for every buffer, so only the checks decide what a call does ----
class Scratch:
    def __init__(self):
        import torch
        self.host = np.full(6 * REGION, 7.0)
        self.dev = torch.full((6 * REGION,), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()

    def region(self, dev, i):
        return self.dev.data_ptr() + 8 * i * REGION if dev else self.host[i * REGION:(i + 1) * REGION]

    def untouched(self):
        return bool((self.host == 7.0).all()) and bool((self.dev.cpu().numpy() == 7.0).all())


@functools.lru_cache(maxsize=None)
def scratch():
    return Scratch()


def arguments(name, cnt=2, first=0, sid=None, null=False, nodes=(0, 1)):
    """The arguments of entry `name` behind ctx: region 0 is the (last) output, NULL when `null`."""
    r = functools.partial(scratch().region, name.endswith("_dev"))
    host = functools.partial(scratch().region, False)
    out = None if null else r(0)
    nd = np.asarray(nodes, dtype=np.int32)
    base = name[4:-4] if name.endswith("_dev") else name[4:]
    if base == "bt_sample":
        return (host(1), host(2), host(3), cnt, 1, first, None, out)
    if base == "ngd_sample":
        return (cnt, 1, first, out)
    if base == "bt_logpdf":
        return (host(1), host(2), host(3), cnt, host(4), out)
    if base == "bt_solve_multi":
        return (host(1), host(2), cnt, host(4), out)
    if base == "bt_cov_columns":
        return (host(1), host(2), cnt, nd, out)
    if base == "ngd_cov_columns":
        return (cnt, nd, out)
    if base == "bt_interp":
        return (host(1), host(2), host(3), host(4), out)
    if base == "ngd_interp":
        return (r(1), out)
    if base == "bt_interp_samples":
        return (cnt, host(1), 7, first, None, out)
    if base == "ngd_sample_interp":
        return (cnt, 1, 7, first, r(1), out)
    if base in ("sample_factor_costs", "sample_clearance"):
        return (1 if sid is None else sid, cnt, r(1), out)
    if base == "sample_costs":
        return (cnt, r(1), out)
    if base == "ngd_sample_costs":
        return (cnt, 1, first, -1 if sid is None else sid, r(1), out, r(2), r(3))
    raise KeyError(name)


COUNT_NAME = {"gvi_bt_solve_multi": "R", "gvi_bt_cov_columns": "ncols", "gvi_ngd_cov_columns": "ncols",
              "gvi_ngd_cov_columns_dev": "ncols"}
NO_COUNT = ("gvi_bt_interp", "gvi_ngd_interp", "gvi_ngd_interp_dev")

# (context, broken preconditions, status, message).  NEG stands for "<the entry's count name> < 0".  The rows every entry has
# (ctx null; count < 0; chain not set; NULL output; and count < 0 with a NULL output at once) are COMMON; `single` breaks
# one more precondition each, `pairs` two at once or one with a zero count (the zero-count return comes last).
# Not reachable: "state_dim > 16" alone in the gvi_ngd_* entries (no resident state exists at n > 16: on `wide` the missing
# gvi_ngd_init is reported, a pair); "ncols * state_dim exceeds 2^31 - 1" (a node list of 2^27 entries); a second
# precondition of gvi_interp_info (it has the null context only).
COMMON = [("plan", dict(h=None), ARG, None), ("plan", dict(cnt=-1), ARG, "NEG"), ("nochain", {}, STATE, CH),
          ("plan", dict(null=True), ARG, NU), ("plan", dict(cnt=-1, null=True), ARG, "NEG"), ("nochain", dict(null=True), STATE, CH)]
NGD_SAMPLE = dict(
    single=[("plan", dict(first=-1), ARG, FI), ("bare3", {}, STATE, NG)],
    pairs=[("wide", {}, STATE, NG), ("bare3", dict(first=-1), ARG, FI), ("plan", dict(first=-1, null=True), ARG, NU),
           ("bare3", dict(cnt=0), STATE, NG)])
NGD_COLUMNS = dict(
    single=[("bare3", {}, STATE, NG), ("plan", dict(nodes=(0, 2)), ARG, ND), ("plan", dict(nodes=(-1, 0)), ARG, ND)],
    pairs=[("wide", {}, STATE, NG), ("bare3", dict(nodes=(7, 0)), STATE, NG), ("bare3", dict(null=True), ARG, NU),
           ("plan", dict(cnt=0, nodes=(9, 9)), OK, None)])
NGD_INTERP = dict(
    single=[("bare3", {}, STATE, NG), ("noitp", {}, STATE, IT)],
    pairs=[("wide", {}, STATE, NG), ("bare3", dict(null=True), ARG, NU), ("noitp", dict(null=True), ARG, NU)])
NGD_SAMPLE_INTERP = dict(
    single=[("plan", dict(first=-1), ARG, FI), ("bare3", {}, STATE, NG), ("noitp", {}, STATE, IT)],
    pairs=[("wide", {}, STATE, NG), ("noitp", dict(first=-1), ARG, FI), ("bare3", dict(null=True), ARG, NU),
           ("noitp", dict(cnt=0), STATE, IT), ("bare3", dict(first=-1), ARG, FI)])
SET_MATRIX = dict(
    single=[("plan", dict(sid=3), ARG, BS), ("plan", dict(sid=-1), ARG, BS), ("cb", dict(sid=0), UNSUP, CB)],
    pairs=[("plan", dict(sid=3, null=True), ARG, NU), ("cb", dict(sid=0, cnt=-1), ARG, "NEG"), ("cb", dict(sid=0, cnt=0), UNSUP, CB),
           ("nochain", dict(sid=9), STATE, CH)])
CLEARANCE = dict(single=SET_MATRIX["single"] + [("plan", dict(sid=0), UNSUP, CL)],
                 pairs=SET_MATRIX["pairs"] + [("plan", dict(sid=0, cnt=0), UNSUP, CL), ("plan", dict(sid=0, null=True), ARG, NU)])
SAMPLE_COSTS = dict(single=[("cb", {}, UNSUP, CB)],
                    pairs=[("cb", dict(null=True), ARG, NU), ("cb", dict(cnt=0), UNSUP, CB), ("nochain", dict(cnt=-1), ARG, "NEG")])
NGD_SAMPLE_COSTS = dict(
    single=[("plan", dict(first=-1), ARG, FI), ("plan", dict(sid=3), ARG, BS), ("bare3", {}, STATE, NG),
            ("plan", dict(sid=0), UNSUP, CL)],
    pairs=[("bare3", dict(sid=5), ARG, BS), ("plan", dict(first=-1, sid=0), ARG, FI), ("wide", {}, STATE, NG),
           ("plan", dict(sid=0, cnt=0), UNSUP, CL), ("plan", dict(first=-1, sid=3), ARG, FI), ("plan", dict(sid=3, null=True), ARG, NU)])
TABLE = {
    "gvi_bt_sample": dict(
        single=[("plan", dict(first=-1), ARG, FI), ("wide", {}, UNSUP, SD)],
        pairs=[("wide", dict(null=True), ARG, NU), ("wide", dict(first=-1), ARG, FI), ("nochain", dict(cnt=-1), ARG, "NEG"),
               ("wide", dict(cnt=0), UNSUP, SD)]),
    "gvi_ngd_sample": NGD_SAMPLE,
    "gvi_ngd_sample_dev": NGD_SAMPLE,
    "gvi_bt_logpdf": dict(single=[("wide", {}, UNSUP, SD)], pairs=[("wide", dict(null=True), ARG, NU), ("wide", dict(cnt=0), UNSUP, SD)]),
    "gvi_bt_solve_multi": dict(single=[("wide", {}, UNSUP, SD)],
                               pairs=[("wide", dict(cnt=-1), ARG, "NEG"), ("wide", dict(null=True), ARG, NU), ("wide", dict(cnt=0), UNSUP, SD)]),
    "gvi_bt_cov_columns": dict(
        single=[("wide", {}, UNSUP, SD), ("plan", dict(nodes=(0, 2)), ARG, ND), ("plan", dict(nodes=(-1, 0)), ARG, ND)],
        pairs=[("wide", dict(nodes=(5, 0)), UNSUP, SD), ("plan", dict(null=True, nodes=(0, 2)), ARG, NU), ("wide", dict(cnt=0), UNSUP, SD),
               ("plan", dict(cnt=0, nodes=(9, 9)), OK, None)]),
    "gvi_ngd_cov_columns": NGD_COLUMNS,
    "gvi_ngd_cov_columns_dev": NGD_COLUMNS,
    # no state_dim rule of its own: at n > 16 no query set can be made, so `wide` misses the set only
    "gvi_bt_interp": dict(single=[("noitp", {}, STATE, IT), ("wide", {}, STATE, IT)], pairs=[("noitp", dict(null=True), ARG, NU)]),
    "gvi_ngd_interp": NGD_INTERP,
    "gvi_ngd_interp_dev": NGD_INTERP,
    "gvi_bt_interp_samples": dict(
        single=[("plan", dict(first=-1), ARG, FI), ("noitp", {}, STATE, IT)],
        pairs=[("noitp", dict(first=-1), ARG, FI), ("noitp", dict(cnt=0), STATE, IT), ("plan", dict(first=-1, null=True), ARG, NU)]),
    "gvi_ngd_sample_interp": NGD_SAMPLE_INTERP,
    "gvi_ngd_sample_interp_dev": NGD_SAMPLE_INTERP,
    "gvi_sample_factor_costs": SET_MATRIX,
    "gvi_sample_clearance": CLEARANCE,
    "gvi_sample_clearance_dev": CLEARANCE,
    "gvi_sample_costs": SAMPLE_COSTS,
    "gvi_sample_costs_dev": SAMPLE_COSTS,
    "gvi_ngd_sample_costs": NGD_SAMPLE_COSTS,
    "gvi_ngd_sample_costs_dev": NGD_SAMPLE_COSTS,
}


def test_error_table():
    ctxs = table_contexts()
    nrows = 0
    for name, rows in TABLE.items():
        common = [r for r in COMMON if not (name in NO_COUNT and "cnt" in r[1])]
        for cname, broken, status, msg in common + rows["single"] + rows["pairs"]:
            kw = dict(broken)
            h = kw.pop("h", "own")
            if name in NO_COUNT:
                kw.pop("cnt", None)
            ctx = ctxs[cname]
            st, got = raw(ctx, name, *arguments(name, **kw), h=h)
            want = f"{COUNT_NAME.get(name, 'S')} < 0" if msg == "NEG" else msg
            assert st == status, (name, cname, broken, st, got)
            if status != OK and h == "own":
                assert got == want, (name, cname, broken, got)
            nrows += 1
        assert rows["pairs"], name
    ctx = ctxs["plan"]
    Q, nbad = C.c_int(-1), C.c_int(-1)
    assert ctx.lib.gvi_interp_info(None, C.byref(Q), C.byref(nbad)) == ARG and Q.value == -1
    assert ctx.lib.gvi_interp_info(ctx.h, C.byref(Q), None) == OK and Q.value == 3
    assert ctxs["noitp"].lib.gvi_interp_info(ctxs["noitp"].h, C.byref(Q), C.byref(nbad)) == OK and (Q.value, nbad.value) == (0, 0)
    print(f"{nrows} rows over {len(TABLE)} entries")
    assert scratch().untouched()             # no refused call wrote anything


def test_zero_counts():
    ctxs = table_contexts()
    for name in TABLE:
        if name not in NO_COUNT:
            assert raw(ctxs["plan"], name, *arguments(name, cnt=0))[0] == OK, name
    # K = 0: the per-set matrices of an empty set
    assert raw(ctxs["bare3"], "gvi_sample_factor_costs", *arguments("gvi_sample_factor_costs", sid=0))[0] == OK
    for name in ("gvi_sample_factor_costs", "gvi_sample_clearance", "gvi_sample_clearance_dev"):
        assert raw(ctxs["bare3"], name, *arguments(name, sid=1))[0] == OK, name
    run(ctxs["plan"], "gvi_ctx_sync")
    assert scratch().untouched()


# ---- values ----
def rel(X, ref):
    return np.abs(X - ref).max() / np.abs(ref).max()


def test_single_state_chain():
    n, S = 2, 5
    rng = np.random.default_rng(11)
    D = np.array([[[2.0, 0.3], [0.3, 1.5]]])
    mu = np.array([[0.7, -1.1]])
    eps, B = rng.standard_normal((S, 1, n)), rng.standard_normal((S, 1, n))
    L = np.linalg.cholesky(D[0])
    ctx = bare(1, n)
    X, lq, Xs, Cc = np.empty((S, 1, n)), np.empty(S), np.empty((S, 1, n)), np.empty((1, 1, n, n))
    run(ctx, "gvi_bt_sample", D, None, mu, S, 0, 0, eps, X)
    ref = mu + np.linalg.solve(L.T, eps[:, 0].T).T[:, None]
    print("sample", rel(X, ref))
    assert rel(X, ref) < 1e-10
    run(ctx, "gvi_bt_logpdf", D, None, mu, S, X, lq)
    Y = (X - mu).reshape(S, n)
    lref = -0.5 * np.einsum("si,ij,sj->s", Y, D[0], Y) + 0.5 * np.linalg.slogdet(D[0])[1] - 0.5 * n * math.log(2.0 * math.pi)
    np.testing.assert_allclose(lq, lref, rtol=1e-10)
    run(ctx, "gvi_bt_solve_multi", D, None, S, B, Xs)
    sref = np.linalg.solve(D[0], B[:, 0].T).T[:, None]
    print("solve", rel(Xs, sref))
    assert rel(Xs, sref) <= 1e-10
    run(ctx, "gvi_bt_cov_columns", D, None, 1, np.zeros(1, np.int32), Cc)
    print("columns", rel(Cc[0, 0], np.linalg.inv(D[0])))
    assert rel(Cc[0, 0], np.linalg.inv(D[0])) <= 1e-10
    ctx.close()


def marginals(ch):
    """(SigD, SigU) of the chain's initial precision, by the dense inverse."""
    T, n = ch["T"], ch["n"]
    A = np.zeros((T * n, T * n))
    for t in range(T):
        A[t * n:(t + 1) * n, t * n:(t + 1) * n] = ch["D0"][t]
        if t + 1 < T:
            A[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] = ch["U0"][t]
            A[(t + 1) * n:(t + 2) * n, t * n:(t + 1) * n] = ch["U0"][t].T
    Sig = np.linalg.inv(A)
    SigD = np.stack([Sig[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
    SigU = np.stack([Sig[t * n:(t + 1) * n, (t + 1) * n:(t + 2) * n] for t in range(T - 1)])
    return SigD, SigU


def staging_ops():
    """name -> (needs the factor sets and the resident state, op(ctx, S) -> tuple of results); inputs depend on S only."""
    ch = planar_chain()
    T, n, Q = ch["T"], ch["n"], 3
    D, U, mu = ch["D0"], ch["U0"], ch["mu0"]
    SigD, SigU = marginals(ch)

    def inputs(S):
        rng = np.random.default_rng(1000 + S)
        return (rng.standard_normal((S, T, n)), mu + 0.3 * rng.standard_normal((S, T, n)), rng.standard_normal((S, Q, n)),
                (np.arange(S) % T).astype(np.int32))

    def sample_eps(ctx, S):
        X = np.empty((S, T, n))
        run(ctx, "gvi_bt_sample", D, U, mu, S, 0, 0, inputs(S)[0], X)
        return (X,)

    def sample(ctx, S):
        X = np.empty((S, T, n))
        run(ctx, "gvi_bt_sample", D, U, mu, S, 11, 2, None, X)
        return (X,)

    def logpdf(ctx, S):
        lq = np.empty(S)
        run(ctx, "gvi_bt_logpdf", D, U, mu, S, inputs(S)[1], lq)
        return (lq,)

    def solve(ctx, S):
        X = np.empty((S, T, n))
        run(ctx, "gvi_bt_solve_multi", D, U, S, inputs(S)[0], X)
        return (X,)

    def columns(ctx, S):
        Cc = np.empty((S, T, n, n))
        run(ctx, "gvi_bt_cov_columns", D, U, S, inputs(S)[3], Cc)
        return (Cc,)

    def interp(ctx, S):
        mean, cov = np.empty((Q, n)), np.empty((Q, n, n))
        run(ctx, "gvi_bt_interp", mu, SigD, SigU, mean, cov)
        return mean, cov

    def interp_samples(ctx, S):
        Xq = np.empty((S, Q, n))
        run(ctx, "gvi_bt_interp_samples", S, inputs(S)[1], 0, 0, inputs(S)[2], Xq)
        return (Xq,)

    def costs(ctx, S):
        J = np.empty(S)
        run(ctx, "gvi_sample_costs", S, inputs(S)[1], J)
        return (J,)

    def ngd_costs(ctx, S):
        X, J, lq, clr = np.empty((S, T, n)), np.empty(S), np.empty(S), np.empty(S)
        run(ctx, "gvi_ngd_sample_costs", S, 5, 1, 1, X, J, lq, clr)
        return X, J, lq, clr

    return dict(sample_eps=(False, sample_eps), sample=(False, sample), logpdf=(False, logpdf), solve=(False, solve),
                columns=(False, columns), interp=(False, interp), interp_samples=(False, interp_samples), costs=(True, costs),
                ngd_costs=(True, ngd_costs))


def test_staging_is_per_call():
    ch = planar_chain()
    ops = staging_ops()
    ctx, _ = planar()
    got = {(k, S): op(ctx, S) for k, (_, op) in ops.items() for S in (5, 64, 3)}
    ctx.close()
    for (k, S), res in got.items():
        if ops[k][0]:
            fresh, _ = planar(interp=False)
        else:
            fresh = bare(ch["T"], ch["n"])
            fresh.interp_set(*interp_queries(ch["T"], ch["n"], 3))
        ref = ops[k][1](fresh, S)
        fresh.close()
        for a, b in zip(res, ref):
            assert np.isfinite(b).all() and np.array_equal(a, b), (k, S)


def test_host_and_dev_variants_agree():
    """Also asserted bit for bit elsewhere, at other shapes: ngd_sample (test_sample_gpu.test_resident_state_samples),
    ngd_cov_columns (test_solve_gpu.test_resident_state_columns), ngd_interp and ngd_sample_interp with and without X_dev
    (test_interp_gpu.test_resident_state), sample_costs and ngd_sample_costs with and without X_dev
    (test_sample_cost_gpu.test_resident_path; that test compares the row minimum of sample_clearance_dev only).  They are
    cheap at T = 2, so every pair is run here."""
    import torch
    ch = planar_chain()
    T, n, Q, S = ch["T"], ch["n"], 3, 9
    ctx, ids = planar()
    K1 = len(ch["specs"][1]["start"])
    nodes = np.array([1, 0, 1], dtype=np.int32)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")   # noqa: E731
    # host variants
    X, Cc, mean, cov = np.empty((S, T, n)), np.empty((3, T, n, n)), np.empty((Q, n)), np.empty((Q, n, n))
    Xi, Xq, Xq2 = np.empty((S, T, n)), np.empty((S, Q, n)), np.empty((S, Q, n))
    clr, J = np.empty((S, K1)), np.empty(S)
    Xc, Jc, lc, cc, Jc2, lc2, cc2 = np.empty((S, T, n)), np.empty(S), np.empty(S), np.empty(S), np.empty(S), np.empty(S), np.empty(S)
    run(ctx, "gvi_ngd_sample", S, 3, 1, X)
    run(ctx, "gvi_ngd_cov_columns", 3, nodes, Cc)
    run(ctx, "gvi_ngd_interp", mean, cov)
    run(ctx, "gvi_ngd_sample_interp", S, 3, 4, 1, Xi, Xq)
    run(ctx, "gvi_ngd_sample_interp", S, 3, 4, 1, None, Xq2)
    run(ctx, "gvi_sample_clearance", ids[1], S, X, clr)
    run(ctx, "gvi_sample_costs", S, X, J)
    run(ctx, "gvi_ngd_sample_costs", S, 3, 1, ids[1], Xc, Jc, lc, cc)
    run(ctx, "gvi_ngd_sample_costs", S, 3, 1, ids[1], None, Jc2, lc2, cc2)
    assert np.array_equal(Xi, X) and np.array_equal(Xc, X) and np.array_equal(Xq2, Xq)
    assert np.array_equal(Jc2, Jc) and np.array_equal(lc2, lc) and np.array_equal(cc2, cc)
    for a in (X, Cc, mean, cov, Xq, clr, J, Jc, lc, cc):
        assert np.isfinite(a).all()
    # _dev variants into NaN-filled torch buffers
    dX, dC, dm, dc = nan(S, T, n), nan(3, T, n, n), nan(Q, n), nan(Q, n, n)
    dXi, dXq, dXq2, dclr, dJ = nan(S, T, n), nan(S, Q, n), nan(S, Q, n), nan(S, K1), nan(S)
    dXc, dJc, dlc, dcc, dJc2, dlc2, dcc2 = nan(S, T, n), nan(S), nan(S), nan(S), nan(S), nan(S), nan(S)
    dXin = torch.from_numpy(X).to("cuda:0")
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()   # noqa: E731
    run(ctx, "gvi_ngd_sample_dev", S, 3, 1, p(dX))
    run(ctx, "gvi_ngd_cov_columns_dev", 3, nodes, p(dC))
    run(ctx, "gvi_ngd_interp_dev", p(dm), p(dc))
    run(ctx, "gvi_ngd_sample_interp_dev", S, 3, 4, 1, p(dXi), p(dXq))
    run(ctx, "gvi_ngd_sample_interp_dev", S, 3, 4, 1, None, p(dXq2))
    run(ctx, "gvi_sample_clearance_dev", ids[1], S, p(dXin), p(dclr))
    run(ctx, "gvi_sample_costs_dev", S, p(dXin), p(dJ))
    run(ctx, "gvi_ngd_sample_costs_dev", S, 3, 1, ids[1], p(dXc), p(dJc), p(dlc), p(dcc))
    run(ctx, "gvi_ngd_sample_costs_dev", S, 3, 1, ids[1], None, p(dJc2), p(dlc2), p(dcc2))
    run(ctx, "gvi_ctx_sync")
    pairs = dict(X=(X, dX), C=(Cc, dC), mean=(mean, dm), cov=(cov, dc), Xi=(X, dXi), Xq=(Xq, dXq), Xq2=(Xq, dXq2), clr=(clr, dclr),
                 J=(J, dJ), Xc=(X, dXc), Jc=(Jc, dJc), lc=(lc, dlc), cc=(cc, dcc), Jc2=(Jc, dJc2), lc2=(lc, dlc2), cc2=(cc, dcc2))
    for k, (a, d) in pairs.items():
        assert np.array_equal(a, d.cpu().numpy()), k
    ctx.close()
