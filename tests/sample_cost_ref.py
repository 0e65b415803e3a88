"""Shapes, inputs and references for the costs of sampled trajectories beyond one factor tile, one sample chunk and 256 columns
(kernels_sample_cost.hpp, run_sample_cost in posterior_host.inc).  Read by tests/test_sample_cost_shapes_host.py, which proves
the references and the tables on the CPU, and by tests/test_sample_cost_shapes_gpu.py, which holds the device to them.

  case(name)        one row: a chain (T, n), its factor sets in list order, S and the samples X [S][T][n] (numpy, seeded per row)
  references(name)  per set: the float64 oracle closure over the temperature, the same form in np.longdouble from the public
                    parameters, and the magnitude mag[s, k] the per-entry bound is taken against
  geometry(...)     restatement 1: what run_sample_cost launches for a list of sets and S
  ordered_sum(...)  restatement 2: the order in which sample_cost_reduce_kernel adds a row

Nothing here reads the library."""
import functools
import zlib

import numpy as np

import gvi_oracle as o
from gaussianvi_amd import synthetic as syn
from test_gpu_parity import quad_params
from test_sample_cost_host import clearance_ref, factor_slices

QUAD, FIXED, HINGE = syn.PSI_QUAD_PRIOR, syn.PSI_FIXED_PRIOR, syn.PSI_HINGE_SDF_2D
SUMSQ = (QUAD, FIXED)
# the signed-distance field F2 of tests/test_factor_routes_gpu.py
F2 = dict(origin=(-5.0, -4.0), cell=0.1, field=syn.circle_sdf((-5.0, -4.0), 0.1, 81, 101, [(0.0, 1.6), (-1.0, -2.2)], [1.2, 0.9]))


# ---- restatement 1: the launch geometry of run_sample_cost ----
WAVES, TARGET_BLOCKS, THREADS = 4, 2048, 256
NM_STEPS = (4, 8, 12, 16, 24, 32)


def group(m):
    """P: lanes of one factor's residual rows, the next power of two >= m."""
    P = 1
    while P < m:
        P <<= 1
    return P


def tile(m):
    """F: factors of one workgroup's tile, 4 waves of G = 64 / P factors."""
    return WAVES * (64 // group(m))


def rows_of(kind, d):
    """m: residual rows of a sum-of-squares set (QUAD_PRIOR: the second state's, FIXED_PRIOR: the whole slice's)."""
    return d // 2 if kind == QUAD else d


def geometry(sets, S):
    """sets: [(kind, d, K)] in list order.  -> dict(NM, blocks, sets=[...]) of the ONE launch over them: empty sets are
    dropped from the list; a sum-of-squares set gets ftiles * ceil(S / schunk) blocks, block -> (tile = blk % ftiles,
    chunk = blk // ftiles), and the body of NM or NM / 2 register columns; any other set ceil(K S / 256) blocks."""
    out, nb, dmax = [], 0, 0
    for kind, d, K in sets:
        if K == 0:
            continue
        g = dict(kind=kind, d=d, K=K, boff=nb)
        if kind in SUMSQ:
            m = rows_of(kind, d)
            P, F = group(m), tile(m)
            ft = -(-K // F)
            nsc = max(1, min(S, -(-TARGET_BLOCKS // ft)))
            schunk = -(-S // nsc)
            chunks = -(-S // schunk)
            g.update(m=m, P=P, G=64 // P, F=F, ftiles=ft, schunk=schunk, chunks=chunks, last=S - (chunks - 1) * schunk,
                     blocks=ft * chunks, waves=sorted({(k % F) // (64 // P) for k in range(K)}),
                     last_tile=K - (ft - 1) * F)
            dmax = max(dmax, d)
        else:
            g.update(blocks=-(-K * S // THREADS))
        nb += g["blocks"]
        out.append(g)
    NM = next((w for w in NM_STEPS if dmax <= w), None) if dmax else NM_STEPS[0]
    for g in out:
        if g["kind"] in SUMSQ:
            g["body"] = NM // 2 if NM >= 8 and 2 * g["d"] <= NM else NM
    return dict(NM=NM, blocks=nb, sets=out)


def launches(c):
    """Every launch the tests make for a row: the whole list (sample_costs), then each set alone (sample_factor_costs)."""
    sets = [(sp["kind"], sp["d"], len(sp["start"])) for sp in c["specs"]]
    return [geometry(sets, c["S"])] + [geometry([s], c["S"]) for s in sets if s[2] > 0]


# ---- restatement 2: the order of sample_cost_reduce_kernel ----
def ordered_sum(M):
    """J [S] of rows M [S][Kt]: thread t adds entries t, t + 256, ... in ascending order from 0.0, then the 256 partial sums
    are folded by halving, 128 down to 1.  Plain float64 adds, so this is the device's J bit for bit."""
    M = np.asarray(M, dtype=np.float64)
    S, Kt = M.shape
    steps = max(1, -(-Kt // THREADS))
    pad = np.zeros((S, steps * THREADS))
    pad[:, :Kt] = M
    pad = pad.reshape(S, steps, THREADS)
    red = np.zeros((S, THREADS))
    for i in range(steps):
        red = red + pad[:, i, :]
    w = THREADS // 2
    while w > 0:
        red = red[:, :w] + red[:, w:2 * w]
        w //= 2
    return red[:, 0]


# ---- factor sets ----
def _temperature(rng, K):
    return rng.uniform(0.5, 2.0, K)


def quad_spec(rng, n, start, indefinite=False):
    """Binary QUAD_PRIOR set, parameters of test_gpu_parity.quad_params; indefinite: Qinv symmetric with eigenvalues of both
    signs, as test_orbit_m1_gpu.problem draws it."""
    K = len(start)
    Phi, Qinv = quad_params(rng, K, n)
    if indefinite:
        assert n >= 2
        for k in range(K):
            while True:
                Qh = rng.normal(size=(n, n))
                Q = 0.5 * (Qh + Qh.T)
                ev = np.linalg.eigvalsh(Q)
                if ev.min() < -0.05 and ev.max() > 0.05:
                    break
            Qinv[k] = Q
    return dict(kind=QUAD, d=2 * n, p=3, start=np.asarray(start, dtype=np.int32), temperature=_temperature(rng, K), Phi=Phi, Qinv=Qinv,
                params=np.concatenate([Phi.reshape(K, n * n), Qinv.reshape(K, n * n)], axis=1), psi_batch=o.psi_batch_quad_prior(Phi, Qinv),
                indefinite=indefinite)


def fixed_spec(rng, d, start):
    """FIXED_PRIOR set on slices of d (n: unary, 2n: binary), Kinv = G G^T / d + 0.3 I as test_factor_routes_gpu._problem."""
    K = len(start)
    mu0, Kh = rng.normal(size=(K, d)), rng.normal(size=(K, d, d))
    Kinv = Kh @ np.transpose(Kh, (0, 2, 1)) / d + 0.3 * np.eye(d)
    return dict(kind=FIXED, d=d, p=3, start=np.asarray(start, dtype=np.int32), temperature=_temperature(rng, K), mu0=mu0, Kinv=Kinv,
                params=np.concatenate([mu0, Kinv.reshape(K, d * d)], axis=1), psi_batch=o.psi_batch_fixed_prior(mu0, Kinv),
                indefinite=False)


def hinge_spec(rng, start):
    """HINGE_SDF_2D on the field F2, d = n = 2; (sigma, eps, r) drawn as test_factor_routes_gpu._problem draws them."""
    K = len(start)
    params = np.column_stack([rng.uniform(5, 20, K), rng.uniform(0.2, 0.8, K), rng.uniform(0.1, 0.5, K)])
    return dict(kind=HINGE, d=2, p=3, start=np.asarray(start, dtype=np.int32), temperature=_temperature(rng, K), params=params,
                sdf_origin=F2["origin"], sdf_cell=F2["cell"], sdf_field=F2["field"],
                psi_batch=o.psi_batch_hinge_sdf2d(params, F2["origin"], F2["cell"], F2["field"]), indefinite=False)


def descending_starts(T):
    """T starts T - 1 ... 0 with one repeat and one gap: entry 5 repeats entry 4, so state T - 6 is read by no factor."""
    s = np.arange(T - 1, -1, -1)
    s[5] = s[4]
    return s


# ---- the rows ----
G_N = tuple(range(1, 17))
G_INDEFINITE, G_UNARY_ONLY, G_DESCENDING, G_CLOSED = (2, 5, 9, 16), (3, 7, 13), (4, 12), 6
W_N = (1, 2, 3, 5, 8, 9, 12, 16)
C_ROWS = {"C2_2049": (2, 3, 2049), "C2_5000": (2, 3, 5000), "C6_1025": (6, 34, 1025), "C1_684": (1, 514, 684), "C1_1400": (1, 514, 1400)}
C_EXPECT = {"C2_2049": (2, 1), "C2_5000": (3, 2), "C6_1025": (2, 1), "C1_684": (2, 2), "C1_1400": (3, 2)}   # (schunk, samples of the last chunk)
R_KT = (1, 255, 256, 257, 513)
R_HINGE_K, R_NAN_FACTORS = 300, (7, 290)
P_S = (1, 86, 257)

G_NAMES = [f"G{n}" for n in G_N] + [f"G{n}u" for n in G_UNARY_ONLY] + [f"G{G_CLOSED}cf"]
W_NAMES = [f"W{n}" for n in W_N]
C_NAMES = list(C_ROWS)
R_NAMES = [f"R{kt}" for kt in R_KT] + ["Rhinge"]
P_NAMES = [f"P{s}" for s in P_S]
NAMES = G_NAMES + W_NAMES + C_NAMES + R_NAMES + P_NAMES
SUMSQ_NAMES = G_NAMES + W_NAMES + C_NAMES + [f"R{kt}" for kt in R_KT]      # rows of sum-of-squares sets only


def _g_row(rng, name):
    n = int(name[1:].rstrip("ucf"))
    T = 2 * tile(n) + 2
    if name.endswith("u"):                       # the unary set alone: the full-width body on d = n
        return T, n, 5, [fixed_spec(rng, n, np.arange(T))], False
    specs = [quad_spec(rng, n, np.arange(T - 1), indefinite=n in G_INDEFINITE), fixed_spec(rng, n, np.arange(T))]
    if n in G_DESCENDING and not name.endswith("cf"):
        specs.append(fixed_spec(rng, n, descending_starts(T)))
    return T, n, 5, specs, name.endswith("cf")


def _w_row(rng, name):
    n = int(name[1:])
    K = 2 * tile(2 * n) + 1
    return K + 1, n, 5, [fixed_spec(rng, 2 * n, np.arange(K))], False


def _c_row(rng, name):
    n, T, S = C_ROWS[name]
    specs = [quad_spec(rng, n, np.arange(T - 1))]
    if n > 1:
        specs.append(fixed_spec(rng, n, np.arange(T)))
    return T, n, S, specs, False


def _r_row(rng, name):
    if name == "Rhinge":                         # a prior in front, so that the hinge columns start at 299
        T = R_HINGE_K
        return T, 2, 9, [quad_spec(rng, 2, np.arange(T - 1)), hinge_spec(rng, np.arange(T))], False
    kt = int(name[1:])
    if kt == 1:
        return 1, 1, 5, [fixed_spec(rng, 1, np.arange(1))], False
    if kt == 255:                                # boundary at column 127
        return 128, 1, 5, [quad_spec(rng, 1, np.arange(127)), fixed_spec(rng, 1, np.arange(128))], False
    if kt == 256:                                # the unary set first: boundary at column 129
        return 129, 2, 5, [fixed_spec(rng, 2, np.arange(129)), quad_spec(rng, 2, np.arange(127))], False
    if kt == 257:                                # boundary at column 128
        return 129, 1, 5, [quad_spec(rng, 1, np.arange(128)), fixed_spec(rng, 1, np.arange(129))], False
    assert kt == 513                             # boundaries at columns 199 and 399
    return 200, 2, 5, [quad_spec(rng, 2, np.arange(199)), fixed_spec(rng, 2, np.arange(200)), fixed_spec(rng, 2, 50 + np.arange(114))], False


def _p_row(rng, name):
    """The point body and the list order: a hinge set first, an empty set in the middle, a hinge set last."""
    specs = [hinge_spec(rng, [0, 2, 3]), fixed_spec(rng, 2, np.arange(4)), fixed_spec(rng, 2, np.zeros(0, dtype=np.int32)),
             quad_spec(rng, 2, np.arange(3)), hinge_spec(rng, [1])]
    return 4, 2, int(name[1:]), specs, False


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, T, n, S, specs, closed_form, X): computed once, read-only."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    T, n, S, specs, closed = {"G": _g_row, "W": _w_row, "C": _c_row, "R": _r_row, "P": _p_row}[name[0]](rng, name)
    hinge = any(sp["kind"] == HINGE for sp in specs)
    mu = rng.uniform(-3.0, 3.0, size=(T, n)) if hinge else rng.normal(size=(T, n))      # inside F2 where a hinge set reads it
    X = mu + 0.7 * rng.normal(size=(S, T, n))
    X.setflags(write=False)
    for sp in specs:
        for v in sp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return dict(name=name, T=T, n=n, S=S, specs=specs, closed_form=closed, X=X)


# ---- references ----
def oracle_cost(sp, X, n):
    """[S][K] float64: the oracle's closure at the factor slices over the temperature."""
    if len(sp["start"]) == 0:
        return np.zeros((X.shape[0], 0))
    return (sp["psi_batch"](factor_slices(X, sp, n)) / np.asarray(sp["temperature"])[:, None]).T


def longdouble_cost(sp, X, n):
    """[S][K] np.longdouble: the quadratic form straight from the public parameters."""
    L = np.longdouble
    Xk = factor_slices(X, sp, n).astype(L)                                  # [K][S][d]
    if sp["kind"] == QUAD:
        m = sp["d"] // 2
        R = np.einsum("kij,ksj->ksi", sp["Phi"].astype(L), Xk[:, :, :m]) - Xk[:, :, m:]
        v = np.einsum("ksi,kij,ksj->ks", R, sp["Qinv"].astype(L), R) / L(2)
    else:
        E = Xk - sp["mu0"].astype(L)[:, None, :]
        v = np.einsum("ksi,kij,ksj->ks", E, sp["Kinv"].astype(L), E)
    return (v / sp["temperature"].astype(L)[:, None]).T


def magnitude(sp, X, n):
    """mag [S][K] from public parameters only: (|x1| + |Phi| |x0|)^T |Qinv| (|x1| + |Phi| |x0|) / T_k, and for the fixed
    prior (|x| + |mu0|)^T |Kinv| (|x| + |mu0|) / T_k."""
    Xk = np.abs(factor_slices(X, sp, n))
    if sp["kind"] == QUAD:
        m = sp["d"] // 2
        v = Xk[:, :, m:] + np.einsum("kij,ksj->ksi", np.abs(sp["Phi"]), Xk[:, :, :m])
        Q = np.abs(sp["Qinv"])
    else:
        v = Xk + np.abs(sp["mu0"])[:, None, :]
        Q = np.abs(sp["Kinv"])
    return (np.einsum("ksi,kij,ksj->ks", v, Q, v) / sp["temperature"][:, None]).T


@functools.lru_cache(maxsize=None)
def references(name):
    """Per set of the row: dict(cost [S][K] float64, and for a sum-of-squares set ld [S][K] longdouble and mag [S][K]; for a
    hinge set clr [S][K]).  Computed once, read-only."""
    c = case(name)
    out = []
    for sp in c["specs"]:
        r = dict(cost=oracle_cost(sp, c["X"], c["n"]))
        if len(sp["start"]) and sp["kind"] in SUMSQ:
            r["ld"], r["mag"] = longdouble_cost(sp, c["X"], c["n"]), magnitude(sp, c["X"], c["n"])
        if len(sp["start"]) and sp["kind"] == HINGE:
            r["clr"] = clearance_ref(sp, factor_slices(c["X"], sp, c["n"])).T
        for v in r.values():
            v.setflags(write=False)
        out.append(r)
    return out


def windows(name):
    """Three windows [a, b) of at most 64 samples of a C row: the first chunk, one straddling a chunk boundary, and one ending
    at S, so that it holds the last chunk."""
    c = case(name)
    schunk = max(g["schunk"] for g in geometry([(sp["kind"], sp["d"], len(sp["start"])) for sp in c["specs"]], c["S"])["sets"])
    mid = (c["S"] // (2 * schunk)) * schunk
    return [(0, schunk), (mid - 1, mid + 1 + schunk), (c["S"] - 2 * schunk - c["S"] % schunk, c["S"])]
