"""Timing of the moving-ball obstacle factors.

    python tools/balls_bench.py [--reps 30] [--out profiles/balls_bench.json]

(a) The moments launch of one ball set on its register instance (PsiHingeBalls) and on the generic kernel, the route the set
    would take without the policy (gvi_set_variant(1)): the bracket gvi_profile_last reports -- HIP events on the context
    stream around the launch of set 0, read after a synchronise -- for every registered instance, the two routes alternating,
    median and spread of --reps.  1024 factors, J = 3 check points, 3 live balls, random read-outs; the balls stand where about
    a third of the sigma points fall inside a hinge.  "keep" is the rule of section 14: the instance stays only if the medians
    differ by more than the larger of the two spreads (max - min).
(b) The same STATIC scene twice on 1024 factors of d = 8 at J = 3: as HINGE_SDF_2D_SEG on a rasterised grid (four gathers per
    check point, whatever the number of obstacles) and as HINGE_BALLS_2D with v = 0 (no memory look-up, work per live ball), at
    1, 3 and 8 balls, each on its register instance.  The two are not the same function -- the grid is bilinear on 0.1 cells --
    so only the times are compared; E[psi] of both is recorded beside them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussianvi_amd import api, synthetic as syn  # noqa: E402

INSTANCES = [(2, 2, 4), (2, 4, 4), (2, 8, 3), (2, 12, 3), (3, 3, 4), (3, 6, 4), (3, 12, 3)]      # (P, d, GH degree)
KIND = {2: api.PSI_HINGE_BALLS_2D, 3: api.PSI_HINGE_BALLS_3D}
ORIGIN, CELL, ROWS, COLS = (-5.0, -4.0), 0.1, 81, 101


def scene(M, P, rng):
    """M static balls inside the grid's extent (the first P coordinates of it)."""
    lo = np.array([-3.5, -2.5, -2.5][:P])
    return rng.uniform(lo, -lo, (M, P)), rng.uniform(0.4, 0.9, M)


def readouts(rng, P, d, J, K):
    W = 0.05 * rng.normal(size=(K, J, P, d))
    W[:, :, np.arange(P), np.arange(P)] += 1.0
    return W, 0.3 * rng.normal(size=(K, J, P))


def balls_case(P, d, J, K, M, p, velocities=True):
    rng = np.random.default_rng(100 * P + d + 7 * M)
    W, c = readouts(rng, P, d, J, K)
    centres, radii = scene(M, P, rng)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
    near = centres[rng.integers(0, M, K)]
    mu[:, :P] = near + rng.normal(size=(K, P)) * 0.8                # poses around the balls: both hinge branches
    vel = rng.uniform(-1.0, 1.0, (M, P)) if velocities else np.zeros((M, P))
    tau = rng.uniform(-0.1, 0.1, (K, J)) if velocities else np.zeros((K, J))
    spec = dict(kind=KIND[P], d=d, p=p, start=np.zeros(K, dtype=np.int32), temperature=np.ones(K),
                params=syn.balls_params(15.5, 0.5, 0.3, W, c, tau, centres, vel, radii))
    return spec, mu, Sigma, (W, c, centres, radii)


def moments_bracket(stream, spec, n, mu, Sigma, reps, routes):
    """{route: [us] * reps} of the moments launch of the one-set context, the routes alternating."""
    ctx = api.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.chain_set(2 if spec["d"] == 2 * n else 1, n)
    sid = ctx.factors_add(spec["d"], spec["p"], spec["start"], spec["kind"], spec["params"], spec["temperature"])
    if "sdf_field" in spec:
        ctx.factors_set_sdf2d(sid, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    ctx.profile_enable(True)
    out = {k: [] for k in routes}
    geo, res = {}, {}
    for it in range(3 + reps):
        for k, v in routes.items():
            ctx.set_variant(v)
            res[k] = ctx.moments(sid, mu, Sigma)                # synchronises: the results come back to the host
            geo[k] = ctx.profile_geometry(sid)
            if it >= 3:
                out[k].append(ctx.profile_last(sid, 0) * 1e3)
    ctx.close()
    return out, geo, res


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=round(float(np.median(ts)), 2), min_us=round(float(ts.min()), 2), max_us=round(float(ts.max()), 2),
                spread_us=round(float(ts.max() - ts.min()), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("balls_bench needs the GPU: nothing is timed without one")
    stream = torch.cuda.Stream()
    K, J = args.K, 3
    rows_a = []
    for P, d, p in INSTANCES:
        spec, mu, Sigma, _ = balls_case(P, d, J, K, 3, p)
        n = d // 2 if d in (8, 12) else d
        ts, geo, res = moments_bracket(stream, spec, n, mu, Sigma, args.reps, {"register": 0, "generic": 1})
        assert geo["register"]["variant"] == 2 and geo["generic"]["variant"] == 1, geo
        gap = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) for a, b in zip(res["register"], res["generic"]))
        reg, gen = stats(ts["register"]), stats(ts["generic"])
        gain = gen["median_us"] - reg["median_us"]
        row = dict(part="a", kind=int(spec["kind"]), d=d, p=p, J=J, K=K, balls=3, N=api.spgh_count(d, p), register=reg, generic=gen,
                   register_chunks=geo["register"]["nchunk"], generic_chunks=geo["generic"]["nchunk"],
                   speedup=round(gen["median_us"] / reg["median_us"], 2), routes_agree_rel=float(gap),
                   share_Ephi_positive=float((res["register"][0] > 0).mean()), keep=bool(gain > max(reg["spread_us"], gen["spread_us"])))
        print(json.dumps(row), flush=True)
        rows_a.append(row)
    rows_b = []
    for M in (1, 3, 8):
        spec, mu, Sigma, (W, c, centres, radii) = balls_case(2, 8, J, K, M, 3, velocities=False)
        grid = dict(kind=api.PSI_HINGE_SDF_2D_SEG, d=8, p=3, start=spec["start"], temperature=spec["temperature"],
                    params=syn.segment_params(15.5, 0.5, 0.3, W, c), sdf_origin=ORIGIN, sdf_cell=CELL,
                    sdf_field=syn.circle_sdf(ORIGIN, CELL, ROWS, COLS, [tuple(x) for x in centres], list(radii)))
        tb, gb, rb = moments_bracket(stream, spec, 4, mu, Sigma, args.reps, {"register": 0})
        tg, gg, rg = moments_bracket(stream, grid, 4, mu, Sigma, args.reps, {"register": 0})
        assert gb["register"]["variant"] == 2 and gg["register"]["variant"] == 2, (gb, gg)
        a, g = stats(tb["register"]), stats(tg["register"])
        row = dict(part="b", d=8, p=3, J=J, K=K, balls=M, N=api.spgh_count(8, 3), analytic=a, grid=g,
                   analytic_over_grid=round(a["median_us"] / g["median_us"], 3), Ephi_sum_analytic=float(rb["register"][0].sum()),
                   Ephi_sum_grid=float(rg["register"][0].sum()),
                   analytic_faster=bool(g["median_us"] - a["median_us"] > max(a["spread_us"], g["spread_us"])))
        print(json.dumps(row), flush=True)
        rows_b.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(reps=args.reps, moments_launch=rows_a, analytic_against_grid=rows_b), f, indent=1)


if __name__ == "__main__":
    main()
