"""Timing of the half-space and corridor limit factors (GVI_PSI_HINGE_HALFSPACE).

    python tools/halfspace_bench.py [--reps 30] [--out profiles/halfspace_bench.json]

The moments launch of one set of K = 1025 factors: the bracket gvi_profile_last reports -- HIP events on the context stream
around the launch of set 0, read after a synchronise -- the routes of a set alternating, median and spread of --reps after three
warm-up rounds.
  (a) half-space sets at (d, J) = (4, 4), (4, 8), (14, 16): the closed-form kernel (moments_halfspace_closed_kernel) and the
      quadrature route at p = 3 (the generic kernel);
  (b) a box of d = 4 (limits +-1 on every coordinate) expressed both ways: a GVI_PSI_HINGE_BOX set on
      moments_box_closed_kernel and a half-space set of the 8 rows +-e_i on moments_halfspace_closed_kernel, each set 0 of a
      context of its own (the bracket is taken around set 0) on the same stream, alternating.
Nothing is gated on these numbers.
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


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=round(float(np.median(ts)), 2), min_us=round(float(ts.min()), 2), max_us=round(float(ts.max()), 2),
                spread_us=round(float(ts.max() - ts.min()), 2))


def halfspace_case(d, J, K):
    """Random normals, every row on, hinges from 2.5 sd outside to 2.5 sd inside the mean."""
    rng = np.random.default_rng(60 + 10 * d + J)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
    A = rng.normal(size=(K, J, d))
    sd = np.sqrt(np.einsum("kja,kab,kjb->kj", A, Sigma, A))
    b = np.einsum("kjd,kd->kj", A, mu) + 0.1 + rng.uniform(-2.5, 2.5, (K, J)) * sd
    return syn.halfspace_params(5.0, 0.1, b, A), mu, Sigma


def routes_bracket(stream, d, K, p, reps, sets, routes, mu, Sigma):
    """sets: [(kind, params)], one context each; routes: [(name, set index, closed_form)] timed in turn."""
    ctxs = []
    for kind, params in sets:
        ctx = api.Context(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.chain_set(1, d)
        ctxs.append((ctx, ctx.factors_add(d, p, np.zeros(K, dtype=np.int32), kind, params)))
        ctx.profile_enable(True)
    out, geo = {name: [] for name, _, _ in routes}, {}
    for it in range(3 + reps):
        for name, si, on in routes:
            ctx, sid = ctxs[si]
            ctx.factors_set_closed_form(sid, on)
            ctx.moments(sid, mu, Sigma)                          # synchronises: the results come back to the host
            geo[name] = ctx.profile_geometry(sid)
            if it >= 3:
                out[name].append(ctx.profile_last(sid, 0) * 1e3)
    for ctx, _ in ctxs:
        ctx.close()
    return out, geo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--K", type=int, default=1025)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("halfspace_bench needs the GPU: nothing is timed without one")
    stream = torch.cuda.Stream()
    K = args.K
    rows_a = []
    for d, J in ((4, 4), (4, 8), (14, 16)):
        params, mu, Sigma = halfspace_case(d, J, K)
        ts, geo = routes_bracket(stream, d, K, 3, args.reps, [(api.PSI_HINGE_HALFSPACE, params)],
                                 [("closed", 0, 1), ("quadrature", 0, 0)], mu, Sigma)
        c, q = stats(ts["closed"]), stats(ts["quadrature"])
        Jp = 1 << (J - 1).bit_length()
        row = dict(part="a", d=d, J=J, p=3, K=K, N=api.spgh_count(d, 3), factors_per_wave=64 // Jp, waves=-(-K // (64 // Jp)), closed=c,
                   quadrature=q, quadrature_kernel=geo["quadrature"]["variant"], quadrature_chunks=geo["quadrature"]["nchunk"],
                   ratio=round(q["median_us"] / c["median_us"], 2))
        print(json.dumps(row), flush=True)
        rows_a.append(row)
    d = 4
    rng = np.random.default_rng(54)
    _, Sigma = syn.random_marginals(rng, K, d, 0.05)
    mu = rng.uniform(-1.3, 1.3, size=(K, d))
    box = np.tile(syn.box_params(5.0, 0.1, np.full(d, -1.0), np.full(d, 1.0)), (K, 1))
    half = np.tile(syn.halfspace_params(5.0, 0.1, 1.0, np.concatenate([np.eye(d), -np.eye(d)])), (K, 1))
    ts, geo = routes_bracket(stream, d, K, 3, args.reps, [(api.PSI_HINGE_BOX, box), (api.PSI_HINGE_HALFSPACE, half)],
                             [("box_closed", 0, 1), ("halfspace_closed", 1, 1)], mu, Sigma)
    bx, hs = stats(ts["box_closed"]), stats(ts["halfspace_closed"])
    row_b = dict(part="b", d=d, K=K, box=dict(kernel="moments_box_closed_kernel", waves=K, **bx),
                 halfspace=dict(kernel="moments_halfspace_closed_kernel", J=2 * d, factors_per_wave=8, waves=-(-K // 8), **hs),
                 us_per_factor=dict(box=round(bx["median_us"] / K, 5), halfspace=round(hs["median_us"] / K, 5)),
                 ratio_box_over_halfspace=round(bx["median_us"] / hs["median_us"], 2))
    print(json.dumps(row_b), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(reps=args.reps, moments_launch=rows_a, box_both_ways=row_b), f, indent=1)


if __name__ == "__main__":
    main()
