"""Timing and accuracy of the read-out-space rule (gvi_factors_set_readout_rule).

    python tools/readout_bench.py [--reps 30] [--out profiles/readout_bench.json] [--parts abc] [--parent-tree DIR]

(a) The moments launch of one set on its current route (order 0: the register instance of its sparse rule) and on the read-out
    route at orders 8 and 12 (P = 2) or 4 and 6 (P = 3): the bracket gvi_profile_last reports -- HIP events on the context stream
    around the launch of set 0, read after a synchronise --, the routes alternating, median and spread of --reps.  1024 factors,
    J = 3 check points.  The rows are the instances of section 17's table (a) (analytic balls, 3 live) and of section 14 (grid
    kinds on a segment).
(b) The kink: HINGE_SDF_2D, d = 4, on a grid holding a plane whose hinge boundary passes through every mean.  E[psi] and Vdmu of
    each route against the exact values from Phi and phi.
(c) With --parent-tree: bench.py (default config and --config planar1k) of this tree and of a checkout of the parent commit
    with its library built, three runs each, alternating.  Neither config reaches the new code.
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussianvi_amd import api, synthetic as syn  # noqa: E402
import balls_bench as bb  # noqa: E402

BALLS = [(2, 2, 4), (2, 4, 4), (2, 8, 3), (2, 12, 3), (3, 3, 4), (3, 6, 4), (3, 12, 3)]      # (P, d, GH degree): section 17 (a)
SEGS = [(2, 4, 4), (2, 8, 3), (2, 12, 3), (3, 6, 4)]                                          # section 14's instances
ORDERS = {2: (8, 12), 3: (4, 6)}
ORIGIN3, CELL3 = (-4.0, -3.0, -2.0), 0.2


def seg_case(P, d, J, K, p):
    rng = np.random.default_rng(200 * P + d)
    W, c = bb.readouts(rng, P, d, J, K)
    centres, radii = bb.scene(3, P, rng)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
    mu[:, :P] = centres[rng.integers(0, 3, K)] + rng.normal(size=(K, P)) * 0.8
    spec = dict(kind=api.PSI_HINGE_SDF_2D_SEG if P == 2 else api.PSI_HINGE_SDF_3D_SEG, d=d, p=p, start=np.zeros(K, dtype=np.int32),
                temperature=np.ones(K), params=syn.segment_params(15.5, 0.5, 0.3, W, c))
    if P == 2:
        spec.update(sdf_origin=bb.ORIGIN, sdf_cell=bb.CELL, sdf_field=syn.circle_sdf(bb.ORIGIN, bb.CELL, bb.ROWS, bb.COLS, [tuple(x) for x in centres], list(radii)))
    else:
        spec.update(sdf_origin=ORIGIN3, sdf_cell=CELL3, sdf_field=syn.sphere_sdf3d(ORIGIN3, CELL3, 31, 41, 21, [tuple(x) for x in centres], list(radii)))
    return spec, mu, Sigma


def load(stream, spec, n):
    ctx = api.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.chain_set(2 if spec["d"] == 2 * n else 1, n)
    sid = ctx.factors_add(spec["d"], spec["p"], spec["start"], spec["kind"], spec["params"], spec["temperature"])
    if "sdf_field" in spec:
        (ctx.factors_set_sdf2d if np.ndim(spec["sdf_field"]) == 2 else ctx.factors_set_sdf3d)(sid, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    return ctx, sid


def brackets(stream, spec, n, mu, Sigma, reps, orders):
    """{order: [us] * reps} of the moments launch, the orders alternating (0: the set's sparse route)."""
    ctx, sid = load(stream, spec, n)
    ctx.profile_enable(True)
    out, geo, res = {q: [] for q in orders}, {}, {}
    for it in range(3 + reps):
        for q in orders:
            ctx.factors_set_readout_rule(sid, q)
            res[q] = ctx.moments(sid, mu, Sigma)
            geo[q] = ctx.profile_geometry(sid)["variant"]
            if it >= 3:
                out[q].append(ctx.profile_last(sid, 0) * 1e3)
    ctx.close()
    return out, geo, res


def part_a(stream, reps, K):
    rows = []
    for family, shapes in (("balls", BALLS), ("segment", SEGS)):
        for P, d, p in shapes:
            if family == "balls":
                spec, mu, Sigma, _ = bb.balls_case(P, d, 3, K, 3, p)
            else:
                spec, mu, Sigma = seg_case(P, d, 3, K, p)
            n = d // 2 if d in (8, 12) else d
            orders = (0,) + ORDERS[P]
            ts, geo, res = brackets(stream, spec, n, mu, Sigma, reps, orders)
            assert geo[0] == 2 and all(geo[q] == 8 for q in ORDERS[P]), geo
            st = {q: bb.stats(ts[q]) for q in orders}
            row = dict(part="a", family=family, kind=int(spec["kind"]), d=d, p=p, J=3, K=K, sparse_points=api.spgh_count(d, p), sparse=st[0],
                       Ephi_sum_sparse=float(res[0][0].sum()))
            for q in ORDERS[P]:
                gain = st[0]["median_us"] - st[q]["median_us"]
                row[f"order_{q}"] = dict(st[q], points_per_check_point=q ** P, sparse_over_readout=round(st[0]["median_us"] / st[q]["median_us"], 2),
                                         faster="readout" if gain > max(st[0]["spread_us"], st[q]["spread_us"]) else
                                         "sparse" if -gain > max(st[0]["spread_us"], st[q]["spread_us"]) else "neither",
                                         Ephi_sum=float(res[q][0].sum()))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def part_b(stream):
    """The kink through the mean: relative errors of E[psi] and Vdmu (max-norm over 64 factors) of every route."""
    rng = np.random.default_rng(5)
    d, K, nrm, b0 = 4, 64, np.array([0.6, -0.8]), 0.25
    xs, ys = bb.ORIGIN[0] + np.arange(bb.COLS) * bb.CELL, bb.ORIGIN[1] + np.arange(bb.ROWS) * bb.CELL
    fld = nrm[0] * xs[None, :] + nrm[1] * ys[:, None] + b0
    mu, Sigma = syn.random_marginals(rng, K, d, 0.02)
    mu[:, :2] = rng.uniform(-0.3, 0.3, (K, 2))
    sigma, r = rng.uniform(5.0, 20.0, K), 0.1
    thr = mu[:, :2] @ nrm + b0                                         # the boundary passes through the mean: c = 0
    prm = np.stack([sigma, thr - r, np.full(K, r)], axis=1)
    s = np.sqrt(np.einsum("a,kab,b->k", nrm, Sigma[:, :2, :2], nrm))
    phi0 = 1.0 / math.sqrt(2.0 * math.pi)
    E_exact = sigma * s * s * 0.5                                      # sigma E[max(0, s t)^2]
    V_exact = np.zeros((K, d))
    V_exact[:, :2] = -nrm[None, :] * (sigma * 2.0 * s * phi0)[:, None]  # E[grad psi] = -n sigma E[2 max(0, s t)]
    rows = []
    for p in (3, 4, 5):
        spec = dict(kind=api.PSI_HINGE_SDF_2D, d=d, p=p, start=np.zeros(K, dtype=np.int32), temperature=np.ones(K), params=prm, sdf_origin=bb.ORIGIN,
                    sdf_cell=bb.CELL, sdf_field=fld)
        ctx, sid = load(stream, spec, d)
        for q in (0, 4, 8, 12, 16) if p == 3 else (0,):
            ctx.factors_set_readout_rule(sid, q)
            E, V, _ = ctx.moments(sid, mu, Sigma)
            row = dict(part="b", route=f"sparse p = {p}, {api.spgh_count(d, p)} points" if q == 0 else f"read-out order {q}, {q * q} points",
                       E_phi_rel_err=float(np.abs(E / E_exact - 1).max()), Vdmu_rel_err=float(np.abs(V - V_exact).max() / np.abs(V_exact).max()))
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    return rows


def part_c(parent_root):
    rows = []
    for config in ("c3", "planar1k"):
        ms = {"this": [], "parent": []}
        for rep in range(3):
            for which in ("this", "parent"):
                root = ROOT if which == "this" else parent_root       # a checkout of the parent commit with its library built
                r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", config], cwd=root, capture_output=True, text=True,
                                   timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"bench.py {config} ({which}) failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                ms[which].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        row = dict(part="c", config=config, this_ms_per_step=ms["this"], parent_ms_per_step=ms["parent"],
                   this_median=float(np.median(ms["this"])), parent_median=float(np.median(ms["parent"])))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds part (c)")
    ap.add_argument("--parts", default="abc", help="which parts to measure in this call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("readout_bench needs the GPU: nothing is timed without one")
    stream = torch.cuda.Stream()
    out = dict(reps=args.reps)
    if os.path.exists(args.out or ""):                                # parts measured in an earlier call stay
        with open(args.out) as f:
            out.update(json.load(f))
    if "a" in args.parts:
        out["moments_launch"] = part_a(stream, args.reps, args.K)
    if "b" in args.parts:
        out["kink"] = part_b(stream)
    if "c" in args.parts and args.parent_tree:
        out["bench"] = part_c(os.path.abspath(args.parent_tree))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
