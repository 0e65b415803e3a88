"""Timing of the limit factors (GVI_PSI_HINGE_BOX).

    python tools/box_bench.py [--reps 30] [--out profiles/box_bench.json]

(a) The moments launch of one box set of K = 1025 factors, d = 4 and d = 14, on the closed-form kernel
    (moments_box_closed_kernel) and on the quadrature route at p = 3 (PsiBoxHinge<4> register instance; d = 14: the generic
    kernel): the bracket gvi_profile_last reports -- HIP events on the context stream around the launch of set 0, read after a
    synchronise -- the two routes alternating, median and spread of --reps after three warm-up rounds.
(b) One iteration of the planar1k graph without and with a velocity-limit set (closed form) on every state, same build: every
    timed iteration is the FIRST iteration from the start state (gvi_ngd_init outside the bracket, HIP events around the
    synchronising gvi_ngd_step), the trials of every round recorded; gvi_ngd_gradients and one gvi_ngd_trial from the start
    state on their own as well, since an iteration's time grows with its line-search trials.  The difference of the two graphs
    is the price of the set.
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

INF = np.inf


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=round(float(np.median(ts)), 2), min_us=round(float(ts.min()), 2), max_us=round(float(ts.max()), 2),
                spread_us=round(float(ts.max() - ts.min()), 2))


def box_case(d, K):
    """Limits +-1 on every coordinate, means spread from well inside to past the limits."""
    rng = np.random.default_rng(50 + d)
    mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
    mu = rng.uniform(-1.3, 1.3, size=(K, d))
    return np.tile(syn.box_params(5.0, 0.1, np.full(d, -1.0), np.full(d, 1.0)), (K, 1)), mu, Sigma


def moments_bracket(stream, d, K, p, reps):
    params, mu, Sigma = box_case(d, K)
    ctx = api.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.chain_set(1, d)
    sid = ctx.factors_add(d, p, np.zeros(K, dtype=np.int32), api.PSI_HINGE_BOX, params)
    ctx.profile_enable(True)
    out, geo = {"closed": [], "quadrature": []}, {}
    for it in range(3 + reps):
        for route, on in (("closed", 1), ("quadrature", 0)):
            ctx.factors_set_closed_form(sid, on)
            ctx.moments(sid, mu, Sigma)                          # synchronises: the results come back to the host
            geo[route] = ctx.profile_geometry(sid)
            if it >= 3:
                out[route].append(ctx.profile_last(sid, 0) * 1e3)
    ctx.close()
    return out, geo


def step_times(stream, ch, reps):
    ctx, ids = api.context_for_chain(ch)
    ctx.set_stream(stream.cuda_stream)
    ts, trials, tg, tt = [], [], [], []
    for it in range(3 + reps):
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = ctx.ngd_step(0.55, 10)
        e1.record(stream)
        torch.cuda.synchronize()
        if it >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3)
            trials.append(r["ntrials"] if r["accepted"] else -r["ntrials"])
    geo = [ctx.profile_geometry(sid)["variant"] for sid in ids]
    for it in range(3 + reps):
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(stream)
        ctx.ngd_gradients()
        ev[1].record(stream)
        torch.cuda.synchronize()
        ev[2].record(stream)
        ctx.ngd_trial(0.55 * 0.75)
        ev[3].record(stream)
        torch.cuda.synchronize()
        if it >= 3:
            tg.append(ev[0].elapsed_time(ev[1]) * 1e3)
            tt.append(ev[2].elapsed_time(ev[3]) * 1e3)
    ctx.close()
    return ts, trials, geo, tg, tt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--K", type=int, default=1025)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("box_bench needs the GPU: nothing is timed without one")
    stream = torch.cuda.Stream()
    rows_a = []
    for d in (4, 14):
        ts, geo = moments_bracket(stream, d, args.K, 3, args.reps)
        c, q = stats(ts["closed"]), stats(ts["quadrature"])
        row = dict(part="a", d=d, p=3, K=args.K, N=api.spgh_count(d, 3), closed=c, quadrature=q,
                   quadrature_kernel=geo["quadrature"]["variant"], quadrature_chunks=geo["quadrature"]["nchunk"],
                   ratio=round(q["median_us"] / c["median_us"], 2))
        print(json.dumps(row), flush=True)
        rows_a.append(row)
    rows_b = []
    base = syn.make_chain("planar1k")
    # the start trajectory moves at (6 / 256, 0.8 / 256); limits that its jittered speeds touch
    v = np.abs(base["mu0"][:, 2:]).max(axis=0)
    limited = syn.add_box_set(base, [-INF, -INF, -0.9 * v[0], -0.9 * v[1]], [INF, INF, 0.9 * v[0], 0.9 * v[1]], sigma=50.0, eps=0.0, p=3,
                              temperature=30.0)
    for tag, ch in (("planar1k", base), ("planar1k + velocity limits", limited)):
        ts, trials, geo, tg, tt = step_times(stream, ch, args.reps)
        row = dict(part="b", graph=tag, T=int(ch["T"]), sets=[dict(kind=int(s["kind"]), d=int(s["d"]), K=int(len(s["start"]))) for s in ch["specs"]],
                   kernels=geo, step=stats(ts), trials=trials, gradients=stats(tg), one_trial=stats(tt))
        print(json.dumps(row), flush=True)
        rows_b.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(reps=args.reps, moments_launch=rows_a, ngd_step=rows_b), f, indent=1)


if __name__ == "__main__":
    main()
