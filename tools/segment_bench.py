"""Timing of the obstacle factors on a segment.

    python tools/segment_bench.py [--reps 30] [--out profiles/segment_bench.json]

(a) The moments launch of one segment set on its register instance (PsiHingeSeg) and on the generic kernel, the route the set
    would take without the policy (gvi_set_variant(1)): the bracket gvi_profile_last reports -- HIP events on the context
    stream around the launch of set 0, read after a synchronise -- for every instance, the two routes alternating, median and
    spread of --reps.  The d = 8 row is the segment set of a planar1k-shaped graph (T = 1025, n = 4, J = 3) at its start
    marginals; the other rows are 1024 factors with random read-outs around poses spread over the grid.  "keep" is the rule of
    section 14: the instance stays only if the medians differ by more than the larger of the two spreads (max - min).
(b) gvi_ngd_step per iteration on two graphs of the same horizon: T = 1025 with a J = 3 segment set, and T = 4097 with unary
    obstacle factors only (support states at every check time).  Every timed iteration is the FIRST iteration from the start
    state: gvi_ngd_init outside the bracket, then HIP events around the synchronising gvi_ngd_step; median of --reps after
    three warm-up rounds.  An iteration's time grows with its line-search trials, so the trials of every round are recorded
    (negative: the line search was exhausted) and the two graphs are comparable only where they agree; gvi_ngd_gradients and
    one gvi_ngd_trial from the same start state are therefore timed on their own as well (iteration = gradients + k trials).
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

DT = 0.25
TAUS = [DT / 4, DT / 2, 3 * DT / 4]


def planar_segment_case(T, p):
    """(spec, mu_k, Sigma_k): the segment set of the planar graph and its marginals at the start state."""
    ch = syn.make_planar_chain(T=T, p=3, p_obstacle=7, segment_taus=TAUS, segment_p=p)
    seg = ch["specs"][2]
    ctx = api.Context(0)
    ctx.chain_set(ch["T"], ch["n"])
    sid = ctx.factors_add(seg["d"], seg["p"], seg["start"], seg["kind"], seg["params"], seg["temperature"])
    SD, SU = ctx.bt_marginals(ch["D0"], ch["U0"])
    mk, Sk = ctx.gather_marginals(sid, ch["mu0"], SD, SU)
    ctx.close()
    return seg, mk, Sk


def random_case(P, d, J, K, p, field):
    """K factors of dimension d with J read-outs near [I_P 0] around poses spread over the grid."""
    rng = np.random.default_rng(100 * P + d)
    W = 0.05 * rng.normal(size=(K, J, P, d))
    W[:, :, np.arange(P), np.arange(P)] += 1.0
    c = 0.3 * rng.normal(size=(K, J, P))
    mu, Sigma = syn.random_marginals(rng, K, d, 0.05)
    lo = np.asarray(field["sdf_origin"])
    hi = lo + field["sdf_cell"] * (np.array(field["sdf_field"].shape)[[1, 0, 2][:P]] - 1)
    mu[:, :P] = rng.uniform(lo, hi, size=(K, P))
    spec = dict(kind=api.PSI_HINGE_SDF_2D_SEG if P == 2 else api.PSI_HINGE_SDF_3D_SEG, d=d, p=p, start=np.zeros(K, dtype=np.int32),
                params=syn.segment_params(15.5, 0.5, 0.3, W, c), temperature=np.ones(K), **field)
    return spec, mu, Sigma


def moments_bracket(stream, spec, n, mu, Sigma, reps):
    """{route: [us] * reps} of the moments launch of the one-set context, the register and the generic route alternating."""
    ctx = api.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.chain_set(2 if spec["d"] == 2 * n else 1, n)
    start = np.zeros(len(spec["start"]), dtype=np.int32)
    sid = ctx.factors_add(spec["d"], spec["p"], start, spec["kind"], spec["params"], spec["temperature"])
    setter = ctx.factors_set_sdf2d if spec["kind"] == api.PSI_HINGE_SDF_2D_SEG else ctx.factors_set_sdf3d
    setter(sid, spec["sdf_origin"], spec["sdf_cell"], spec["sdf_field"])
    ctx.profile_enable(True)
    routes = {"register": 0, "generic": 1}
    out = {k: [] for k in routes}
    geo, res = {}, {}
    for it in range(3 + reps):
        for k, v in routes.items():
            ctx.set_variant(v)
            res[k] = ctx.moments(sid, mu, Sigma)                # synchronises: the results come back to the host
            geo[k] = ctx.profile_geometry(sid)
            if it >= 3:
                out[k].append(ctx.profile_last(sid, 0) * 1e3)
    assert geo["register"]["variant"] == 2 and geo["generic"]["variant"] == 1, geo
    gap = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) for a, b in zip(res["register"], res["generic"]))
    ctx.close()
    return out, geo, float(gap)


def step_times(stream, ch, reps):
    ctx, ids = api.context_for_chain(ch)
    ctx.set_stream(stream.cuda_stream)
    ts, trials = [], []
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
    cost = ctx.ngd_cost()
    # the two halves of an iteration on their own, from the same start state: the gradients (factor pass of every set,
    # assemble, solve) and ONE line-search trial (chain factorisation and marginals at the trial point, cost pass)
    tg, tt = [], []
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
    return ts, trials, geo, cost, tg, tt


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=round(float(np.median(ts)), 2), min_us=round(float(ts.min()), 2), max_us=round(float(ts.max()), 2),
                spread_us=round(float(ts.max() - ts.min()), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--T", type=int, default=1025)
    ap.add_argument("--segment-p", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench needs the GPU: nothing is timed without one")
    stream = torch.cuda.Stream()
    K = args.T - 1
    planar = syn.make_planar_chain(T=3)["specs"][1]
    field2 = {k: planar[k] for k in ("sdf_origin", "sdf_cell", "sdf_field")}
    pr3d = syn.make_obstacle_chain("pr3d", T=3)["specs"][1]
    field3 = {k: pr3d[k] for k in ("sdf_origin", "sdf_cell", "sdf_field")}
    cases = [("planar segment set", 4) + planar_segment_case(args.T, args.segment_p),
             ("random read-outs", 4) + random_case(2, 4, 3, K, 4, field2),
             ("random read-outs", 6) + random_case(2, 12, 3, K, 3, field2),
             ("random read-outs", 6) + random_case(3, 6, 3, K, 4, field3)]
    rows_a = []
    for what, n, spec, mu, Sigma in cases:
        ts, geo, gap = moments_bracket(stream, spec, n, mu, Sigma, args.reps)
        reg, gen = stats(ts["register"]), stats(ts["generic"])
        gain = gen["median_us"] - reg["median_us"]
        row = dict(part="a", input=what, kind=int(spec["kind"]), d=int(spec["d"]), p=int(spec["p"]), J=3, K=int(len(spec["start"])),
                   N=api.spgh_count(spec["d"], spec["p"]), register=reg, generic=gen, register_chunks=geo["register"]["nchunk"],
                   generic_chunks=geo["generic"]["nchunk"], speedup=round(gen["median_us"] / reg["median_us"], 2),
                   routes_agree_rel=gap, keep=bool(gain > max(reg["spread_us"], gen["spread_us"])))
        print(json.dumps(row), flush=True)
        rows_a.append(row)
    rows_b = []
    horizon = (args.T - 1) * DT
    A = syn.make_planar_chain(T=args.T, p=3, p_obstacle=7, segment_taus=TAUS, segment_p=args.segment_p)
    B = syn.make_planar_chain(T=4 * (args.T - 1) + 1, p=3, p_obstacle=7, horizon=horizon)
    for tag, ch in (("segment set, J = 3", A), ("support states at every check time", B)):
        for spec in ch["specs"][1:-1]:                           # the planning benchmark's high temperature (make_chain, planar1k)
            spec["temperature"] = np.full(len(spec["start"]), 30.0)
        ts, trials, geo, cost, tg, tt = step_times(stream, ch, args.reps)
        row = dict(part="b", graph=tag, T=int(ch["T"]), n=int(ch["n"]), sets=[dict(kind=int(s["kind"]), d=int(s["d"]), p=int(s["p"]),
                   K=int(len(s["start"]))) for s in ch["specs"]], kernels=geo, step=stats(ts), trials=trials, cost_after=cost,
                   gradients=stats(tg), one_trial=stats(tt))
        print(json.dumps(row), flush=True)
        rows_b.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(reps=args.reps, moments_launch=rows_a, ngd_step=rows_b), f, indent=1)


if __name__ == "__main__":
    main()
