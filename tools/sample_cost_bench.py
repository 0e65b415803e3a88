"""Timing of the costs of sampled trajectories: gvi_ngd_sample_costs_dev with X = NULL on the initial
states of the C3 and planar1k chains.

    python tools/sample_cost_bench.py [--configs c3,planar1k] [--S 1,64,1024] [--reps 30] [--out profiles/sample_cost_bench.json]

Per (config, S), from HIP events on the context stream around synchronised work (median of --reps):
    whole_us     the resident call with log q and the minimum clearance (planar1k: of the obstacle set)
    sampler_us   gvi_ngd_sample_dev alone -- the factorisation launches and the sweep of section 10
    cost_us      gvi_sample_costs_dev on those samples -- the launch over every set and the ordered reduction
    logq_us      whole - (the same call without log q)
The one bound that can be derived for the cost launch: reading X once, S T n 8 bytes at 6.1 TB/s (the rate section 10 uses).
Run it a second time under `rocprofv3 --kernel-trace --stats -- python tools/sample_cost_bench.py` for the per-kernel split
(its own run: no counters together with tracing).
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

READ_TBS = 6.1


def timed(stream, fn, reps):
    ts = []
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,planar1k")
    ap.add_argument("--S", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_cost_bench.json"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()            # a stream of its own: the events and the library's launches share it
    rows = []
    for name in args.configs.split(","):
        ch = syn.make_chain(name)
        T, n = ch["T"], ch["n"]
        ctx, ids = api.context_for_chain(ch)
        ctx.set_stream(stream.cuda_stream)
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        hinge = [i for i, sp in zip(ids, ch["specs"]) if sp["kind"] >= syn.PSI_HINGE_SDF_2D]
        cset = hinge[0] if hinge else -1
        K = sum(len(sp["start"]) for sp in ch["specs"])
        for S in (int(s) for s in args.S.split(",")):
            new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda:0")   # noqa: E731
            X, J, lq, cm = new(S, T, n), new(S), new(S), new(S)
            cptr = cm.data_ptr() if cset >= 0 else None
            whole = timed(stream, lambda: ctx.ngd_sample_costs_dev(S, J.data_ptr(), seed=1, clearance_set=cset, logq_ptr=lq.data_ptr(),
                                                                   clr_min_ptr=cptr), args.reps)
            nolq = timed(stream, lambda: ctx.ngd_sample_costs_dev(S, J.data_ptr(), seed=1, clearance_set=cset, clr_min_ptr=cptr),
                         args.reps)
            smp = timed(stream, lambda: ctx.ngd_sample_dev(S, X.data_ptr(), seed=1), args.reps)
            cost = timed(stream, lambda: ctx.sample_costs_dev(S, X.data_ptr(), J.data_ptr()), args.reps)
            bound = S * T * n * 8 / (READ_TBS * 1e12) * 1e6
            row = dict(config=name, T=T, n=n, factors=K, S=S, whole_us=round(whole, 2), sampler_us=round(smp, 2), cost_us=round(cost, 2),
                       logq_us=round(whole - nolq, 2), read_bound_us=round(bound, 3), cost_read_share=round(bound / cost, 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
