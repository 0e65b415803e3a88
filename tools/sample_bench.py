"""Timing of the samplers: gvi_ngd_sample_dev on the initial states of the C3, c5 and planar1k chains.

    python tools/sample_bench.py [--configs c3,c5,planar1k] [--S 1,64,1024] [--reps 30] [--out profiles/sample_bench.json]

Per (config, S): the device time of the whole call (factorisation + sweep), and of the factorisation alone (the same call
with the sweep switched off through gvi_set_option("sample_sweep", 0)), from HIP events on the context stream around
synchronised work (median of --reps); the sweep is the difference.  Store bound: S T n 8 bytes at 6.1 TB/s (plain stores,
MI355X_MICROARCH.md).  Run it a second time under `rocprofv3 --kernel-trace --stats -- python tools/sample_bench.py` for
the per-kernel split (its own run: no counters together with tracing).
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

STORE_TBS = 6.1


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
    ap.add_argument("--configs", default="c3,c5,planar1k")
    ap.add_argument("--S", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.Stream()            # a stream of its own: the events and the library's launches share it
    rows = []
    for name in args.configs.split(","):
        ch = syn.make_chain(name)
        T, n = ch["T"], ch["n"]
        ctx = api.Context(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.chain_set(T, n)                 # the state alone: sampling reads (mu, D, U), not the factors
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        for S in (int(s) for s in args.S.split(",")):
            buf = torch.empty((S, T, n), dtype=torch.float64, device="cuda:0")
            ctx.set_option("sample_sweep", 1)
            whole = timed(stream, lambda: ctx.ngd_sample_dev(S, buf.data_ptr(), seed=1), args.reps)
            ctx.set_option("sample_sweep", 0)
            fac = timed(stream, lambda: ctx.ngd_sample_dev(S, buf.data_ptr(), seed=1), args.reps)
            ctx.set_option("sample_sweep", 1)
            sweep = whole - fac
            bound = S * T * n * 8 / (STORE_TBS * 1e12) * 1e6
            row = dict(config=name, T=T, n=n, S=S, whole_us=round(whole, 2), factor_us=round(fac, 2), sweep_us=round(sweep, 2),
                       store_bound_us=round(bound, 2), sweep_store_share=round(bound / sweep, 3) if sweep > 0 else None)
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
