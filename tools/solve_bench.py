"""Timing of the multi-right-hand-side solve on the initial states of the C3, c5 and planar1k chains.

    python tools/solve_bench.py [--configs c3,c5,planar1k] [--R 1,n,64,1024] [--reps 30] [--out profiles/solve_bench.json]

Per (config, R):
  * device time, from HIP events on the context stream around synchronised work (median of --reps), of
    gvi_ngd_cov_columns_dev -- the only entry point of the sweep that takes no host buffers -- with ceil(R / n) columns, i.e.
    R_swept = ceil(R / n) n >= R right-hand sides: the whole call, and the factorisation alone (the same call with the sweep
    switched off through gvi_set_option("sample_sweep", 0)); the sweep is the difference.  Store bound: R_swept T n 8 bytes at
    6.1 TB/s (plain stores, MI355X_MICROARCH.md);
  * host wall-clock of ONE gvi_bt_solve_multi with exactly R right-hand sides against R calls of gvi_bt_solve on the same
    host buffers (both copy in, run, copy out and synchronise): median of --wall-reps, one pass for the R = 1024 loop.
"""
import argparse
import json
import os
import sys
import time

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


def wall(fn, reps):
    ts = []
    fn()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5,planar1k")
    ap.add_argument("--R", default="1,n,64,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.Stream()            # a stream of its own: the events and the library's launches share it
    rows = []
    for name in args.configs.split(","):
        ch = syn.make_chain(name)
        T, n = ch["T"], ch["n"]
        D, U = np.ascontiguousarray(ch["D0"], dtype=float), np.ascontiguousarray(ch["U0"], dtype=float)
        ctx = api.Context(0)
        ctx.set_stream(stream.cuda_stream)
        ctx.chain_set(T, n)                 # the state alone: the solve reads (D, U), not the factors
        ctx.ngd_init(ch["mu0"], D, U)
        rng = np.random.default_rng(T)
        for R in (n if r == "n" else int(r) for r in args.R.split(",")):
            ncols = (R + n - 1) // n
            nodes = [(c * 7919) % T for c in range(ncols)]
            buf = torch.empty((ncols, T, n, n), dtype=torch.float64, device="cuda:0")
            ctx.set_option("sample_sweep", 1)
            whole = timed(stream, lambda: ctx.ngd_cov_columns_dev(nodes, buf.data_ptr()), args.reps)
            ctx.set_option("sample_sweep", 0)
            fac = timed(stream, lambda: ctx.ngd_cov_columns_dev(nodes, buf.data_ptr()), args.reps)
            ctx.set_option("sample_sweep", 1)
            sweep = whole - fac
            bound = ncols * n * T * n * 8 / (STORE_TBS * 1e12) * 1e6
            B = rng.standard_normal((R, T, n))
            multi = wall(lambda: ctx.bt_solve_multi(D, U, B), args.wall_reps)

            def singles():
                for r in range(R):
                    ctx.bt_solve(D, U, B[r])
            loop = wall(singles, 1 if R > 64 else args.wall_reps)
            row = dict(config=name, T=T, n=n, R=R, R_swept=ncols * n, whole_us=round(whole, 2), factor_us=round(fac, 2),
                       sweep_us=round(sweep, 2), store_bound_us=round(bound, 2),
                       sweep_store_share=round(bound / sweep, 3) if sweep > 0 else None,
                       solve_multi_wall_us=round(multi, 1), solve_loop_wall_us=round(loop, 1),
                       loop_over_multi=round(loop / multi, 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
