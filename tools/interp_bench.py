"""Timing of the dense-time posterior: gvi_ngd_interp_dev and the sample sweep of
gvi_ngd_sample_interp_dev on the initial states of the C3, planar1k and c5 chains, Q = 8 (T - 1) queries (every interval at
eight times, the constant-velocity operators of synthetic.minacc_interpolation -- the timing does not depend on the values).

    python tools/interp_bench.py [--configs c3,planar1k,c5] [--S 1,64,1024] [--reps 30] [--out profiles/interp_bench.json]

The method of tools/sample_bench.py: HIP events on the context stream around synchronised work, median of --reps.  Per config
the moments launch; per (config, S) the sweep alone = gvi_ngd_sample_interp_dev minus gvi_ngd_sample_dev, once with Qt (the
generator runs) and once with Qt = NULL (no generator: the difference is the generator's share), against the store bound
S Q n 8 bytes at 6.1 TB/s.  One wall-clock line (C3, S = 64): gvi_ngd_sample_interp against gvi_ngd_sample plus the same
algebra in numpy on the host -- the reason for the resident path.
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
from sample_bench import STORE_TBS, timed  # noqa: E402

PER_INTERVAL = 8


def query_set(T, n):
    ops = [syn.minacc_interpolation(n // 2, syn.QC, 0.25, j * 0.25 / PER_INTERVAL) for j in range(PER_INTERVAL)]
    idx = np.repeat(np.arange(T - 1, dtype=np.int32), PER_INTERVAL)
    A, B, Qt = (np.tile(np.stack([o[k] for o in ops]), (T - 1, 1, 1)) for k in range(3))
    return idx, A, B, Qt


def host_interp(X, idx, A, B, L, z):
    return np.einsum("qrk,sqk->sqr", A, X[:, idx]) + np.einsum("qrk,sqk->sqr", B, X[:, idx + 1]) + np.einsum("qrk,sqk->sqr", L, z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,planar1k,c5")
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
        ctx.chain_set(T, n)                 # the state alone: the queries read (mu, D, U, SigD, SigU), not the factors
        ctx.ngd_init(ch["mu0"], ch["D0"], ch["U0"])
        idx, A, B, Qt = query_set(T, n)
        Q = idx.size
        ctx.interp_set(idx, A, B, None, Qt)
        dm = torch.empty((Q, n), dtype=torch.float64, device="cuda:0")
        dc = torch.empty((Q, n, n), dtype=torch.float64, device="cuda:0")
        mom = timed(stream, lambda: ctx.ngd_interp_dev(dm.data_ptr(), dc.data_ptr()), args.reps)
        row = dict(config=name, T=T, n=n, Q=Q, what="moments", moments_us=round(mom, 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
        for S in (int(s) for s in args.S.split(",")):
            dX = torch.empty((S, T, n), dtype=torch.float64, device="cuda:0")
            dXq = torch.empty((S, Q, n), dtype=torch.float64, device="cuda:0")
            sample = timed(stream, lambda: ctx.ngd_sample_dev(S, dX.data_ptr(), seed=1), args.reps)
            both = timed(stream, lambda: ctx.ngd_sample_interp_dev(S, dXq.data_ptr(), 1, 2, 0, x_ptr=dX.data_ptr()), args.reps)
            ctx.interp_set(idx, A, B, None, None)
            quiet = timed(stream, lambda: ctx.ngd_sample_interp_dev(S, dXq.data_ptr(), 1, 2, 0, x_ptr=dX.data_ptr()), args.reps)
            ctx.interp_set(idx, A, B, None, Qt)
            sweep, sweep0 = both - sample, quiet - sample
            bound = S * Q * n * 8 / (STORE_TBS * 1e12) * 1e6
            row = dict(config=name, T=T, n=n, Q=Q, what="sweep", S=S, sample_us=round(sample, 2), sweep_us=round(sweep, 2),
                       sweep_no_noise_us=round(sweep0, 2), generator_us=round(sweep - sweep0, 2), store_bound_us=round(bound, 2),
                       sweep_store_share=round(bound / sweep, 3) if sweep > 0 else None)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del dX, dXq
        if name == "c3":                    # wall clock, host buffers: everything on the device against the host's algebra
            S = 64
            L = np.zeros_like(Qt)
            for q in range(PER_INTERVAL):   # the host's factor of each distinct Qt (tau = 0 has none)
                if Qt[q].any():
                    L[q::PER_INTERVAL] = np.linalg.cholesky(Qt[q])
            dev, host, rng = [], [], np.random.default_rng(2)
            for _ in range(7):
                t0 = time.perf_counter()
                ctx.ngd_sample_interp(S, 1, 2, 0, want_X=False)
                t1 = time.perf_counter()
                X = ctx.ngd_sample(S, 1, 0)
                z = rng.standard_normal((S, Q, n))          # the host's own normals
                host_interp(X, idx, A, B, L, z)
                t2 = time.perf_counter()
                dev.append(t1 - t0)
                host.append(t2 - t1)
            row = dict(config=name, what="wall", S=S, Q=Q, ngd_sample_interp_ms=round(float(np.median(dev)) * 1e3, 3),
                       ngd_sample_plus_numpy_ms=round(float(np.median(host)) * 1e3, 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
