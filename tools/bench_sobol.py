#!/usr/bin/env python
"""Time the Sobol' bootstrap at the reference's case (N = 256, d = 8, p = 8, R = 9,999) on the GPU
against a numpy restatement of the reference's resampling loop on the host.

    python tools/bench_sobol.py [--reps 30] [--out FILE]

GPU: (a) gp_sobol_replicates alone, PHILOX, R = 9,999 with the general indices, device events
around `--reps` back-to-back launches after a warm-up; (b) the whole analysis
(sensitivity.sobol_indices: point estimate, resamples, jackknife, BCa intervals of all four
statistics), host clock around calls that end in a synchronise.  Host: the four statistics of
src/utils.py:207-236 written from their formulas, each evaluated once per resample on fancy-indexed
(d, N, p) arrays, 9,999 resamples + N jackknife samples per statistic as scipy's BCa does (the
interval arithmetic itself is not included), with whatever thread count numpy is given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gladsgp_amd import sensitivity as sn  # noqa: E402

N, D, P, R = 256, 8, 8, 9999


def host_loop(fA, fB, fAB, pcvar, rng):
    """fA, fB (N, p), fAB (d, N, p): 4 x (R + N) statistic evaluations; seconds."""
    def first(arg):
        a, b, c = fA[arg], fB[arg], fAB[:, arg]
        v = np.mean(a * (c - b), axis=1)
        v[v < 0] = 0
        return (v / np.var([a, b], axis=(0, 1))).T

    def total(arg):
        a, b, c = fA[arg], fB[arg], fAB[:, arg]
        return (0.5 * np.mean((b - c) ** 2, axis=1) / np.var([a, b], axis=(0, 1))).T

    w = np.vstack(pcvar)
    stats = (first, total, lambda arg: np.sum(first(arg) * w, axis=0),
             lambda arg: np.sum(total(arg) * w, axis=0))
    t0 = time.perf_counter()
    for st in stats:
        idx = rng.integers(0, N, (R, N))
        for r in range(R):
            st(idx[r])
        base = np.arange(N)
        for r in range(N):
            st(np.delete(base, r))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sobol: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    fA = rng.standard_normal((N, P))
    fB = rng.standard_normal((N, P))
    mix = rng.uniform(0, 1, (D, 1, P))
    fAB = fB[None] + mix * (fA[None] - fB[None]) + 0.05 * rng.standard_normal((D, N, P))
    pcvar = rng.dirichlet(np.ones(P))

    a = torch.from_numpy(np.ascontiguousarray(fA.T)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(fB.T)).to(dev)
    ab = torch.from_numpy(np.ascontiguousarray(fAB.transpose(0, 2, 1))).to(dev)
    pv = torch.from_numpy(pcvar).to(dev)

    def kernel():
        return sn.sobol_replicates(a, b, ab, sn.PHILOX, R=R, seed=1, pcvar=pv, clamp=True)

    for _ in range(5):
        kernel()
    torch.cuda.synchronize()
    kern = []
    for _ in range(5):                                   # 5 windows of `reps` launches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            kernel()
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1) / args.reps)

    tA, tB, tAB = (torch.from_numpy(x).to(dev) for x in (fA, fB, fAB))

    def analysis():
        r = sn.sobol_indices(tA, tB, tAB, pcvar, n_resamples=R, seed=1)
        torch.cuda.synchronize()
        return r

    for _ in range(3):
        analysis()
    full = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            analysis()
        full.append((time.perf_counter() - t0) / args.reps * 1e3)

    host = [host_loop(fA, fB, fAB, pcvar, np.random.default_rng(k)) for k in range(2)]
    gathers = R * P * N * (D + 2)
    out = {"case": {"N": N, "d": D, "p": P, "R": R},
           "kernel_ms_windows": kern, "kernel_ms_median": float(np.median(kern)),
           "kernel_gathers_per_s": gathers / (float(np.median(kern)) * 1e-3),
           "analysis_ms_windows": full, "analysis_ms_median": float(np.median(full)),
           "host_loop_s": host, "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "host_over_analysis": min(host) / (float(np.median(full)) * 1e-3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
