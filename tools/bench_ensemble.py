"""Ensemble sampler against the same chains run one after another (mcmc.EnsembleSampler vs C lone
mcmc.GPUSamplers), at the two shapes the reference drives:

  scalar   16 P = 1 emulators on one n = 512, d = 8 design (fit_scalar_models.py:438-477);
  chains   4 repeat chains of the n = 512, P = 8 fit model (mcmc_diagnostics_advanced.py:50-54).

Each timed window is ``--nsamp`` recorded sweeps of every chain after warm-up (graphs captured,
every shape run once), a host clock around run(), which ends in a device synchronise and the
copy of the samples to the host.  GPUSampler is the baseline: the sequential window is what the
package did before it had an ensemble.  Windows alternate in ABBA order (ensemble, sequential,
sequential, ensemble) ``--repeats`` times in one process; the report gives each side's median
and its spread (min .. max), and the ensemble's gp_loglik time per call (device events around a
run of calls on the largest group's batch).  One JSON line per shape; ``--out`` also writes them
to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gladsgp_amd import mcmc  # noqa: E402

F64 = torch.float64


def problem(n, d, P, C, same_w, seed):
    """One design and C sets of PC weights drawn from GPs (one set repeated when ``same_w``)."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    D2 = (X[:, None, :] - X[None, :, :]) ** 2
    sets = []
    for _ in range(1 if same_w else C):
        w = np.empty((P, n))
        for j in range(P):
            G = np.exp(-(D2 * rng.uniform(0.5, 4.0, d)).sum(-1)) + 1e-3 * np.eye(n)
            w[j] = np.linalg.cholesky(G) @ rng.standard_normal(n)
        sets.append(w)
    w = np.stack(sets * C if same_w else sets)
    lam = np.tile(rng.uniform(1.0, 10.0, (1, P)), (C, 1)) if same_w else rng.uniform(1, 10, (C, P))
    return X, w, lam


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loglik_ms_per_call(ens, calls=200):
    sets = max(k for k in ens._gbuf)
    for _ in range(10):
        ens._loglik(sets)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        ens._loglik(sets)
    b.record()
    torch.cuda.synchronize()
    buf = ens._gbuf[sets]
    slices = -(-ens.C // buf["chunk"])
    return {"state_sets": sets, "problems": ens.C * sets * ens.P, "slices": slices,
            "ms_per_call": a.elapsed_time(b) / calls / slices}


def measure(name, n, d, P, C, same_w, nsamp, repeats, dev, spec=None):
    X, w, lam = problem(n, d, P, C, same_w, seed=P)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa: E731
    Xd = t(X)
    ens = mcmc.EnsembleSampler(Xd, t(w), t(lam), [mcmc.ModelParams(d, P) for _ in range(C)],
                               spec=spec)
    lone = [mcmc.GPUSampler(Xd, t(w[c]), t(lam[c]), mcmc.ModelParams(d, P)) for c in range(C)]
    rngs = [np.random.default_rng(c) for c in range(C)]
    warm = 2 * ens.block + 3

    def run_ens():
        return ens.run(nsamp, rngs)

    def run_seq():
        return [s.run(nsamp, r) for s, r in zip(lone, rngs)]

    ens.run(warm, rngs)
    for s, r in zip(lone, rngs):
        s.run(warm, r)
    te, ts = [], []
    for _ in range(repeats):                            # ABBA
        te.append(window(run_ens))
        ts.append(window(run_seq))
        ts.append(window(run_seq))
        te.append(window(run_ens))
    out = {"shape": name, "n": n, "d": d, "P": P, "chains": C, "sweeps": nsamp,
           "repeats": repeats, "ensemble_spec": ens.spec, "lone_spec": lone[0].spec,
           "max_batch": ens.max_batch,
           "ensemble_s": {"median": statistics.median(te), "min": min(te), "max": max(te)},
           "sequential_s": {"median": statistics.median(ts), "min": min(ts), "max": max(ts)},
           "ensemble_ms_per_sweep": 1e3 * statistics.median(te) / nsamp,
           "sequential_ms_per_sweep_all_chains": 1e3 * statistics.median(ts) / nsamp,
           "speedup_median": statistics.median(ts) / statistics.median(te),
           "beats_by_more_than_spread": min(ts) > max(te),
           "ensemble_loglik": loglik_ms_per_call(ens)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--nsamp", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="scalar,chains")
    ap.add_argument("--ens-spec", type=int, default=None,
                    help="group size of the ensemble (default: its own choice)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs a HIP device")
    dev = torch.device("cuda:0")
    res = []
    if "scalar" in a.shapes:
        res.append(measure("scalar", a.n, 8, 1, 16, False, a.nsamp, a.repeats, dev,
                           a.ens_spec))
    if "chains" in a.shapes:
        res.append(measure("chains", a.n, 8, 8, 4, True, a.nsamp, a.repeats, dev,
                           a.ens_spec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
