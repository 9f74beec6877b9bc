#!/usr/bin/env python
"""Time the joint predictive covariance (gp_predict_cov) and the full joint-draw chain against the
composition the API offered before it, at (n, m, batch) = (512, 512, 512) and (512, 64, 512), d = 8.

    python tools/bench_joint.py [--reps 10] [--batch 512] [--out FILE]

GPU, device events around single calls after a warm-up, median of `--reps`:
  (a) gp_predict_cov from a given L^-1 (cross-covariance, V = L^-1 K*, C = K** - V^T V);
  (b) the composition: kernels.cross, torch.bmm with the dense L^-1, a Gram over Xs with
      s_pred - s on its diagonal and torch.baddbmm into it -- the same C to rounding, which is
      checked before anything is timed;
  (c) the joint chain of EmulatorPrediction(realize="joint") for one group: gram ->
      cholesky_inverse -> predict -> predict_cov -> gp_potrf -> gp_mvn_draw (one draw).
TF/s of (a) count its own arithmetic, n^2 m (the triangular product) + n m^2 (the lower tiles,
mirrored); (b) performs 2 n^2 m + 2 n m^2.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gladsgp_amd import kernels  # noqa: E402

D = 8
SHAPES = [(512, 512), (512, 64)]


def _event_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def case(dev, n, m, U, reps):
    rng = np.random.default_rng([n, m])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float64)   # noqa: E731
    X, Xs = t(rng.random((n, D))), t(rng.random((m, D)))
    beta = t(rng.uniform(0.5, 5.0, (U, D)))
    s = t(rng.uniform(0.5, 2.0, U))
    delta = t(rng.uniform(1e-4, 1e-2, U))
    sp = s + 0.4 * delta
    Xh = X.cpu().numpy()
    w = t(np.sin(2 * np.pi * Xh @ rng.uniform(0, 1, (D, U))).T + 0.1 * np.sum(Xh * Xh, 1))
    ch = kernels.cholesky_inverse(kernels.gram(X, beta, s, delta, batch=U))
    ch.check()
    ws = kernels.PredictWorkspace()
    C = torch.empty((U, m, m), dtype=torch.float64, device=dev)
    LinvT = ch.linv_buf[:, :n, :n]             # memory [b, column, row]: L^-T as a row-major view

    def new():
        kernels.predict_cov(ch, X, Xs, beta, s, sp, out=C, workspace=ws)

    def composed():
        Ks = kernels.cross(X, Xs, beta, s, batch=U)               # (U, m, n): K* row-major
        Vt = torch.bmm(Ks, LinvT)                                  # K* L^-T = V^T
        Kss = kernels.gram(Xs, beta, s, sp - s, batch=U)
        return torch.baddbmm(Kss, Vt, Vt.transpose(1, 2), alpha=-1.0, out=Kss)

    mean = torch.empty((U, m), dtype=torch.float64, device=dev)
    var = torch.empty_like(mean)
    draws = torch.empty((U, 1, m), dtype=torch.float64, device=dev)

    def chain():
        c = kernels.cholesky_inverse(kernels.gram(X, beta, s, delta, batch=U))
        kernels.predict(c, X, Xs, beta, s, sp, w, workspace=ws, out=(mean, var))
        kernels.predict_cov(c, X, Xs, beta, s, sp, out=C, workspace=ws)
        info, _ = kernels.cholesky_inplace(C)
        kernels.mvn_draw(C, mean, 1, 0, 1, out=draws)
        return info

    for fn in (new, composed, chain):
        for _ in range(3):
            fn()
    new()
    diff = float((C - composed()).abs().max())
    assert diff <= 1e-9 * float(s.max()), diff
    assert int(chain().abs().max()) == 0
    new_ms = _event_ms(new, reps)
    comp_ms = _event_ms(composed, reps)
    chain_ms = _event_ms(chain, reps)
    med = lambda v: float(np.median(v))                                         # noqa: E731
    flop = float(U) * (n * n * m + n * m * m)
    return {"n": n, "m": m, "d": D, "batch": U, "max_abs_diff": diff,
            "predict_cov_ms": med(new_ms), "predict_cov_min_ms": min(new_ms),
            "predict_cov_tflops": flop / med(new_ms) * 1e-9,
            "composed_ms": med(comp_ms), "composed_min_ms": min(comp_ms),
            "composed_over_predict_cov": med(comp_ms) / med(new_ms),
            "joint_chain_ms": med(chain_ms), "joint_chain_min_ms": min(chain_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_joint: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "cases": [case(dev, n, m, args.batch, args.reps) for n, m in SHAPES]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
