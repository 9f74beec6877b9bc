#!/usr/bin/env python
"""Time the cross-validated predictions (gp_xval) of 512 (sample, PC) units at n = 512, d = 8
against the factorisation they follow and against the refit route through the existing API.

    python tools/bench_xval.py [--reps 10] [--units 512] [--out FILE]

GPU, device events around single calls after a warm-up, median of `--reps`:
  (a) gp_xval, leave-one-out (the NULL fold form) -- algorithmic bytes 4 n^2 per unit;
  (b) gp_xval, 8 folds of 64 drawn from a permutation -- 8 sum_F (n - min F) f bytes per unit;
  (c) gp_potrf_inv on the same batch (each call on a fresh copy of the Gram matrices);
  (d) the refit route for the 8 folds: eight emulator.predict_units calls, each on the design
      without its fold, predicting at the fold's points (host clock around calls that end in a
      synchronise).
GB/s are the algorithmic bytes over the time; z = L^-1 w (gp_xval's first kernel, another
4 n^2 bytes per unit) is inside (a) and (b) and not in their byte counts.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gladsgp_amd import _capi, emulator, kernels  # noqa: E402

N, D, NFOLDS, F = 512, 8, 8, 64


def _event_ms(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xval: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    U = args.units
    rng = np.random.default_rng(0)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa
    X = t(rng.random((N, D)))
    beta = t(rng.uniform(0.5, 5.0, (U, D)))
    s = t(rng.uniform(0.5, 2.0, U))
    delta = t(rng.uniform(1e-4, 1e-2, U))
    sp = s + 0.4 * delta
    shift = (s + delta - sp).contiguous()
    Xh = X.cpu().numpy()
    w = t(np.sin(2 * np.pi * Xh @ rng.uniform(0, 1, (D, U))).T + 0.1 * np.sum(Xh * Xh, 1))
    folds = rng.permutation(N).reshape(NFOLDS, F)
    ptr = t(np.arange(0, N + 1, F), torch.int32)
    idx = t(folds.reshape(-1), torch.int32)

    G = kernels.gram(X, beta, s, delta, batch=U)
    ch = kernels.cholesky_inverse(G.clone())
    ch.check()
    npad = kernels.padded_n(N)
    mean = torch.empty((U, N), dtype=torch.float64, device=dev)
    var = torch.empty_like(mean)
    info = torch.empty(U, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_capi.lib().gp_xval_ws_bytes(N, NFOLDS, N, U)), dtype=torch.uint8,
                     device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def xval(p, i, nf, ni):
        _capi.call("gp_xval", ch.linv_buf.data_ptr(), npad, npad * npad, N, w.data_ptr(), N, p, i,
                   nf, ni, shift.data_ptr(), mean.data_ptr(), var.data_ptr(), N, info.data_ptr(),
                   U, ws.data_ptr(), ws.numel(), st)

    loo = lambda: xval(None, None, 0, 0)                                      # noqa: E731
    kfold = lambda: xval(ptr.data_ptr(), idx.data_ptr(), NFOLDS, N)           # noqa: E731
    for fn in (loo, kfold):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        assert int(info.abs().max()) == 0
    loo_ms = _event_ms(loo, args.reps)
    kfold_ms = _event_ms(kfold, args.reps)

    box = {}
    potrf_ms = _event_ms(lambda: kernels.cholesky_inverse(box["G"]), args.reps + 2,
                         before=lambda: box.update(G=G.clone()))[2:]
    box.clear()

    def refit():
        for Fk in folds:
            rest = torch.as_tensor(np.setdiff1d(np.arange(N), Fk), device=dev)
            emulator.predict_units(X[rest].contiguous(), X[torch.as_tensor(Fk, device=dev)]
                                   .contiguous(), w[:, rest].contiguous(), beta, s, delta, sp)
        torch.cuda.synchronize()

    refit()
    refit_ms = []
    for _ in range(max(2, args.reps // 3)):
        t0 = time.perf_counter()
        refit()
        refit_ms.append((time.perf_counter() - t0) * 1e3)

    loo_bytes = 4.0 * N * N * U
    kfold_bytes = 8.0 * U * sum((N - int(Fk.min())) * F for Fk in folds)
    med = lambda v: float(np.median(v))                                        # noqa: E731
    out = {"case": {"n": N, "d": D, "units": U, "folds": NFOLDS, "fold_size": F},
           "xval_loo_ms": loo_ms, "xval_loo_ms_median": med(loo_ms),
           "xval_loo_GBps": loo_bytes / med(loo_ms) / 1e6,
           "xval_kfold_ms": kfold_ms, "xval_kfold_ms_median": med(kfold_ms),
           "xval_kfold_GBps": kfold_bytes / med(kfold_ms) / 1e6,
           "potrf_inv_ms": potrf_ms, "potrf_inv_ms_median": med(potrf_ms),
           "refit_8fold_ms": refit_ms, "refit_8fold_ms_median": med(refit_ms),
           "refit_over_potrf_plus_xval": med(refit_ms) / (med(potrf_ms) + med(kfold_ms))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
