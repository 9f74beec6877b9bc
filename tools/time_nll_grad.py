"""Time the analytic likelihood gradient against a factorisation and against forward differences.

    python tools/time_nll_grad.py [--reps 30] [--out FILE.json]

At (n, d, batch) = (512, 8, 1), (512, 8, 8) and (4096, 8, 1), with HIP events around each group
of launches on the current stream (warmed up first, the median of ``--reps`` repeats):

  1. grad    gp_alpha + gp_nll_grad from an L^-1 that is already there
  2. potrf   one gp_potrf_inv of the same shape (the Gram is rebuilt outside the timed window)
  3. fd      what forward differences cost beside the value: d + 2 further Gram -> gp_potrf_inv ->
             gp_nll chains, one per perturbed parameter
  4. value   one Gram -> gp_potrf_inv -> gp_nll chain (the value both ways need)

Prints one JSON line per shape.  Needs a HIP device: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gladsgp_amd import _capi, kernels  # noqa: E402

SHAPES = ((512, 8, 1), (512, 8, 8), (4096, 8, 1))


def _median_ms(fn, reps, before=None):
    times = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def time_shape(n, d, batch, reps, dev):
    rng = np.random.default_rng(n + batch)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()  # noqa: E731
    Xn = rng.random((n, d))
    X = t(Xn)
    beta = t(rng.uniform(0.5, 5.0, (batch, d)))
    s = t(np.ones(batch))
    delta = t(np.full(batch, 1e-2))
    a = rng.uniform(0, 1, d)
    w = t(np.tile(np.sin(2 * np.pi * Xn @ a) + 0.1 * np.sum(Xn * Xn, axis=1), (batch, 1)))

    G0 = kernels.gram(X, beta, s, delta, batch=batch)
    ch = kernels.cholesky_inverse(G0.clone())
    ch.check()
    # (1) and (2) straight through the C ABI on buffers made once, so the window holds the
    # launches and not the allocator
    lib, st = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    npad = kernels.padded_n(n)
    L = ch.linv_buf
    f64 = dict(dtype=torch.float64, device=dev)
    al, g = torch.empty((batch, n), **f64), torch.empty((batch, d + 2), **f64)
    scratch = lambda nb: torch.empty(max(int(nb), 256), dtype=torch.uint8, device=dev)  # noqa: E731
    ws_a = scratch(lib.gp_alpha_ws_bytes(n, batch))
    ws_g = scratch(lib.gp_nll_grad_ws_bytes(n, d, batch))
    ws_p = scratch(lib.gp_potrf_inv_ws_bytes(n, batch))
    A, L2 = torch.empty_like(G0), torch.empty_like(L)
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    logdet = torch.empty(batch, **f64)

    def grad():
        _capi.call("gp_alpha", L.data_ptr(), npad, npad * npad, n, w.data_ptr(), n, al.data_ptr(),
                   n, batch, ws_a.data_ptr(), ws_a.numel(), st)
        _capi.call("gp_nll_grad", L.data_ptr(), npad, npad * npad, X.data_ptr(), d, n, d,
                   beta.data_ptr(), d, s.data_ptr(), al.data_ptr(), n, g.data_ptr(), d + 2, batch,
                   ws_g.data_ptr(), ws_g.numel(), st)

    def regram():
        A.copy_(G0)

    def potrf():
        _capi.call("gp_potrf_inv_ws", A.data_ptr(), n, n, n * n, L2.data_ptr(), npad, npad * npad,
                   batch, info.data_ptr(), logdet.data_ptr(), ws_p.data_ptr(), ws_p.numel(), st)

    def chain():
        kernels.nll(kernels.cholesky_inverse(kernels.gram(X, beta, s, delta, batch=batch)), w)

    def fd():
        for _ in range(d + 2):
            chain()

    out = {"n": n, "d": d, "batch": batch, "reps": reps}
    for name, fn, before in (("grad", grad, None), ("potrf", potrf, regram),
                             ("value", chain, None), ("fd", fd, None)):
        for _ in range(3):                       # warm-up: code objects, scratch growth
            if before is not None:
                before()
            fn()
        torch.cuda.synchronize(dev)
        med, lo, hi = _median_ms(fn, reps, before)
        out[name + "_ms"] = round(med, 4)
        out[name + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
    out["grad_over_potrf"] = round(out["grad_ms"] / out["potrf_ms"], 3)
    out["value_plus_grad_in_chains"] = round((out["value_ms"] + out["grad_ms"]) / out["value_ms"], 3)
    out["fd_in_chains"] = round((out["value_ms"] + out["fd_ms"]) / out["value_ms"], 3)
    out["tile_flop"] = batch * n ** 3 / 3.0          # the triangular K^-1 product alone
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nll_grad: no HIP device (there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [time_shape(n, d, b, args.reps, dev) for n, d, b in SHAPES]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
