"""Time the closed-form Sobol' indices against the Saltelli path they replace.

    python tools/time_sobol_exact.py [--reps 5] [--out FILE.json]

At the reference's configuration (n = 512, d = 8, S = 32 posterior samples, P = 8 PCs;
sensitivity_indices.py:71, 96), in one process, the median of ``--reps`` repeats after a warm-up:

  1. kernel_mean    gp_sobol_exact alone, one PC of the "mean" mode (G = 1, M = 32: 528 unit pairs
                    of 512^2 point pairs), HIP events; its achieved erf/s by the operation count
                    2 d erf per point pair and unit pair (+ n d per unit), and the fraction of the
                    fp64 vector rate that count stands for
  2. kernel_sample  gp_sobol_exact alone, one PC of the "sample" mode (G = 32, M = 1)
  3. exact_mean     sensitivity.exact_indices(average="mean"): the alpha chain of all 256 GPs, 8
                    kernel calls, the index arithmetic; host clock around a call that ends in a
                    synchronise
  4. exact_sample   the same with average="sample"
  5. saltelli       PCA_saltelli_sensitivity_indices over emulator_func with m = 8 and 9,999
                    resamples, as the driver runs it

Prints one JSON line.  Needs a HIP device: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gladsgp_amd import _capi, response, sensitivity  # noqa: E402
from gladsgp_amd import model as gm  # noqa: E402

N, D, S, P, NY = 512, 8, 32, 8, 64
# operations per erf / erfc the fraction is quoted for: ocml's rational approximations take about
# 40 fp64 VALU operations each; with the exp (19) and the ~15 multiplies and adds around them a
# (point pair, dimension) costs about 2 * 40 + 19 + 15 = 114
OPS_PER_PAIR_DIM = 114
PEAK_FP64_VALU = 78.6e12          # MI355X data sheet, vector fp64 flop/s (an fma counts 2)


def _ensemble(rng):
    t = rng.random((N, D))
    modes = rng.standard_normal((P, NY)) * (0.6 ** np.arange(P))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, D) + k) for k in range(P)], 1)
    y = 3.0 + coef @ modes + 1e-2 * rng.standard_normal((N, NY))
    return t.astype(np.float32), y.astype(np.float32)


def _samples(rng):
    return {"betaU": rng.uniform(0.2, 3.0, (S, (D + 1) * P)),
            "lamUz": rng.uniform(0.5, 3.0, (S, P)),
            "lamWs": rng.uniform(200, 3000, (S, P)),
            "lamWOs": rng.uniform(50, 500, (S, 1))}


def _events_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def _clock_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sobol_exact: no HIP device (there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    t, y = _ensemble(rng)
    with tempfile.TemporaryDirectory() as tmp:
        _, model = gm.init_model(t, y, "time_sobol_exact", P, data_dir=tmp, device=dev,
                                 verbose=False)
    samples = _samples(rng)
    pcvar = rng.dirichlet(np.ones(P))

    # the kernel alone, through the C ABI on buffers made once
    alpha, beta, s, _, _ = response.unit_alpha(model, samples)
    pm = lambda a: a.reshape(S, P, -1).transpose(0, 1).reshape(P * S, -1).contiguous()  # noqa: E731
    alpha, beta, s = pm(alpha)[:S], pm(beta)[:S], pm(s).reshape(-1)[:S].contiguous()   # PC 0
    X = model.data.sim_data.t_dev.contiguous()
    lib, st = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    nq = 2 * D + 1
    out = {"n": N, "d": D, "S": S, "P": P, "reps": args.reps}
    for name, G, M in (("kernel_mean", 1, S), ("kernel_sample", S, 1)):
        nb = int(lib.gp_sobol_exact_ws_bytes(N, D, G, M))
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
        E = torch.empty(S, dtype=torch.float64, device=dev)
        Q = torch.empty((G, M, M, nq), dtype=torch.float64, device=dev)

        def call():
            _capi.call("gp_sobol_exact", X.data_ptr(), N, D, D, G, M, alpha.data_ptr(), N,
                       beta.data_ptr(), D, s.data_ptr(), None, None, E.data_ptr(), 1,
                       Q.data_ptr(), nq, M * nq, M * M * nq, ws.data_ptr(), nb, st)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        med, lo, hi = _events_ms(call, args.reps)
        pairs = G * M * (M + 1) // 2
        # a unit paired with itself needs the lower tiles only: 36 of 64 at n = 512
        nt = -(-N // 64)
        tile_pairs = (pairs - G * M) * nt * nt + G * M * (nt * (nt + 1) // 2)
        pair_dims = tile_pairs * 64 * 64 * D
        out[name + "_ms"] = round(med, 4)
        out[name + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
        out[name + "_erf_per_s"] = 2 * pair_dims / (med * 1e-3)
        out[name + "_fp64_valu_fraction"] = round(
            pair_dims * OPS_PER_PAIR_DIM / (med * 1e-3) / (PEAK_FP64_VALU / 2), 4)
        out[name + "_ws_bytes"] = nb

    for mode in ("mean", "sample"):
        fn = lambda: sensitivity.exact_indices(model, samples, pcvar=pcvar, average=mode)  # noqa
        fn()
        torch.cuda.synchronize()
        med, lo, hi = _clock_ms(fn, args.reps)
        out[f"exact_{mode}_ms"] = round(med, 3)
        out[f"exact_{mode}_min_max_ms"] = [round(lo, 3), round(hi, 3)]

    func = sensitivity.emulator_func(model, samples)
    salt = lambda: sensitivity.PCA_saltelli_sensitivity_indices(func, D, 8, pcvar, seed=1)  # noqa
    salt()
    torch.cuda.synchronize()
    med, lo, hi = _clock_ms(salt, args.reps)
    out["saltelli_ms"] = round(med, 3)
    out["saltelli_min_max_ms"] = [round(lo, 3), round(hi, 3)]
    ex = sensitivity.exact_indices(model, samples, pcvar=pcvar).numpy()
    sl = salt()
    out["saltelli_minus_exact_max"] = {
        "first_order": float(np.max(np.abs(sl[0] - ex.first_order))),
        "total_index": float(np.max(np.abs(sl[1] - ex.total_index)))}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
