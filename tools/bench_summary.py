#!/usr/bin/env python
"""Time EmulatorPrediction.summary() (gp_field_summary: mean and quantile band without the field)
against the composed route that gives the same result from the stored field --
get_y(to_host=False) in float32, then torch.mean and two torch.quantile calls over the sample
axis -- and against gp_field alone on the same S m x ny rows.

Shapes: S = 64 and S = 32 posterior samples, P = 8 PCs, m = 256 test points, ny = 10 000 nodes
(--S / --m / --ny / --P to change).  Method: every route is warmed up, then timed with HIP events
in ABBA order (summary, composed, composed, summary per round; the two bare kernels -- gp_field and
gp_field_summary into preallocated outputs -- after each pair); a timed window repeats its route
until it lasts about --window-ms, so the sub-millisecond routes are not timing the event pair; the
median over rounds is reported with the spread (max - min over rounds, relative to the median).
torch.quantile refuses inputs above 16 M elements, so the composed route takes its quantiles in
blocks of test points below that limit (the mean is one call).

    python tools/bench_summary.py [--rounds 5] [--window-ms 100]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUANTILE_LIMIT = 16_000_000          # torch.quantile's input size limit (elements)


def build_prediction(S, m, P, ny, dev, tmp):
    from gladsgp_amd import model as gm
    from gladsgp_amd.emulator import EmulatorPrediction
    rng = np.random.default_rng(0)
    n, d = 64, 6
    t = rng.random((n, d)).astype(np.float32)
    modes = rng.standard_normal((P + 2, ny)) * (0.7 ** np.arange(P + 2))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + k) for k in range(P + 2)], 1)
    y = (3.0 + coef @ modes + 1e-2 * rng.standard_normal((n, ny))).astype(np.float32)
    _, model = gm.init_model(t, y, "bench_summary", P, data_dir=tmp, device=dev, verbose=False)
    samples = {"betaU": rng.uniform(0.2, 3.0, (S, (d + 1) * P)),
               "lamUz": rng.uniform(0.5, 3.0, (S, P)),
               "lamWs": rng.uniform(200, 3000, (S, P)),
               "lamWOs": rng.uniform(50, 500, (S, 1))}
    preds = EmulatorPrediction(model=model, samples=samples, t_pred=rng.random((m, d)),
                               realize=True, seed=1)
    preds.w = preds.w.astype(np.float32)          # the reference's float32 path
    return preds


def composed(preds, q):
    """The route without the summary kernel: the float32 field, its mean and two quantiles."""
    y = preds.get_y(to_host=False)
    S, m, ny = y.shape
    mean = torch.mean(y, dim=0)
    lo = torch.empty_like(mean)
    hi = torch.empty_like(mean)
    mb = max(1, QUANTILE_LIMIT // (S * ny))
    for a in range(0, m, mb):
        lo[a:a + mb] = torch.quantile(y[:, a:a + mb], q, dim=0)
        hi[a:a + mb] = torch.quantile(y[:, a:a + mb], 1 - q, dim=0)
    return mean, lo, hi


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--S", type=int, nargs="+", default=[64, 32])
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--ny", type=int, default=10_000)
    ap.add_argument("--q", type=float, default=0.025)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_summary: no HIP device (timings are taken on the GPU only)")
    import tempfile
    from gladsgp_amd import blas
    dev = torch.device("cuda:0")
    for S in args.S:
        with tempfile.TemporaryDirectory() as tmp:
            preds = build_prediction(S, args.m, args.P, args.ny, dev, tmp)
        m, P, ny, q = args.m, args.P, args.ny, args.q
        sd_ = preds.model.data.sim_data
        w2 = preds.w_dev.reshape(S * m, P).contiguous()
        yf = torch.empty((S * m, ny), dtype=torch.float32, device=dev)
        so = tuple(torch.empty((m, ny), dtype=torch.float32, device=dev) for _ in range(3))
        routes = {
            "summary": lambda: preds.summary(q, add_error=False, to_host=False),
            "composed": lambda: composed(preds, q),
            "field": lambda: blas.field(w2, sd_.K, sd_.y_sd, sd_.y_mean, None, f32=True, out=yf),
            "kernel": lambda: blas.field_summary(preds.w_dev, sd_.K, sd_.y_sd, sd_.y_mean, None,
                                                 q=q, f32=True, out=so),
        }
        # same result first (float32 outputs of fp64 sums against float32 sums / sorts)
        got, ref = routes["summary"](), routes["composed"]()
        scale = float(ref[0].abs().max())
        diffs = [float((g - r).abs().max()) / scale for g, r in zip(got, ref)]
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        reps = {k: max(3, int(np.ceil(args.window_ms / max(timed(fn, 3), 1e-3))))
                for k, fn in routes.items()}
        ts = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k in ("summary", "composed", "composed", "summary"):        # ABBA
                ts[k].append(timed(routes[k], reps[k]))
            for k in ("field", "kernel"):
                ts[k].append(timed(routes[k], reps[k]))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ts.items()}
        field_bytes, out_bytes = S * m * ny * 4, 3 * m * ny * 4
        print(f"S={S} m={m} P={P} ny={ny} q={q}  rounds={args.rounds} calls per window "
              + " ".join(f"{k}={v}" for k, v in reps.items()))
        print(f"  summary()      {med['summary']:9.3f} ms  spread {100 * spread['summary']:5.1f} %"
              f"  writes {out_bytes / 1e6:8.1f} MB")
        print(f"  composed route {med['composed']:9.3f} ms  spread "
              f"{100 * spread['composed']:5.1f} %  writes {(field_bytes + out_bytes) / 1e6:8.1f} MB (field + results; the sorts'"
              " scratch not counted)")
        print(f"  gp_field alone {med['field']:9.3f} ms  spread {100 * spread['field']:5.1f} %"
              f"  writes {field_bytes / 1e6:8.1f} MB")
        print(f"  gp_field_summary alone {med['kernel']:9.3f} ms  spread "
              f"{100 * spread['kernel']:5.1f} %  writes {out_bytes / 1e6:8.1f} MB")
        print(f"  composed / summary = {med['composed'] / med['summary']:.2f}x, "
              f"summary / gp_field = {med['summary'] / med['field']:.2f}x, "
              f"gp_field_summary / gp_field = {med['kernel'] / med['field']:.2f}x, "
              f"max |summary - composed| / max|mean| = "
              f"{diffs[0]:.1e} (mean) {diffs[1]:.1e} (lower) {diffs[2]:.1e} (upper)")
        del preds, yf, so
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
