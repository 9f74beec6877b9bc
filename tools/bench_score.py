#!/usr/bin/env python
"""Time the fused test-error scoring (gp_field_score, EmulatorPrediction.score) against what it
replaces, on one device in one run:

  (a) gp_field_score alone (blas.field_score, no maps: m x 8 and ny x 4 sums)
  (b) gp_field_summary alone (blas.field_summary into preallocated (m, ny) outputs)
  (c) the composed device route: summary(to_host=False), then the torch reductions that give the
      same rows and cols on the device (gladsgp_amd.score.sums_from_maps)
  (d) end to end to host numpy: score(y_test) against summary() followed by the host
      reductions its caller needs (per-point RMSE, floored MAPE, mean bounds, coverage; per-node
      RMSE), in numpy on the float32 maps

Shapes: P = 8 PCs, m = 256 test points, ny = 10 000 nodes, S = 32 and 64 posterior samples,
float32 outputs (--S / --m / --ny / --P to change).  Method (tools/bench_summary.py's): every route
is warmed up, then timed with HIP events -- the end-to-end pair ends in host arrays, so its
windows are closed by the copies themselves -- in ABBA order per pair; a timed window repeats
its route until it lasts about --window-ms; the median over rounds is reported with the spread
(max - min over rounds, relative to the median).  Also prints gp_field_score's workspace size here
and at the reference's ny = 1 347 945, m = 100.

    python tools/bench_score.py [--rounds 5] [--window-ms 100]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_summary import build_prediction, timed  # noqa: E402


def numpy_scores(mean, lo, hi, y, lq):
    """What a caller of summary() computes on the host, in the arrays' own dtype: per-point
    RMSE, floored MAPE, mean bounds and coverage, and the per-node RMSE."""
    sq = (mean - y) ** 2
    ape = np.where(y < lq, np.nan, np.abs((mean - y) / y))
    inside = (lo <= y) & (y <= hi)
    table = np.stack([np.sqrt(sq.mean(1)), np.nanmean(ape, 1), lo.mean(1), hi.mean(1),
                      inside.mean(1)], axis=1)
    return table, np.sqrt(np.nanmean(sq, 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--S", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--ny", type=int, default=10_000)
    ap.add_argument("--q", type=float, default=0.025)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_score: no HIP device (timings are taken on the GPU only)")
    from gladsgp_amd import blas
    from gladsgp_amd import score as gscore
    dev = torch.device("cuda:0")
    print(f"gp_field_score workspace: {blas.field_score_ws_bytes(64, 100, 8, 1_347_945) / 1e6:.1f}"
          f" MB at ny = 1 347 945, m = 100 (three float32 maps: "
          f"{3 * 4 * 100 * 1_347_945 / 1e6:.1f} MB)")
    for S in args.S:
        with tempfile.TemporaryDirectory() as tmp:
            preds = build_prediction(S, args.m, args.P, args.ny, dev, tmp)
        m, P, ny, q = args.m, args.P, args.ny, args.q
        sd_ = preds.model.data.sim_data
        so = tuple(torch.empty((m, ny), dtype=torch.float32, device=dev) for _ in range(3))
        mean0 = preds.summary(q, add_error=False)[0]
        rng = np.random.default_rng(1)
        y_host = (mean0 + 0.05 * rng.standard_normal((m, ny))).astype(np.float32)
        Y = torch.as_tensor(y_host, device=dev)
        lq = float(np.quantile(y_host, 0.1))
        W, K, sd, mu = preds.w_dev, sd_.K, sd_.y_sd, sd_.y_mean

        def composed():
            maps = preds.summary(q, add_error=False, to_host=False)
            return gscore.sums_from_maps(*maps, Y, lq)

        routes = {
            "score": lambda: blas.field_score(W, K, sd, mu, None, Y, q=q, mape_floor=lq, f32=True),
            "summary": lambda: blas.field_summary(W, K, sd, mu, None, q=q, f32=True, out=so),
            "composed": composed,
            "score_host": lambda: preds.score(y_host, q, mape_floor=lq, add_error=False).table(),
            "summary_host": lambda: numpy_scores(*preds.summary(q, add_error=False), y_host, lq),
        }
        # the same numbers first: kernel sums against the torch reduction of the stored maps, and
        # the end-to-end tables (fp64 sums against the reference's float32 numpy)
        r1, c1 = routes["score"]()
        r2, c2 = routes["composed"]()
        d_rows = float(((r1 - r2).abs() / r2.abs().clamp_min(1e-300)).max())
        d_cols = float(((c1 - c2).abs() / c2.abs().clamp_min(1e-300)).max())
        t1 = routes["score_host"]()
        t2, _ = routes["summary_host"]()
        d_tab = float(np.nanmax(np.abs(t1[:, [0, 1, 2, 3, 5]] - t2) / np.abs(t2)))
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        reps = {k: max(3, int(np.ceil(args.window_ms / max(timed(fn, 3), 1e-3))))
                for k, fn in routes.items()}
        ts = {k: [] for k in routes}
        for _ in range(args.rounds):
            for a, b in (("score", "summary"), ("score", "composed"),
                         ("score_host", "summary_host")):
                for k in (a, b, b, a):                                      # ABBA
                    ts[k].append(timed(routes[k], reps[k]))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ts.items()}
        ws = blas.field_score_ws_bytes(S, m, P, ny)
        print(f"S={S} m={m} P={P} ny={ny} q={q}  rounds={args.rounds} calls per window "
              + " ".join(f"{k}={v}" for k, v in reps.items()))
        names = {"score": "(a) gp_field_score alone", "summary": "(b) gp_field_summary alone",
                 "composed": "(c) summary + torch reductions", "score_host": "(d) score() to host",
                 "summary_host": "(d) summary() + numpy"}
        for k, nm in names.items():
            print(f"  {nm:32s} {med[k]:9.3f} ms  spread {100 * spread[k]:5.1f} %")
        print(f"  (a) / (b) = {med['score'] / med['summary']:.2f}, (c) / (a) = "
              f"{med['composed'] / med['score']:.2f}x, (d) summary+numpy / score = "
              f"{med['summary_host'] / med['score_host']:.2f}x; workspace {ws / 1e6:.2f} MB, "
              f"outputs {(m * 8 + ny * 4) * 8 / 1e3:.1f} KB against {3 * m * ny * 4 / 1e6:.1f} MB "
              "of maps")
        print(f"  max rel. difference: rows {d_rows:.1e}, cols {d_cols:.1e} (kernel against torch "
              f"on the stored maps), table {d_tab:.1e} (fp64 sums against float32 numpy)")
        del preds, so
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
