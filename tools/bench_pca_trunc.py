#!/usr/bin/env python
"""Time the fused PCA truncation-error curve (gp_pca_trunc, blas.pca_trunc) against the loop it
replaces, on one device in one run:

  (a) fused: one blas.pca_trunc call for all levels (tot only)
  (b) loop:  per level, blas.gemm for the rank-k product C[:, :k] V[:k] (an (n, ny) fp64 output)
      and torch for the residual and its squared norm, in place on the product
      (plot_PC_RMSE.py:96-102 with this package's pieces before gp_pca_trunc existed)

Cases: the reference's architecture study (n = 512 simulations, ny = 1 347 945 nodes, float32
ensemble, its 26 ranks up to 100) and a small one (n = 64, ny = 100 000, the ranks clamped to 64).
Random operands (signal + noise), generated on the device.  Method: both routes are warmed up,
then timed with HIP events; a timed window repeats its route until it lasts about --window-ms
(at least once); windows alternate ABBA per round; the median over rounds is reported with the
spread (max - min over rounds, relative to the median).  Also reported: the fused call's
fraction of the fp64 MFMA floor 2 n ny Kpad / 78.6 TF/s (Kpad: the inner dimension with every
level's segment padded to a multiple of 4) and of the single-read HBM floor (Y, V, mu, sd once
at 8 TB/s).

    python tools/bench_pca_trunc.py [--rounds 3] [--window-ms 200] [--cases big small]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_summary import timed  # noqa: E402

MFMA_F64 = 78.6e12        # flop/s, fp64 MFMA peak
HBM = 8.0e12              # B/s
REFERENCE_RANKS = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 17, 21, 25, 30, 35, 40, 46, 53,
                            60, 67, 74, 82, 91, 100])      # the architecture study's 26 ranks
CASES = {"big": (512, 1_347_945), "small": (64, 100_000)}


def padded_k(ranks):
    kp, prev = 0, 0
    for r in ranks:
        kp += (r - prev + 3) // 4 * 4
        prev = r
    return max(kp, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", nargs="+", default=["small", "big"], choices=sorted(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pca_trunc: no HIP device (timings are taken on the GPU only)")
    from gladsgp_amd import blas
    from gladsgp_amd.blas import CM, gemm
    dev = torch.device("cuda:0")
    for case in args.cases:
        n, ny = CASES[case]
        ranks = [int(r) for r in np.unique(np.minimum(REFERENCE_RANKS, min(100, n)))]
        p = ranks[-1]
        g = torch.Generator(device=dev).manual_seed(1)
        S = 2.0 ** (-torch.arange(p, dtype=torch.float64, device=dev) / 8.0)
        C = torch.randn((n, p), dtype=torch.float64, device=dev, generator=g) * S[None, :]
        V = torch.randn((p, ny), dtype=torch.float64, device=dev, generator=g) / np.sqrt(p)
        mu = torch.randn(ny, dtype=torch.float64, device=dev, generator=g) * 3.0
        sd = torch.rand(ny, dtype=torch.float64, device=dev, generator=g) * 1.5 + 0.5
        Y = torch.empty((n, ny), dtype=torch.float32, device=dev)
        for i0 in range(0, n, 64):                      # in row blocks: no second (n, ny) fp64
            blk = C[i0:i0 + 64] @ V
            blk.mul_(sd).add_(mu)
            blk.add_(torch.randn(blk.shape, dtype=torch.float64, device=dev, generator=g), alpha=1e-3)
            Y[i0:i0 + 64] = blk.to(torch.float32)
            del blk
        Vc = [CM.of_rowmajor(V[:k]) for k in ranks]                     # (ny x k) views
        Cc = [CM.of_rowmajor(C[:, :k].contiguous()) for k in ranks]     # (k x n)
        prod = CM.empty(ny, n, dev)                                     # (n, ny) row-major
        sse_loop = torch.empty(len(ranks), dtype=torch.float64, device=dev)

        def fused():
            return blas.pca_trunc(Y, C, V, ranks, mu=mu, sd=sd)[0]

        def loop():
            for i in range(len(ranks)):
                gemm(False, False, Vc[i], Cc[i], C=prod)
                e = prod.rowmajor_T()
                e.mul_(sd).sub_(Y).add_(mu)                             # -(residual), in place
                sse_loop[i] = torch.linalg.vector_norm(e) ** 2
            return sse_loop

        a = fused()[:, 0].clone()
        b = loop().clone()
        diff = float(((a - b).abs() / b).max())
        routes = {"fused": fused, "loop": loop}
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        reps = {k: max(1, int(np.ceil(args.window_ms / max(timed(fn, 1), 1e-3))))
                for k, fn in routes.items()}
        ts = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k in ("fused", "loop", "loop", "fused"):                # ABBA
                ts[k].append(timed(routes[k], reps[k]))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ts.items()}
        kpad = padded_k(ranks)
        t_mfma = 2.0 * n * ny * kpad / MFMA_F64 * 1e3
        t_hbm = (4.0 * n * ny + 8.0 * p * ny + 16.0 * ny) / HBM * 1e3
        print(f"{case}: n={n} ny={ny} float32 Y, {len(ranks)} levels up to rank {p}, Kpad={kpad}; "
              f"rounds={args.rounds} calls per window fused={reps['fused']} loop={reps['loop']}")
        print(f"  (a) fused gp_pca_trunc           {med['fused']:10.3f} ms  spread "
              f"{100 * spread['fused']:5.1f} %")
        print(f"  (b) gemm + torch per level        {med['loop']:10.3f} ms  spread "
              f"{100 * spread['loop']:5.1f} %")
        print(f"  (b) / (a) = {med['loop'] / med['fused']:.1f}x; fp64 MFMA floor {t_mfma:.3f} ms "
              f"(fused at {t_mfma / med['fused']:.2f} of it), single-read HBM floor {t_hbm:.3f} ms "
              f"(fused at {t_hbm / med['fused']:.2f} of it)")
        print(f"  max rel. difference of sum e^2, fused against loop: {diff:.1e}; workspace "
              f"{blas._capi.lib().gp_pca_trunc_ws_bytes(n, ny, len(ranks)) / 1e6:.2f} MB against "
              f"{8 * n * ny / 1e6:.0f} MB per (n, ny) fp64 temporary of the loop")
        del Y, V, C, prod, Vc, Cc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
