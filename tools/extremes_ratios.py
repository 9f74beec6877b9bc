"""Print DESIGN.md section 7's tables: the measured error / noise of every chain quantity per
(regime, n), worst over the entry points that produce it and over the factorisation paths, from
the helpers of tests/test_gpu_extremes.py; then the same for the PCA front end (statistics,
eigensolver, randomized SVD, weights) from tests/test_gpu_pca_extremes.py, and for the joint
covariance, its factor and the joint draws from tests/test_gpu_joint_extremes.py, and for the
field back end (gp_field, gp_field_summary, gp_field_score, gp_pca_trunc) from
tests/test_gpu_field_extremes.py, and for gp_xval (the chain and the kernel alone, per fold
plan) from tests/test_gpu_xval_extremes.py.  Needs a HIP device.  Entries above 16 also show, in
parentheses, 16 error / bound with the documented term: they must be in tests/_mp_ref.FINDINGS,
tests/_mp_pca_ref.FINDINGS, tests/_mp_joint_ref.FINDINGS_COV, tests/_mp_field_ref.FINDINGS or
tests/_mp_xval_ref.FINDINGS.

    python tools/extremes_ratios.py [chain|pca|joint|field|xval]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import numpy as np  # noqa: E402

import _mp_pca_ref as P  # noqa: E402
import _mp_ref as M  # noqa: E402
import test_gpu_extremes as T  # noqa: E402
import test_gpu_pca_extremes as TP  # noqa: E402


def fmt(x):
    return f"{x:.2g}" if x < 100 else f"{round(x)}"


def chain(dev):
    sources = dict(T.SOURCES, mean=["mean/" + s for s in T.PRED_SOURCES],
                   var=["var/" + s for s in T.PRED_SOURCES])
    print("| regime | n | " + " | ".join(sources) + " |")
    print("|---|---|" + "---|" * len(sources))
    for regime in M.REGIMES:
        for n in M.SIZES:
            cells = []
            for q, srcs in sources.items():
                err = max(e for s in srcs for e in T.chain_errors(dev, s, regime, n).values())
                nz, lim = M.noise(q, regime, n), M.limit(q, regime, n)
                cell = fmt(err / nz)
                if err > M.MARGIN * nz:
                    cell += f" ({fmt(M.MARGIN * err / lim)})"
                    if (q, regime, n) not in M.FINDINGS:
                        cell += " NOT A DOCUMENTED FINDING"
                cells.append(cell)
            print(f"| {regime} | {n} | " + " | ".join(cells) + " |")


def _worst(err, nz):
    err, nz = np.asarray(err, dtype=float), np.asarray(nz, dtype=float)
    with np.errstate(all="ignore"):
        ratio = np.where(nz > 0, err / nz, np.where(err > 0, np.inf, 0.0))
    return float(np.max(ratio)) if ratio.size else 0.0


def pca(dev):
    print("\n| statistics (n, ny) | mu | sd | y_std |")
    print("|---|---|---|---|")
    for n, ny in TP.STAT_SHAPES:
        err, _ = TP.stats_errors(dev, n, ny)
        print(f"| {n}, {ny} | " + " | ".join(fmt(_worst(*err[q])) for q in ("mu", "sd", "y_std"))
              + " |")
    print("\n| gp_syevj input | r | W | V^T V - I | A V - V W |")
    print("|---|---|---|---|---|")
    for kind in P.EIG_KINDS:
        for r in TP.EIG_SIZES:
            e = TP.eig_errors(dev, kind, r)
            print(f"| {kind} | {r} | " + " | ".join(fmt(_worst(*e[q])) for q in ("W", "VtV", "AV"))
                  + " |")
    cols = ("S", "U", "Vh", "PU0", "PV0", "UtU", "VVt", "resid")
    print("\n| randomized_svd case | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for case in P.SVD_CASES:
        e = TP.svd_errors(dev, case)
        cells = []
        for q in cols:
            if q not in e:
                cells.append("-")
                continue
            err, nz, lim = e[q]
            cell = fmt(_worst(err, nz))
            if np.any(np.asarray(err) > P.MARGIN * np.asarray(nz)):
                cell += f" ({fmt(P.MARGIN * _worst(err, lim))})"
                if (q, case) not in P.FINDINGS:
                    cell += " NOT A DOCUMENTED FINDING"
            cells.append(cell)
        print(f"| {case} | " + " | ".join(cells) + " |")
    print("\n| weights regime | w_hat | LamSim |")
    print("|---|---|---|")
    for regime in ("d2", "d4", "d6"):
        e = TP.weights_errors(dev, regime)
        print(f"| {regime} | {fmt(_worst(*e['w_hat']))} | {fmt(_worst(*e['LamSim']))} |")


def joint(dev):
    """The joint covariance, its factor and the draws (tests/test_gpu_joint_extremes.py)."""
    import _mp_joint_ref as J
    import test_gpu_joint_extremes as TJ
    cols = [f"{n} {pts}" for n, pts in J.CASES]
    print("\n| C: regime | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for regime in M.REGIMES:
        cells = []
        for n, pts in J.CASES:
            err, _ = TJ.cov_errors(dev, regime, n, pts)
            nz, lim = J.noise_cov(regime, n, pts), J.limit_cov(regime, n, pts)
            cell = fmt(err / nz)
            if err > M.MARGIN * nz:
                cell += f" ({fmt(M.MARGIN * err / lim)})"
                if (regime, n) not in J.FINDINGS_COV:
                    cell += " NOT A DOCUMENTED FINDING"
            cells.append(cell)
        print(f"| {regime} | " + " | ".join(cells) + " |")
    cases = [(n, pts, ng) for n, pts in TJ.FACTOR_CASES for ng in (True, False)]
    print("\n| R, logdet: regime | " +
          " | ".join(f"{pts} {'nugget' if ng else 'jitter'}" for _, pts, ng in cases) + " |")
    print("|---|" + "---|" * len(cases))
    for regime in M.REGIMES:
        cells = []
        for n, pts, ng in cases:
            (eR, nR), (eld, nld) = TJ.factor_errors(dev, regime, n, pts, ng)
            cells.append(f"{fmt(eR / nR)}, {fmt(eld / nld)}")
        print(f"| {regime} | " + " | ".join(cells) + " |")
    print("\n| default jitter 1e-8 s at (n, m) = (130, 130): regime | derived sufficient / s | "
          "info | draws finite |")
    print("|---|---|---|---|")
    for group in M.GROUPS:
        for regime, derived, info, finite in TJ.default_jitter_run(dev, group):
            print(f"| {regime} | {derived:.2e} | {info} | {finite} |")
    print("\n| draws: m | " + " | ".join(f"nsamp {k}: error / noise, / bound, / per-element bound"
                                         for k in (1, 8, 9)) + " |")
    print("|---|---|---|---|")
    for m in (1, 63, 64, 65, 257):
        cells = []
        for nsamp in (1, 8, 9):
            err, bound, nz, tight = TJ.draw_errors(dev, m, nsamp)
            cells.append(f"{fmt(float(np.max(err / nz)))}, {fmt(float(np.max(err / bound)))}, "
                         f"{fmt(float(np.max(err / tight)))}")
        print(f"| {m} | " + " | ".join(cells) + " |")


def field(dev):
    """The field back end (tests/test_gpu_field_extremes.py): worst error / noise per (kernel
    output, regime) over the regime's cases; float32 columns show what is left above half a
    float32 ulp of the truth."""
    import _mp_field_ref as F
    import test_gpu_field_extremes as TF

    def table(title, names, regimes, cells):
        print(f"\n| {title} | " + " | ".join(names) + " |")
        print("|---|" + "---|" * len(names))
        for regime in regimes:
            print(f"| {regime} | " + " | ".join(cells[regime].get(nm, "-") for nm in names) + " |")

    def put(acc, regime, nm, ratio):
        acc.setdefault(regime, {})
        acc[regime][nm] = max(acc[regime].get(nm, 0.0), ratio)

    acc = {}
    for case in F.FIELD_CASES:
        for sdmu, err, e64, nz, exc, _, _ in TF.field_errors(dev, case):
            put(acc, case[0], "field fp64", _worst(e64, nz))
            put(acc, case[0], "field float32", _worst(exc, nz))
    for case in F.SUMMARY_CASES:
        for nm, (e, nz, exc) in TF.summary_errors(dev, case)[0].items():
            put(acc, case[0], nm, _worst(e, nz))
            put(acc, case[0], nm + " float32", _worst(exc, nz))
    for scase in F.SCORE_CASES:
        er, nr, ec, nc, _, _ = TF.score_errors(dev, scase)
        regime = F.SUMMARY_CASES[scase[0]][0]
        sr = [k for k in range(8) if k not in TF.ROW_COUNTS]
        sc = [k for k in range(4) if k not in TF.COL_COUNTS]
        put(acc, regime, "score rows", _worst(er[:, sr], nr[:, sr]))
        put(acc, regime, "score cols", _worst(ec[:, sc], nc[:, sc]))
    names = ["field fp64", "field float32", "mean", "lo", "hi", "mean float32", "lo float32",
             "hi float32", "score rows", "score cols"]
    table("field regime", names, F.FIELD_REGIMES,
          {r: {nm: fmt(v) for nm, v in acc[r].items()} for r in acc})

    acc, cells = {}, {}
    names = ["sse", "sum", "node", "rmse", "var"]
    for case in F.TRUNC_CASES:
        for nm, (e, nz, lim) in TF.trunc_errors(dev, case).items():
            put(acc, case[0], nm, _worst(e, nz))
            if np.any(e > F.MARGIN * nz):
                put(acc, case[0], nm + " bound", F.MARGIN * _worst(e, lim))
    for regime, row in acc.items():
        cells[regime] = {}
        for nm in names:
            cell = fmt(row[nm])
            if nm + " bound" in row:
                cell += f" ({fmt(row[nm + ' bound'])})"
                if (nm, regime) not in F.FINDINGS:
                    cell += " NOT A DOCUMENTED FINDING"
            cells[regime][nm] = cell
    table("gp_pca_trunc regime", names, F.TRUNC_REGIMES, cells)


def xval(dev):
    """gp_xval (tests/test_gpu_xval_extremes.py): error / noise per (quantity, regime, n, plan)
    for the chain and for the kernel alone on the truth's and on the device's L^-1."""
    import _mp_xval_ref as X
    import test_gpu_xval_extremes as TX
    layers = ("chain", "hi", "dev")
    print("\n| regime | n | plan | " +
          " | ".join(f"{layer} {q}" for layer in layers for q in X.QUANTITIES) + " |")
    print("|---|---|---|" + "---|" * (3 * len(layers)))
    worst = {layer: (0.0, None) for layer in layers}
    for regime, n, plan in X.REGIME_CASES:
        res = TX.xval_errors(dev, regime, n, plan)
        cells = []
        for layer in layers:
            for q in X.QUANTITIES:
                err, nz, lim = res[layer][q]
                cell = fmt(err / nz)
                if err / nz > worst[layer][0]:
                    worst[layer] = (err / nz, (q, regime, n, plan))
                if err > M.MARGIN * nz:
                    cell += f" ({fmt(M.MARGIN * err / lim)})"
                    if layer != "chain" or (q, regime, n, plan) not in X.FINDINGS:
                        cell += " NOT A DOCUMENTED FINDING"
                cells.append(cell)
        print(f"| {regime} | {n} | {plan} | " + " | ".join(cells) + " |", flush=True)
    for layer in layers:
        print(f"largest ratio, {layer}: {fmt(worst[layer][0])} at {worst[layer][1]}")


def main():
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    dev = torch.device("cuda:0")
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("chain", "all", "both"):
        chain(dev)
    if which in ("pca", "all", "both"):
        pca(dev)
    if which in ("joint", "all"):
        joint(dev)
    if which in ("field", "all"):
        field(dev)
    if which in ("xval", "all"):
        xval(dev)


if __name__ == "__main__":
    main()
