"""Print DESIGN.md section 7's table: the measured error / noise of every chain quantity per
(regime, n), worst over the entry points that produce it and over the factorisation paths, from
the helpers of tests/test_gpu_extremes.py.  Needs a HIP device.  Entries above 16 also show, in
parentheses, error / (noise + explicit-inverse term): they must be in tests/_mp_ref.FINDINGS.

    python tools/extremes_ratios.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import _mp_ref as M  # noqa: E402
import test_gpu_extremes as T  # noqa: E402


def fmt(x):
    return f"{x:.2g}" if x < 100 else f"{round(x)}"


def main():
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    dev = torch.device("cuda:0")
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


if __name__ == "__main__":
    main()
