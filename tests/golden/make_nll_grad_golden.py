"""Regenerate ``nll_grad_truth.npz`` (CPU only; n = 321 takes a few minutes of mpmath).

    python tests/golden/make_nll_grad_golden.py

For every case of ``_nll_grad_ref.GOLDEN_CASES`` (scattered designs, beta ~ U(0.5, 5), s = 1,
the C2 response) the file holds the 50-digit gradient as a double-double pair (``*_g_hi``,
``*_g_lo``), the gross sums ``*_G``, the ratios of the two fp64 restatements against that truth
(``*_lapack``, ``*_explicit``) and the case's ``(n, d, delta, seed)`` (``*_case``), from which
``_nll_grad_ref.golden_inputs`` rebuilds the inputs.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _nll_grad_ref as R  # noqa: E402


def main() -> None:
    out = {}
    for name, case in R.GOLDEN_CASES.items():
        t0 = time.time()
        inp = R.golden_inputs(name)
        g, G = R.truth(*inp)
        lap, exp = R.restatement_ratios(*inp, g, G)
        out[name + "_g_hi"], out[name + "_g_lo"], out[name + "_G"] = g.hi, g.lo, G
        out[name + "_lapack"], out[name + "_explicit"] = np.float64(lap), np.float64(exp)
        out[name + "_case"] = np.array(case, dtype=np.float64)
        print(f"{name}: lapack {lap / R.EPS:.1f} eps, explicit {exp / R.EPS:.1f} eps, "
              f"{time.time() - t0:.0f} s", flush=True)
    np.savez(os.path.join(HERE, "nll_grad_truth.npz"), **out)


if __name__ == "__main__":
    main()
