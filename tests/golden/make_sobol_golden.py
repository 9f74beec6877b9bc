"""Regenerate ``sobol_ref_d3_m6.npz`` (run in the build container, NOT on the GPU box).

    python tests/golden/make_sobol_golden.py --reference REFERENCE_ROOT

Imports the reference's own ``src/utils.py`` from the read-only reference tree and calls its
``PCA_saltelli_sensitivity_indices`` with ``bootstrap=False``, n_dim = 3, m = 6 and a fixed
analytic three-output ``func`` that records its inputs (the reference draws an unseeded scrambled
Sobol' design, so the design is whatever ``func`` saw).  Stored, as data only: A, B, the recorded
outputs fA, fB (N, p) and fAB (d, N, p), ``pcvar`` and the four returned arrays.
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_DIM, M_LOG2 = 3, 6
PCVAR = np.array([0.6, 0.3, 0.1])


def func(x):
    """Three analytic outputs of x in [0, 1]^3: an additive one, an interaction, an Ishigami-like
    one."""
    x1, x2, x3 = x[:, 0], x[:, 1], x[:, 2]
    return np.stack([4.0 * x1 + 2.0 * x2 + x3,
                     x1 * x2 + 0.5 * x3 ** 2 + 0.2 * np.sin(2 * np.pi * x1),
                     np.sin(np.pi * (2 * x1 - 1)) + 7.0 * np.sin(np.pi * (2 * x2 - 1)) ** 2
                     + 0.1 * (np.pi * (2 * x3 - 1)) ** 4 * np.sin(np.pi * (2 * x1 - 1))], axis=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the read-only reference tree")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_utils", os.path.join(args.reference, "src", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen, outs = [], []

    def recording(x):
        seen.append(np.array(x, dtype=np.float64))
        outs.append(func(x))
        return outs[-1]

    first, total, gfirst, gtotal, res = mod.PCA_saltelli_sensitivity_indices(
        recording, N_DIM, M_LOG2, PCVAR, bootstrap=False)
    assert res is None and len(seen) == N_DIM + 2
    np.savez_compressed(os.path.join(HERE, "sobol_ref_d3_m6.npz"), A=seen[0], B=seen[1],
                        fA=outs[0], fB=outs[1], fAB=np.stack(outs[2:]), pcvar=PCVAR,
                        first_order=first, total_index=total, gen_first_order=gfirst,
                        gen_total_index=gtotal)
    print("sobol golden written: N =", seen[0].shape[0], "first_order", first.shape)


if __name__ == "__main__":
    main()
