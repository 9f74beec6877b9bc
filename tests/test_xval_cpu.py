"""CPU: the closed form gp_xval implements (tests/_xval_ref.closed_form) against brute-force
refits through oracle.gp_ref.predict, on the inputs of tests/test_gpu_xval.py.  Guards the
formula, not rounding: the two agree to a few 1e-14 on these well-conditioned inputs and the
bounds are 1e-12 max|w| (mean) and 1e-12 s (variance).

At n >= 128 leave-one-out is refitted for a spread of indices only (both ends, the 16- and 128-row
tile edges and every 37th), so the whole file takes seconds; the folds are refitted in full.
"""
import numpy as np
import pytest

import _xval_ref as ref
from oracle import gp_ref


def _agree(p, folds):
    A = gp_ref.gram_ardse(p["X"], p["beta"], p["s"], p["delta"])
    mc, vc = ref.closed_form(A, p["w"], folds, p["shift"])
    mb, vb = ref.brute_force(p["X"], p["w"], p["beta"], p["s"], p["delta"], p["s_pred"], folds)
    assert np.array_equal(np.isnan(mc), np.isnan(mb))
    cov = ~np.isnan(mc)
    assert cov.sum() == sum(len(F) for F in folds)
    em = np.max(np.abs(mc[cov] - mb[cov]))
    ev = np.max(np.abs(vc[cov] - vb[cov]))
    print(f"n={len(p['w'])} mean err {em:.3e} var err {ev:.3e}")
    assert em <= 1e-12 * np.max(np.abs(p["w"]))
    assert ev <= 1e-12 * p["s"]


@pytest.mark.parametrize("n", [1, 2, 17, 128, 129, 200, 513])
@pytest.mark.parametrize("b", [0, 1, 2])
def test_leave_one_out_matches_refits(n, b):
    d = 8 if n >= 128 else 3
    idx = range(n) if n < 128 else sorted(
        set(range(0, n, 37)) | {15, 16, 17, 127, n - 1} | ({128} if n > 128 else set()))
    _agree(ref.problem(n, d, b), [[i] for i in idx])


@pytest.mark.parametrize("n", [200, 513])
def test_folds_match_refits(n):
    _agree(ref.problem(n, 8, 0), ref.mixed_folds(n))


def test_n33_matches_refits():
    p = ref.problem(33, 3, 0)
    _agree(p, [[i] for i in range(33)])
    _agree(p, [list(range(9, 25))])
