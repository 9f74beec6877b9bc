"""CPU: the likelihood gradient's reference (tests/_nll_grad_ref.py) checks itself.

The 50-digit gradient agrees with 50-digit central differences of the 50-digit nll in every
entry (delta included), the numpy restatement stays within the figures measured on the three
cases of the module (9.1, 13.0 and 5.1e5 eps of the gross sums: its floating-point order is
LAPACK's, so the bound is those figures with the project's margin), and the committed golden
truths rebuild from their seeds.
"""
import os

import numpy as np
import pytest
from mpmath import mp, mpf

import _nll_grad_ref as R
from _mp_ref import DPS, EPS, MARGIN


@pytest.mark.parametrize("n,d,s,delta", [(7, 3, 0.7, 1e-2), (12, 1, 1.3, 1e-4)])
def test_mp_gradient_against_central_differences(n, d, s, delta):
    X, beta, s, delta, w = R.scattered(n, d, s, delta, 10 + n)
    with mp.workdps(DPS):
        Xm, bt, sm, dm, wm = R._mp_inputs(X, beta, s, delta, w)
        g, _ = R.grad_mp(Xm, bt, sm, dm, wm)
    # the differences at 90 digits with h = 1e-28: truncation (h / delta)^2 ~ 1e-48 relative,
    # rounding 1e-90 / h = 1e-62
    with mp.workdps(90):
        h = mpf(10) ** -28

        def cd(e):
            def at(step):
                b2 = [v + (step if e == 2 + k else 0) for k, v in enumerate(bt)]
                return R.nll_mp(Xm, b2, sm + (step if e == 0 else 0),
                                dm + (step if e == 1 else 0), wm)
            return (at(h) - at(-h)) / (2 * h)

        for e in range(d + 2):
            rel = abs(cd(e) - g[e]) / abs(g[e])
            assert rel <= mpf(10) ** -25, (e, float(rel))


# the LAPACK restatement's measured ratios, in eps of the gross sums
MEASURED = {"scattered_1e-6": 9.1, "scattered_1e-2": 13.0, "c1_grid": 5.1e5}


@pytest.mark.parametrize("case", sorted(R.CPU_CASES))
def test_numpy_restatement_within_its_measured_error(case):
    inp = R.CPU_CASES[case]()
    g, G = R.truth(*inp)
    lap, exp = R.restatement_ratios(*inp, g, G)
    print(f"{case}: lapack {lap / EPS:.3g} eps, explicit {exp / EPS:.3g} eps")
    assert lap <= MARGIN * MEASURED[case] * EPS
    # within the limit the device is held to, which is never below MARGIN x either restatement
    lim = R.limit(*inp, g, G)
    assert lap <= lim and lim >= MARGIN * max(lap, exp) and lim >= MARGIN * R.FLOOR_EPS * EPS
    # and the nll of the restatement is the chain's
    import _mp_ref
    t = _mp_ref.truth(inp[0], np.zeros((0, inp[0].shape[1])), inp[4], inp[1], inp[2], inp[3], 1.0)
    nll = R.grad_lapack(*inp)[0]
    assert t.nll.err(nll) <= 1e-7 * abs(float(t.nll.hi))


def test_gross_sums_bound_the_gradient():
    inp = R.CPU_CASES["scattered_1e-2"]()
    g, G = R.truth(*inp)
    assert np.all(np.abs(g.hi) <= G * (1 + 4 * EPS)) and np.all(G > 0)
    # dNLL/ddelta's sum has one sign per term only where W's diagonal has: G >= |g| is all
    assert G.shape == (inp[0].shape[1] + 2,)


def test_golden_rebuilds_from_its_seeds(golden_dir):
    z = np.load(os.path.join(golden_dir, "nll_grad_truth.npz"))
    assert sorted(z.files) == sorted(nm + "_" + f for nm in R.GOLDEN_CASES for f in
                                     ("g_hi", "g_lo", "G", "lapack", "explicit", "case"))
    name = "n130_d3"
    assert tuple(z[name + "_case"]) == tuple(float(v) for v in R.GOLDEN_CASES[name])
    inp = R.golden_inputs(name)
    g, G = R.truth(*inp)
    np.testing.assert_array_equal(g.hi, z[name + "_g_hi"])
    np.testing.assert_array_equal(g.lo, z[name + "_g_lo"])
    np.testing.assert_array_equal(G, z[name + "_G"])
    # the stored restatement ratios are another BLAS's rounding noise on another machine: a
    # restatement here stays within the limit built from them
    lap, exp = R.restatement_ratios(*inp, g, G)
    assert max(lap, exp) <= R.limit_from(float(z[name + "_lapack"]), float(z[name + "_explicit"]))
    for nm in R.GOLDEN_CASES:
        assert z[nm + "_g_hi"].shape == (R.GOLDEN_CASES[nm][1] + 2,)
    assert os.path.getsize(os.path.join(golden_dir, "nll_grad_truth.npz")) < 16384
