"""CPU: the references of gp_sobol_exact (tests/_sobol_exact_ref.py) stand on their own -- the
50-digit truth against quadrature of the definitions, the fp64 restatement against the truth
(which fixes C0, the constant of the device's limit), the analytic special cases, and the seeded
Saltelli consistency case of tests/test_gpu_sobol_exact.py with the numpy oracle in place of the
device.  No device work happens here.
"""
import numpy as np
import pytest

import _sobol_exact_ref as R
import _sobol_ref as sref
from oracle import gp_ref


def test_truth_one_dimensional_integrals_against_mp_quad():
    """The closed forms of I_k and J_k against mp.quad of their integrands: inside the box,
    outside it on either side (same-sign brackets), sharp and flat kernels."""
    for b, b2, x, x2, lo, hi in [(1.3, 0.7, 0.2, 0.9, 0.0, 1.0), (4.0, 4.0, 0.1, 0.1, 0.3, 0.6),
                                 (2.0, 3.0, 0.9, 0.95, 0.3, 0.6), (1e4, 1e4, 0.5, 0.51, 0.0, 1.0),
                                 (1e-6, 1e-6, 0.3, 0.8, 0.0, 1.0), (0.5, 5e3, 0.4, 0.7, -1.0, 2.0)]:
        dI, dJ = R.mp_quad_check(b, b2, x, x2, lo, hi)
        assert dI <= 1e-30 and dJ <= 1e-30, (b, b2, x, x2, lo, hi, dI, dJ)


@pytest.mark.parametrize("regime", ["plain", "subbox"])
@pytest.mark.parametrize("n,d,G,M", [(1, 1, 1, 1), (7, 1, 1, 2), (5, 2, 2, 1), (24, 3, 1, 2),
                                     (9, 2, 1, 2)])
def test_truth_against_quadrature(regime, n, d, G, M):
    """E, Q_tot, Q_main_i and Q_not_i of the truth against 40-point tensor Gauss-Legendre
    quadrature of f_u f_v, E[f_u|x_i] E[f_v|x_i] and E[f_u|x_~i] E[f_v|x_~i]: nothing of the closed
    form enters the quadrature.  The integrands are entire with beta <= 5 on a box of width <= 1,
    so 40 nodes converge far below fp64; what is left is the rounding of sums of 40^d products
    with the majorant's scale, held to 1e-12 A (a definition slip is O(A))."""
    X, beta, s, alpha, lo, hi = R.make_case(n, d, G * M, regime, 0)
    tr = R.mp_moments(X, alpha, beta, s, M, lo, hi)
    q = R.quad_moments(X, alpha, beta, s, M, lo, hi)
    rE = R.err_ratio(q["E"], tr["E"], tr["AE"])
    rQ = R.err_ratio(q["Q"], tr["Q"], tr["AQ"])
    print(f"{regime} n={n} d={d} M={M}: quadrature - truth {rE:.2f} eps AE, {rQ:.2f} eps AQ")
    assert rE * R.EPS <= 1e-12 and rQ * R.EPS <= 1e-12


@pytest.mark.parametrize("regime", R.REGIMES)
def test_restatement_against_truth(regime):
    """The fp64 restatement's own error over the tiny cases, in units of eps A: this is what
    fixes C0 (tests/_sobol_exact_ref.py), so it must stay below it."""
    wE = wQ = 0.0
    for n, d, G, M in R.TINY_CASES:
        for seed in (0, 1):
            X, beta, s, alpha, lo, hi = R.make_case(n, d, G * M, regime, seed)
            tr = R.mp_moments(X, alpha, beta, s, M, lo, hi)
            ref = R.np_moments(X, alpha, beta, s, M, lo, hi)
            wE = max(wE, R.err_ratio(ref["E"], tr["E"], tr["AE"]))
            wQ = max(wQ, R.err_ratio(ref["Q"], tr["Q"], tr["AQ"]))
            assert np.isfinite(ref["Q"]).all()
            np.testing.assert_array_equal(ref["Q"], np.swapaxes(ref["Q"], 1, 2))
    print(f"{regime}: restatement - truth <= {wE:.2f} eps AE, {wQ:.2f} eps AQ (C0 = {R.C0})")
    assert wE <= R.C0 and wQ <= R.C0


def test_one_dimension_gives_one():
    """d = 1: every bit of variance is x_0's, S = T = 1."""
    X, beta, s, alpha = R.conditioned_case(20, 1, 2, seed=1)
    for M in (1, 2):
        ref = R.np_moments(X, alpha, beta, s, M)
        _, V, first, total = R.np_indices(ref["E"], ref["Q"], M)
        tf, tt = R.index_tolerance(ref, M, R.C0 * R.EPS)
        assert (V > 0).all()
        assert (np.abs(first - 1) <= tf).all() and (np.abs(total - 1) <= tt).all()


def test_additive_function_has_no_interactions():
    """An additive f has S_i = T_i.  A single unit cannot be additive (its mean is a sum of
    products over ALL dimensions: points that differ from a base point in one coordinate still
    multiply the base point's sections in the others), so the toy is a group of d units, unit a
    with beta = 1e-9 in every dimension but a: f_a depends on x_k, k != a, through factors in
    [1 - 1e-9, 1], and the group mean f = (1/d) sum_a f_a is additive up to a part of sup norm
    <= (d - 1) 1e-9 max|f_a|.  Its variance, <= ((d - 1) 1e-9 max|f_a|)^2, is all T_i - S_i can
    hold beside the rounding tolerance."""
    n, d = 10, 3
    rng = np.random.default_rng(5)
    X = rng.random((n, d))
    beta = np.full((d, d), 1e-9)
    beta[np.arange(d), np.arange(d)] = rng.uniform(0.5, 5.0, d)
    s = np.ones(d)
    alpha = rng.standard_normal((d, n))
    ref = R.np_moments(X, alpha, beta, s, d)
    _, V, first, total = R.np_indices(ref["E"], ref["Q"], d)
    tf, tt = R.index_tolerance(ref, d, R.C0 * R.EPS)
    fmax = np.abs(alpha).sum(1).max()
    slack = ((d - 1) * 1e-9 * fmax) ** 2 / V[0]
    print(f"additive toy: V {V[0]:.3e} S {first[0]} T {total[0]} tol {tf[0] + tt[0]} "
          f"non-additive part <= {slack:.1e}")
    assert V[0] > 1e-3
    assert (np.abs(total - first) <= tf + tt + slack).all()
    assert abs(first.sum() - 1) <= tf.sum() + slack
    assert (first > 1e-4).all()                         # every dimension carries variance


def test_indices_of_a_product_function():
    """n = 1: f = s alpha prod_k h_k(x_k), whose indices are known in closed form from the
    one-dimensional moments m_k = E h_k, v_k = E h_k^2: V = prod v - prod m^2,
    S_i = (v_i / m_i^2 - 1) prod m^2 / V, T_i = (1 - m_i^2 / v_i) prod v / V."""
    import mpmath as mp
    X, beta, s, alpha, lo, hi = R.make_case(1, 3, 1, "plain", 4)
    tr = R.mp_moments(X, alpha, beta, s, 1, lo, hi)
    with mp.workdps(50):
        E, Q = tr["E"][0], tr["Q"][0, 0, 0]
        m = [None] * 3
        v = [None] * 3
        for k in range(3):
            b, x = mp.mpf(float(beta[0, k])), mp.mpf(float(X[0, k]))
            m[k] = mp.quad(lambda t: mp.exp(-b * (t - x) ** 2), [0, x, 1])
            v[k] = mp.quad(lambda t: mp.exp(-2 * b * (t - x) ** 2), [0, x, 1])
        c2 = (mp.mpf(float(s[0])) * mp.mpf(float(alpha[0, 0]))) ** 2
        pm2, pv = c2 * mp.fprod(m) ** 2, c2 * mp.fprod(v)
        V = Q[0] - E ** 2
        assert abs(V - (pv - pm2)) <= mp.mpf(10) ** -40 * pv
        for i in range(3):
            S = (Q[1 + i] - E ** 2) / V
            T = (Q[0] - Q[4 + i]) / V
            assert abs(S - (v[i] / m[i] ** 2 - 1) * pm2 / V) <= mp.mpf(10) ** -35
            assert abs(T - (1 - m[i] ** 2 / v[i]) * pv / V) <= mp.mpf(10) ** -35


def test_saltelli_consistency_with_the_numpy_oracle():
    """The consistency case of tests/test_gpu_sobol_exact.py on the host: the Saltelli estimate
    of the small emulator's mean function from the seeded design (oracle.gp_ref predictions, the
    estimators and the Philox resamples of tests/_sobol_ref.py) against the closed form
    (np_moments on numpy's own alpha).  Every exact index lies within 6 bootstrap standard errors
    of the estimate for the chosen seed: the margin the device is held to is met by the
    references alone."""
    from scipy.stats import qmc
    em = R.small_emulator()
    t, K, samples = em["t"], em["K"], em["samples"]
    n, d, P, S = em["n"], em["d"], em["P"], em["S"]
    _, _, y_std = gp_ref.standardize(em["y"])
    w_hat = gp_ref.pc_weights(y_std, K)
    lam = np.diag(K @ K.T)
    beta, s, delta, _ = gp_ref.sepia_gp_params(samples, lam, d, P, True)
    # exact: units (j, a), the S samples of a PC consecutive
    alpha = np.stack([R.gp_alpha(t, beta[a, j], s[a, j], delta[a, j], w_hat[:, j])
                      for j in range(P) for a in range(S)])
    ref = R.np_moments(t, alpha, R.group_by_pc(beta.reshape(S * P, d), S, P),
                       R.group_by_pc(s.reshape(-1), S, P), S)
    _, V, first, total = R.np_indices(ref["E"], ref["Q"], S)
    assert (V > 0).all()
    gfirst, gtotal = em["pcvar"] @ first, em["pcvar"] @ total
    # Saltelli: the design of sensitivity.saltelli_design, func = mean over the samples
    AB = qmc.Sobol(d=2 * d, seed=R.SALTELLI_SEED).random_base2(m=R.SALTELLI_M)
    A, B = AB[:, d:], AB[:, :d]
    N = A.shape[0]

    def func(x):
        return gp_ref.sepia_predict_w(t, x, w_hat, samples, lam)[0].mean(0)
    fA, fB = func(A), func(B)
    fAB = np.empty((d, N, P))
    for i in range(d):
        C = B.copy()
        C[:, i] = A[:, i]
        fAB[i] = func(C)
    a, b, ab = sref.to_output_major(fA, fB, fAB)
    est = sref.replicates(a, b, ab, np.arange(N)[None], em["pcvar"])
    boot = sref.replicates(a, b, ab, sref.philox_rows(N, N, R.SALTELLI_RESAMPLES,
                                                      R.SALTELLI_SEED), em["pcvar"], clamp=True)
    for name, exact in (("first", first), ("total", total), ("gfirst", gfirst),
                        ("gtotal", gtotal)):
        se = boot[name].std(0, ddof=1)
        z, ok = R.within_margin(exact, est[name][0], se)
        print(f"{name}: exact {np.round(exact, 4).tolist()} estimate "
              f"{np.round(est[name][0], 4).tolist()} worst z {z.max():.2f}")
        assert ok, (name, z)
