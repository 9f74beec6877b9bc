"""CPU: the numpy reference of the joint predictive covariance (tests/_joint_ref.closed_form)
against conditioning the (n + m)-point joint prior by brute force, and at n = 17, m = 5 against
mpmath at 50 digits.  The GPU tests compare gp_predict_cov with this reference."""
import numpy as np
import pytest

from oracle import gp_ref
import _joint_ref
import _xval_ref

EPS = 2.0 ** -52


def _inputs(n, m, d, b):
    p = _xval_ref.problem(n, d, b)
    return p, _joint_ref.test_points(n, m, d)


@pytest.mark.parametrize("n,m,d", [(1, 1, 3), (17, 5, 3), (129, 17, 8), (64, 33, 11)])
@pytest.mark.parametrize("b", [0, 1, 2])
def test_closed_form_matches_conditioning_the_joint_prior(n, m, d, b):
    """The precision-matrix route inverts the joint prior Sigma and then its test block, so its
    error is bounded by a small multiple of cond(Sigma) eps |C|; |C| <= s_pred.  The factor 50
    covers the two inversions' growth (each a few n eps cond)."""
    p, Xs = _inputs(n, m, d, b)
    args = (p["X"], Xs, p["beta"], p["s"], p["delta"], p["s_pred"])
    C = _joint_ref.closed_form(*args)
    B = _joint_ref.brute_force(*args)
    Sigma, _ = _joint_ref.joint_prior(*args)
    bound = 50 * np.linalg.cond(Sigma) * EPS * p["s_pred"]
    err = float(np.max(np.abs(C - B)))
    print(f"n={n} m={m} b={b}: |closed - brute| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(C, C.T)
    # the diagonal is gp_ref.predict's marginal variance
    _, var = gp_ref.predict(p["X"], Xs, p["w"], p["beta"], p["s"], p["delta"], p["s_pred"])
    assert np.max(np.abs(np.diag(C) - var)) <= 1e-11 * p["s"]


def test_no_training_points_gives_the_prior():
    p, Xs = _inputs(17, 5, 3, 0)
    C = _joint_ref.closed_form(p["X"][:0], Xs, p["beta"], p["s"], p["delta"], p["s_pred"], 0.25)
    assert np.array_equal(np.diag(C), np.full(5, p["s_pred"] + 0.25))
    assert np.array_equal(C, _joint_ref.prior(Xs, p["beta"], p["s"], p["s_pred"], 0.25))


@pytest.mark.parametrize("b", [0, 1, 2])
def test_closed_form_against_mpmath_50_digits(b):
    """n = 17, m = 5: the same formula with every step (exponentials, solve, products) at 50
    digits from the same fp64 inputs.  The fp64 closed form loses cond(A) eps s at most a small
    multiple of times (cond(A) <= 1e4 here: about 1.5e-12 s); 1e-11 s leaves that multiple."""
    mp = pytest.importorskip("mpmath")
    n, m, d = 17, 5, 3
    p, Xs = _inputs(n, m, d, b)
    X, beta, s, delta, sp = p["X"], p["beta"], p["s"], p["delta"], p["s_pred"]
    A = gp_ref.gram_ardse(X, beta, s, delta)
    assert np.linalg.cond(A) <= 1e4
    with mp.workdps(50):
        f = lambda v: mp.mpf(float(v))                                        # noqa: E731
        k = lambda a, c: f(s) * mp.exp(-sum(f(beta[q]) * (f(a[q]) - f(c[q])) ** 2   # noqa: E731
                                            for q in range(d)))
        Amp = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                Amp[i, j] = k(X[i], X[j]) + (f(delta) if i == j else 0)
        Ks = mp.matrix(n, m)
        for i in range(n):
            for j in range(m):
                Ks[i, j] = k(X[i], Xs[j])
        Sol = mp.matrix(n, m)
        for j in range(m):                       # lu_solve takes one right-hand side
            Sol[:, j] = mp.lu_solve(Amp, Ks[:, j])
        Q = Ks.T * Sol
        Cmp = np.empty((m, m))
        worst = 0.0
        C = _joint_ref.closed_form(X, Xs, beta, s, delta, sp, 1e-3)
        for i in range(m):
            for j in range(m):
                pr = (f(sp) + f(1e-3)) if i == j else k(Xs[i], Xs[j])
                worst = max(worst, float(abs(pr - Q[i, j] - f(C[i, j]))))
                Cmp[i, j] = float(pr - Q[i, j])
    print(f"b={b}: |closed - mpmath| = {worst:.3e} ({worst / s:.3e} s)")
    assert worst <= 1e-11 * s
    assert np.all(np.linalg.eigvalsh(Cmp) > 0)


def test_draw_reference_layout():
    """draws(): unit0 selects a problem's slice of the stream, and a split batch equals one."""
    rng = np.random.default_rng(5)
    R = rng.standard_normal((2, 4, 4))
    mean = rng.standard_normal((2, 4))
    both, mag = _joint_ref.draws(R, mean, 11, 3, 3)
    one, _ = _joint_ref.draws(R[1:], mean[1:], 11, 3, 3, unit0=1)
    assert np.array_equal(both[1:], one)
    from oracle import rng_ref
    z = rng_ref.normals(2 * 3 * 4, 11, 3).reshape(2, 3, 4)
    assert np.array_equal(both[0, 2], mean[0] + np.tril(R[0]) @ z[0, 2])
    assert np.all(mag >= np.abs(both) - 1e-15)
