"""numpy references of the joint predictive covariance (gp_predict_cov) and of the joint draws
(gp_mvn_draw), and the inputs their tests share.

``closed_form`` restates include/gpfit.h from oracle.gp_ref's Gram and cross-covariance:
C = K** + (s_pred + jitter - s) I - V^T V with V = L^-1 K*.  ``brute_force`` conditions the joint
prior of the n training and m test points through its precision matrix instead:
C = (Sigma^-1)[test, test]^-1, which shares no step with the closed form.
"""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import gp_ref, rng_ref
import _xval_ref

SHAPES = [(1, 1, 3), (17, 5, 3), (129, 17, 8), (200, 130, 8), (513, 257, 8), (64, 33, 11)]


def test_points(n, m, d):
    return np.random.default_rng([n, m, 7]).random((m, d))


def prior(Xs, beta, s, s_pred, jitter=0.0):
    """K** with s_pred + jitter itself on the diagonal."""
    K = gp_ref.gram_ardse(Xs, beta, s, 0.0)
    K[np.diag_indices_from(K)] = s_pred + jitter
    return K


def closed_form(X, Xs, beta, s, delta, s_pred, jitter=0.0):
    """(m, m) joint predictive covariance, exactly symmetric."""
    C = prior(Xs, beta, s, s_pred, jitter)
    if X.shape[0] == 0:
        return C
    L = np.linalg.cholesky(gp_ref.gram_ardse(X, beta, s, delta))
    V = sla.solve_triangular(L, gp_ref.cross_ardse(Xs, X, beta, s).T, lower=True)   # (n, m)
    C = C - V.T @ V
    return 0.5 * (C + C.T)


def joint_prior(X, Xs, beta, s, delta, s_pred, jitter=0.0):
    """The (n + m) x (n + m) prior covariance of (w at X, w at Xs)."""
    n = X.shape[0]
    Ks = gp_ref.cross_ardse(Xs, X, beta, s)                                          # (m, n)
    return np.block([[gp_ref.gram_ardse(X, beta, s, delta), Ks.T],
                     [Ks, prior(Xs, beta, s, s_pred, jitter)]]), n


def brute_force(X, Xs, beta, s, delta, s_pred, jitter=0.0):
    Sigma, n = joint_prior(X, Xs, beta, s, delta, s_pred, jitter)
    return np.linalg.inv(np.linalg.inv(Sigma)[n:, n:])


@functools.lru_cache(maxsize=None)
def reference(n, m, d, b, jitter=0.0):
    """closed_form of problem(n, d, b) at test_points(n, m, d), computed once and shared
    (read-only) between the tests."""
    p = _xval_ref.problem(n, d, b)
    C = closed_form(p["X"], test_points(n, m, d), p["beta"], p["s"], p["delta"], p["s_pred"],
                    jitter)
    C.setflags(write=False)
    return C


def draws(R, mean, seed, offset, nsamp, unit0=0):
    """(batch, nsamp, m): mean_b + tril(R_b) xi with xi elements ((unit0 + b) nsamp + r) m + k of
    rng_ref.normals(., seed, offset); also the magnitude sum |mean_i| + sum_k |R_ik xi_k| that
    scales the tolerance."""
    R = np.asarray(R)
    batch, m, _ = R.shape
    z = rng_ref.normals((unit0 + batch) * nsamp * m, seed, offset)
    z = z.reshape(unit0 + batch, nsamp, m)[unit0:]
    T = np.tril(R)
    mu = np.zeros((batch, m)) if mean is None else np.asarray(mean)
    out = mu[:, None, :] + np.einsum("bik,brk->bri", T, z)
    mag = np.abs(mu)[:, None, :] + np.einsum("bik,brk->bri", np.abs(T), np.abs(z))
    return out, mag
