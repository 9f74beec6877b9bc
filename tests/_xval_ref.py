"""numpy references of the cross-validated predictions (gp_xval) and the inputs its tests share.

``closed_form`` restates the formulas of include/gpfit.h in numpy from the Gram matrix;
``brute_force`` refits: it removes the fold from the design and predicts the removed points with
``oracle.gp_ref.predict``, which is what SEPIA's SepiaXvalEmulatorPrediction does per fold.
"""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import gp_ref

S0 = 1.3


def problem(n, d, b=0):
    """Problem ``b`` on the design X = default_rng(n).random((n, d)): beta ~ U(0.5, 5), s = 1.3
    (+ 0.2 per problem), delta alternating 1e-2 / 1e-4, s_pred = s + 0.4 delta and
    w = sin(2 pi X a) + 0.1 |x|^2."""
    X = np.random.default_rng(n).random((n, d))
    rng = np.random.default_rng([n, d, b])
    beta = rng.uniform(0.5, 5.0, d)
    a = rng.uniform(0.0, 1.0, d)
    s = S0 + 0.2 * b
    delta = (1e-2, 1e-4)[b % 2]
    w = np.sin(2 * np.pi * X @ a) + 0.1 * np.sum(X * X, axis=1)
    return dict(X=X, beta=beta, s=s, delta=delta, s_pred=s + 0.4 * delta, w=w,
                shift=s + delta - (s + 0.4 * delta))


def mixed_folds(n, seed=0):
    """Folds of 1, 2, 15, 16, 17, 63 and 64 indices drawn from a permutation of range(n) (n >=
    178), every other one sorted; the remaining indices are in no fold."""
    perm = np.random.default_rng([n, seed]).permutation(n)
    folds, at = [], 0
    for k, f in enumerate((1, 2, 15, 16, 17, 63, 64)):
        F = perm[at:at + f]
        at += f
        folds.append([int(i) for i in (np.sort(F) if k % 2 else F)])
    return folds


def closed_form(A, w, folds, shift):
    """(mean, var), each (n,), NaN where no fold covers: for F in folds, with Q = A^-1,
    mean_F = w_F - Q_FF^-1 (Q w)_F and var_F = diag(Q_FF^-1) - shift."""
    n = A.shape[0]
    L = np.linalg.cholesky(A)
    Linv = sla.solve_triangular(L, np.eye(n), lower=True)
    Q = Linv.T @ Linv
    alpha = Linv.T @ (Linv @ w)
    mean = np.full(n, np.nan)
    var = np.full(n, np.nan)
    for F in (([i] for i in range(n)) if folds is None else folds):
        F = np.asarray(F, dtype=int)
        C = np.linalg.inv(Q[np.ix_(F, F)])
        mean[F] = w[F] - C @ alpha[F]
        var[F] = np.diag(C) - shift
    return mean, var


def brute_force(X, w, beta, s, delta, s_pred, folds):
    """The same by refitting: the GP on the design without F, predicting at X[F] with s_pred on
    the diagonal (an empty remainder predicts the prior: mean 0, variance s_pred)."""
    n = X.shape[0]
    mean = np.full(n, np.nan)
    var = np.full(n, np.nan)
    for F in (([i] for i in range(n)) if folds is None else folds):
        F = np.asarray(F, dtype=int)
        rest = np.setdiff1d(np.arange(n), F)
        if rest.size == 0:
            mean[F], var[F] = 0.0, s_pred
            continue
        mean[F], var[F] = gp_ref.predict(X[rest], X[F], w[rest], beta, s, delta, s_pred)
    return mean, var


@functools.lru_cache(maxsize=None)
def reference(n, d, b, fold_key):
    """closed_form of problem(n, d, b) for ``fold_key`` (None, or a tuple of tuples), computed
    once and shared (read-only) between the tests."""
    p = problem(n, d, b)
    A = gp_ref.gram_ardse(p["X"], p["beta"], p["s"], p["delta"])
    folds = None if fold_key is None else [list(F) for F in fold_key]
    mean, var = closed_form(A, p["w"], folds, p["shift"])
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


def key(folds):
    return None if folds is None else tuple(tuple(F) for F in folds)
