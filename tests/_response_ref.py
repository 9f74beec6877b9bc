"""numpy references of the mean-response surfaces (gp_mean_response), written from the formulas
of include/gpfit.h: ``direct`` materialises the test points of every grid node and averages the
posterior mean over them (what the reference's drivers do through the emulator), ``bound`` is the
sum of absolute terms that the rounding-error bounds of the GPU tests scale with.
"""
import numpy as np

from oracle import gp_ref

CYCLIC, ASCENDING = "cyclic", "ascending"


def free_dims(effect):
    return [int(k) for k in np.atleast_1d(effect)]


def int_dims(effect, order, d):
    """The dimension integration column c takes, for c = 0 .. d - nfree - 1."""
    free = free_dims(effect)
    if order == CYCLIC:
        assert len(free) == 1
        return [(free[0] + 1 + c) % d for c in range(d - 1)]
    assert order == ASCENDING
    return [k for k in range(d) if k not in free]


def points(effect, order, t1, t2, Xint, d):
    """The explicit test points of one grid node: x_d1 = t1, x_d2 = t2 (None for a main effect)
    and the columns of Xint in the other dimensions -- (I, d), or (1, d) when every dimension is
    free."""
    free = free_dims(effect)
    cols = int_dims(effect, order, d)
    rows = 1 if not cols else np.asarray(Xint).shape[0]
    P = np.zeros((rows, d))
    if cols:
        P[:, cols] = np.asarray(Xint)[:, :len(cols)]
    P[:, free[0]] = t1
    if len(free) == 2:
        P[:, free[1]] = t2
    return P


def _grid(effect, t1, t2):
    t1 = np.asarray(t1, dtype=np.float64).reshape(-1)
    t2 = [None] if len(free_dims(effect)) == 1 else np.asarray(t2, dtype=np.float64).reshape(-1)
    return t1, t2


def direct(X, alpha, beta, s, effect, order, t1, t2, Xint):
    """The surface of one effect, (T1,) or (T2, T1): the mean over the integration points of
    cross_ardse(points) @ alpha at every node."""
    d = X.shape[1]
    t1, t2 = _grid(effect, t1, t2)
    P = np.concatenate([points(effect, order, v1, v2, Xint, d) for v2 in t2 for v1 in t1])
    mean = gp_ref.cross_ardse(P, X, beta, s) @ alpha
    out = mean.reshape(len(t2), len(t1), -1).mean(axis=2)
    return out[0] if t2[0] is None else out


def predicted(X, w, beta, s, delta, effect, order, t1, t2, Xint):
    """The same through the oracle's own solve: gp_ref.predict at the points of every node,
    averaged (one predict call over all nodes)."""
    d = X.shape[1]
    t1, t2 = _grid(effect, t1, t2)
    P = np.concatenate([points(effect, order, v1, v2, Xint, d) for v2 in t2 for v1 in t1])
    mean, _ = gp_ref.predict(X, P, w, beta, s, delta)
    out = mean.reshape(len(t2), len(t1), -1).mean(axis=2)
    return out[0] if t2[0] is None else out


def bound(X, alpha, beta, s, effect, order, t1, t2, Xint):
    """s sum_n |alpha_n| M_n E1[n, a1] E2[n, a2], the shape of ``direct``."""
    d = X.shape[1]
    free = free_dims(effect)
    beta = np.asarray(beta, dtype=np.float64)
    t1, t2 = _grid(effect, t1, t2)
    cols = int_dims(effect, order, d)
    M = np.ones(X.shape[0])
    if cols:
        bi = np.zeros(d)
        bi[cols] = beta[cols]
        M = gp_ref.cross_ardse(points(effect, order, 0.0, 0.0 if len(free) == 2 else None,
                                      Xint, d), X, bi, 1.0).mean(axis=0)
    E1 = np.exp(-beta[free[0]] * (X[:, free[0]][:, None] - t1[None, :]) ** 2)      # (n, T1)
    g = s * np.abs(alpha) * M
    if len(free) == 1:
        return g @ E1
    E2 = np.exp(-beta[free[1]] * (X[:, free[1]][:, None] - t2[None, :]) ** 2)      # (n, T2)
    return (g[:, None] * E2).T @ E1
