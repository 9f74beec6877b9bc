"""The likelihood gradient at 50 digits (mpmath), its fp64 restatements and the tests' limit.

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.

With NLL = 1/2 w^T K^-1 w + 1/2 log|K|, K = s R + delta I, R_ij = exp(-sum_k beta_k D_ijk^2),
D_ijk = X[i,k] - X[j,k], alpha = K^-1 w and W = K^-1 - alpha alpha^T, the gradient is

    g = [dNLL/ds, dNLL/ddelta, dNLL/dbeta_0 ... dNLL/dbeta_{d-1}]
    dNLL/ds      =  1/2 sum_ij W_ij R_ij
    dNLL/ddelta  =  1/2 sum_i  W_ii
    dNLL/dbeta_k = -1/2 s sum_ij W_ij R_ij D_ijk^2

* ``truth``: g at ``mp.dps = 50`` (the inputs taken as the exact binary values of the fp64
  arrays) as a ``_mp_ref.DD`` pair, and the gross sums G of the same sums with every term's
  absolute value.  The gradient cancels to zero at an optimum, so an error relative to |g| means
  nothing: every error here is ``ratio = max_e |g_got - g_true|_e / G_e``.
* ``grad_lapack``: numpy with LAPACK ``cho_factor`` / ``cho_solve``;  ``grad_explicit``: the
  library's arithmetic, the blocked explicit-inverse factors of ``_mp_ref.explicit_factor``
  and products with them.
* ``limit``: what a device gradient's ratio may reach, built as ``_mp_ref.limit`` builds its
  limits: MARGIN (16, the project's own margin) x the larger of the two restatements' ratios
  against the truth on the same inputs, never below FLOOR_EPS eps.  The ill-conditioned 1-D grid
  is kappa-limited (the LAPACK restatement is 5e5 eps off there), which is why the limit comes
  from the restatements and not from a constant.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
from mpmath import mp, mpf

import _mp_ref
from _mp_ref import DD, DPS, EPS, MARGIN

FLOOR_EPS = 4.0          # the floor of a limit, in eps of G (as _mp_ref.floor_of: 4 eps of scale)


# ------------------------------------------------------------------------------------ inputs
def c2_w(X, seed=1):
    """The C2 recipe's response on a design X (tests/golden/make_golden.py c2_golden)."""
    a = np.random.default_rng(seed).uniform(0, 1, X.shape[1])
    return np.sin(2 * np.pi * X @ a) + 0.1 * np.sum(X * X, axis=1)


def scattered(n, d, s, delta, seed):
    """A scattered design with beta ~ U(0.5, 5) and the C2 response: (X, beta, s, delta, w)."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    beta = rng.uniform(0.5, 5.0, d)
    return X, beta, float(s), float(delta), c2_w(X, seed + 1)


C1_THETA = (1.436, 0.3926)      # near the optimum of BASELINE config 1 (nugget 1e-3)


def c1_grid(n=64, theta=C1_THETA, nugget=1e-3):
    """BASELINE config 1 at ``theta``: x = linspace(1/8, 7/8, n), y = x sin(2 pi x)."""
    X = np.linspace(1 / 8, 7 / 8, n).reshape(n, 1)
    w = (X * np.sin(2 * np.pi * X)).reshape(-1)
    return X, np.array([1.0 / (2.0 * theta[1] ** 2)]), float(theta[0] ** 2), nugget ** 2, w


# The three cases the restatement was measured on (max ratio: 9.1, 13.0 and 5.1e5 eps).
CPU_CASES = {
    "scattered_1e-6": lambda: scattered(65, 8, 1.0, 1e-6, 65),
    "scattered_1e-2": lambda: scattered(65, 8, 1.0, 1e-2, 65),
    "c1_grid": c1_grid,
}

# tests/golden/nll_grad_truth.npz: name -> (n, d, delta, seed); s = 1.
GOLDEN_CASES = {"n130_d3": (130, 3, 1e-2, 130), "n200_d8": (200, 8, 1e-6, 200),
                "n321_d8": (321, 8, 1e-2, 321)}


def golden_inputs(name):
    n, d, delta, seed = GOLDEN_CASES[name]
    return scattered(n, d, 1.0, delta, seed)


# ------------------------------------------------------------------------------------- truth
def _mp_inputs(X, beta, s, delta, w):
    Xm = _mp_ref._rows(X)
    bt = [mpf(float(v)) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
    wm = [mpf(float(v)) for v in np.asarray(w, dtype=np.float64).reshape(-1)]
    return Xm, bt, mpf(float(s)), mpf(float(delta)), wm


def _factor_mp(Xm, bt, sm, dm):
    """R (rows), the Cholesky factor of s R + delta I and the columns of its inverse."""
    n = len(Xm)
    R = [[mpf(1)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            R[i][j] = R[j][i] = _mp_ref.kernel_exp(Xm[i], Xm[j], bt)
    A = [[sm * R[i][j] + (dm if i == j else 0) for j in range(n)] for i in range(n)]
    L = _mp_ref._chol_mp(A)
    return R, L, _mp_ref._linv_mp(L)


def nll_mp(Xm, bt, sm, dm, wm):
    """The NLL from mpf inputs (call under ``mp.workdps``)."""
    n = len(Xm)
    _, L, C = _factor_mp(Xm, bt, sm, dm)
    z = [mp.fdot([C[j][i] for j in range(i + 1)], wm[:i + 1]) for i in range(n)]
    return mp.fdot(z, z) / 2 + mp.fsum(mp.log(L[i][i]) for i in range(n))


def grad_mp(Xm, bt, sm, dm, wm):
    """(g, G) as lists of mpf (call under ``mp.workdps``)."""
    n, d = len(Xm), len(bt)
    R, L, C = _factor_mp(Xm, bt, sm, dm)
    z = [mp.fdot([C[j][i] for j in range(i + 1)], wm[:i + 1]) for i in range(n)]
    alpha = [mp.fdot(C[j][j:], z[j:]) for j in range(n)]
    g = [mpf(0)] * (d + 2)
    G = [mpf(0)] * (d + 2)
    for i in range(n):
        Ci = C[i][i:]
        for j in range(i + 1):
            wij = mp.fdot(Ci, C[j][i:]) - alpha[i] * alpha[j]
            if i == j:
                g[0] += wij
                G[0] += abs(wij)
                g[1] += wij
                G[1] += abs(wij)
                continue
            t = 2 * wij * R[i][j]                   # (i, j) and (j, i)
            g[0] += t
            G[0] += abs(t)
            for k in range(d):
                dk = Xm[i][k] - Xm[j][k]
                g[2 + k] -= sm * t * dk * dk
                G[2 + k] += abs(sm * t * dk * dk)
    return [v / 2 for v in g], [v / 2 for v in G]


def truth(X, beta, s, delta, w):
    """(g, G): the gradient as a DD of d + 2 entries and the gross sums as fp64."""
    with mp.workdps(DPS):
        g, G = grad_mp(*_mp_inputs(X, beta, s, delta, w))
        return DD(g), np.array([float(v) for v in G])


def ratio(got, g: DD, G) -> float:
    """max_e |got - truth|_e / G_e.  Where G_e = 0 the sum has no term (the beta entries at
    n = 1) and the entry must be exactly 0."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    if got.shape != g.hi.shape or not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs((got - g.hi) - g.lo)
    empty = G == 0
    if np.any(err[empty] != 0):
        return float("inf")
    return float(np.max(err[~empty] / G[~empty]))


# ------------------------------------------------------------------------------ restatements
def _rd2(X, beta):
    D2 = (X[:, None, :] - X[None, :, :]) ** 2
    return np.exp(-(D2 @ np.asarray(beta, dtype=np.float64).reshape(-1))), D2


def _sums(Kinv, alpha, R, D2, s):
    W = Kinv - np.outer(alpha, alpha)
    WR = W * R
    return np.concatenate([[0.5 * WR.sum(), 0.5 * np.trace(W)],
                           -0.5 * s * np.einsum("ij,ijk->k", WR, D2)])


def grad_lapack(X, beta, s, delta, w):
    """(nll, g) in fp64 with LAPACK cho_factor / cho_solve."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    R, D2 = _rd2(X, beta)
    c = sla.cho_factor(s * R + delta * np.eye(n), lower=True, check_finite=False)
    alpha = sla.cho_solve(c, w, check_finite=False)
    Kinv = sla.cho_solve(c, np.eye(n), check_finite=False)
    nll = 0.5 * w @ alpha + np.sum(np.log(np.diag(c[0])))
    return float(nll), _sums(Kinv, alpha, R, D2, s)


def grad_explicit(X, beta, s, delta, w, sizes):
    """g in fp64 as the library forms it: blocked explicit-inverse factors, then products."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    R, D2 = _rd2(X, beta)
    _, Li = _mp_ref.explicit_factor(s * R + delta * np.eye(n), sizes)
    return _sums(Li.T @ Li, Li.T @ (Li @ w), R, D2, s)


def restatement_ratios(X, beta, s, delta, w, g: DD, G):
    """(LAPACK, explicit-inverse) ratios against the truth; the explicit one is the larger of
    the library's two blockings."""
    lap = ratio(grad_lapack(X, beta, s, delta, w)[1], g, G)
    exp = max(ratio(grad_explicit(X, beta, s, delta, w, sizes), g, G)
              for sizes in _mp_ref.BLOCKINGS)
    return lap, exp


def limit_from(lap: float, exp: float) -> float:
    return MARGIN * max(lap, exp, FLOOR_EPS * EPS)


def limit(X, beta, s, delta, w, g: DD, G) -> float:
    """The bound on a device gradient's ratio for these inputs."""
    return limit_from(*restatement_ratios(X, beta, s, delta, w, g, G))


# --------------------------------------------------------------------------------- theta maps
def theta_grad(theta, g, ard: bool):
    """The gradient in GPmodule's theta from g = [d/ds, d/ddelta, d/dbeta_k]: s = theta0^2,
    beta_k = 1 / (2 l_k^2), one l for every k unless ``ard``."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    if ard:
        return np.concatenate([[2.0 * theta[0] * g[0]], -g[2:] / theta[1:] ** 3])
    return np.array([2.0 * theta[0] * g[0], -np.sum(g[2:]) / theta[1] ** 3])
