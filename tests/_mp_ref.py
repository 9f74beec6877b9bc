"""The GP chain at 50 digits (mpmath), the fp64 noise level per regime, and the regimes.

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.  Three things live here.

* ``truth``: Gram -> column Cholesky -> L^-1 -> logdet, z, nll, alpha -> predictive mean and
  variance at ``mp.dps = 50``, the inputs taken as the exact binary values of the fp64 arrays.
  Every result is kept as a double-double pair (``DD``: hi = the truth rounded to fp64, lo = the
  rest), so ``DD.err(x)`` is the error of an fp64 array against the truth, not against the
  truth's own rounding.
* ``problem`` / ``REGIMES`` / ``SIZES``: the hyperparameter regimes the sampler can reach (flat,
  sharp, mixed, an ill-conditioned 1-D grid, d = 12, d = 32 = GPFIT_MAX_DIM) at the sizes that
  cross every 64-tile edge of the 128 pad.
* ``noise``: what fp64 itself delivers for a quantity in a regime -- the largest error against
  the truth over an ensemble of equally valid fp64 restatements (``oracle.gp_ref``'s formulas on
  the design as given and on 8 seeded permutations of the training points, each with the
  oracle's Gram and with a Gram formed in the device's order), never below 4 eps of the
  quantity's scale.  A test then asks ``error <= MARGIN * noise``.  Only at the entries of
  ``FINDINGS`` (the 1-D grid from n = 64 on, where the device was measured above that) the
  bound is ``MARGIN * (noise + explicit-inverse term)``: what the library's documented
  arithmetic (products with explicit block inverses, never a substitution) adds on
  ill-conditioned diagonal blocks, see ``explicit_inverse_term``.

  alpha, mean, var, logdet and nll do not depend on the order of the training points (alpha
  after un-permuting), so every member is compared with the one truth.  L, L^-1 and z do: a
  permuted member is compared with an extended-precision (64-bit significand) factorisation
  of the equally permuted truth Gram, see ``factor_extended``.

``device_gram`` / ``bound_rel`` restate ``ardse_kernel``'s order of operations (sq = sqrt(beta),
dt = sq xa - sq xb, a chain of dt^2, then exp and the scale) and the bound on a kernel value's
relative error that order implies; see ``bound_rel``.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla
from mpmath import mp, mpf

from oracle import gp_ref

DPS = 50
EPS = float(np.finfo(np.float64).eps)          # 2^-52
TINY = float(2.0 ** -1074)                     # the smallest subnormal
MARGIN = 16.0
NPERM = 8

SIZES = (1, 5, 64, 65, 130)
REGIMES = ("mid", "flat", "sharp", "mixed", "grid", "d12", "d32")
D8 = ("mid", "flat", "sharp", "mixed")        # share X: one batch of 4 on the device
GROUPS = {"d8": D8, "grid": ("grid",), "d12": ("d12",), "d32": ("d32",)}
QUANTITIES = ("L", "Linv", "logdet", "z", "nll", "alpha", "mean", "var")
ORDER_DEPENDENT = ("L", "Linv", "z")


def group_of(regime: str) -> str:
    return "d8" if regime in D8 else regime


# ------------------------------------------------------------------------------ double-double
class DD:
    """A 50-digit array kept as hi + lo in fp64 (hi the rounded truth)."""

    def __init__(self, vals, shape=None):
        flat = list(vals)
        hi = np.array([float(v) for v in flat], dtype=np.float64)
        lo = np.array([float(v - mpf(h)) for v, h in zip(flat, hi.tolist())], dtype=np.float64)
        self.hi = hi.reshape(shape) if shape is not None else hi
        self.lo = lo.reshape(shape) if shape is not None else lo

    def err(self, x) -> float:
        """max |x - truth| (x - hi is exact for x within a factor 2 of hi)."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != self.hi.shape:
            raise ValueError(f"shape {x.shape} against truth {self.hi.shape}")
        if x.size == 0:
            return 0.0
        e = np.abs((x - self.hi) - self.lo)
        return float(np.max(e)) if np.all(np.isfinite(e)) else float("inf")

    def scale(self) -> float:
        return float(np.max(np.abs(self.hi))) if self.hi.size else 0.0

    def take(self, idx):
        out = DD.__new__(DD)
        out.hi, out.lo = self.hi[idx], self.lo[idx]
        return out


# ------------------------------------------------------------------------------------- truth
def _rows(a):
    return [[mpf(v) for v in row] for row in np.asarray(a, dtype=np.float64).tolist()]


def kernel_exp(a, b, beta):
    """exp(-sum_k beta_k (a_k - b_k)^2) as an mpf (call under ``mp.workdps(DPS)``)."""
    acc = mpf(0)
    for x, y, bk in zip(a, b, beta):
        t = x - y
        acc += bk * t * t
    return mp.exp(-acc)


def kernel_values(XA, XB, beta, s=1.0):
    """s exp(-sum_k beta_k (xa_k - xb_k)^2) for every pair, a list of rows of mpf."""
    with mp.workdps(DPS):
        A, B = _rows(XA), _rows(XB)
        bt = [mpf(float(v)) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
        sm = mpf(float(s))
        return [[sm * kernel_exp(a, b, bt) for b in B] for a in A]


def _chol_mp(A):
    """Plain column Cholesky of the lower triangle of A (rows of mpf): L as rows."""
    n = len(A)
    L = [[mpf(0)] * n for _ in range(n)]
    for j in range(n):
        Lj = L[j]
        Lj[j] = mp.sqrt(A[j][j] - mp.fdot(Lj[:j], Lj[:j]))
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], Lj[:j])) / Lj[j]
    return L


def _linv_mp(L):
    """L^-1 by forward substitution, as columns C[j][i] = (L^-1)[i][j]."""
    n = len(L)
    C = []
    for j in range(n):
        c = [mpf(0)] * n
        c[j] = 1 / L[j][j]
        for i in range(j + 1, n):
            c[i] = -mp.fdot(L[i][j:i], c[j:i]) / L[i][i]
        C.append(c)
    return C


class Truth:
    """The chain's quantities as DD arrays (matrices in logical row-major [i][j])."""


def _factor_truth(A, w):
    """L, L^-1, z (DD) and the mpf rows / columns, from a Gram given as rows of mpf."""
    n = len(A)
    L = _chol_mp(A)
    C = _linv_mp(L)
    R = [[C[j][i] for j in range(n)] for i in range(n)]          # rows of L^-1
    z = [mp.fdot(R[i][:i + 1], w[:i + 1]) for i in range(n)]
    return L, C, R, z


def truth(X, Xs, w, beta, s, delta, s_pred):
    """The whole chain at 50 digits.  X (n, d), Xs (m, d), w (n,), beta (d,); scalars s, delta,
    s_pred.  Returns a :class:`Truth` with DD fields A, L, Linv, logdet, z, nll, alpha, mean,
    var, and ``w_mp`` (the exact w as mpf)."""
    X = np.asarray(X, dtype=np.float64)
    Xs = np.asarray(Xs, dtype=np.float64)
    n, m = X.shape[0], Xs.shape[0]
    with mp.workdps(DPS):
        Xm, Xsm = _rows(X), _rows(Xs)
        bt = [mpf(float(v)) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
        wm = [mpf(float(v)) for v in np.asarray(w, dtype=np.float64).reshape(-1)]
        sm, dm, spm = mpf(float(s)), mpf(float(delta)), mpf(float(s_pred))
        A = [[mpf(0)] * n for _ in range(n)]
        for i in range(n):
            for j in range(i):
                A[i][j] = A[j][i] = sm * kernel_exp(Xm[i], Xm[j], bt)
            A[i][i] = sm + dm
        L, C, R, z = _factor_truth(A, wm)
        logdet = 2 * mp.fsum(mp.log(L[i][i]) for i in range(n))
        nll = mp.fdot(z, z) / 2 + logdet / 2
        alpha = [mp.fdot(C[j][j:], z[j:]) for j in range(n)]
        mean, var = [], []
        for q in range(m):
            k = [sm * kernel_exp(Xsm[q], Xm[i], bt) for i in range(n)]
            mean.append(mp.fdot(k, alpha))
            v = [mp.fdot(R[i][:i + 1], k[:i + 1]) for i in range(n)]
            var.append(spm - mp.fdot(v, v))
        t = Truth()
        t.n, t.m = n, m
        t.A = DD((A[i][j] for i in range(n) for j in range(n)), (n, n))
        t.L = DD((L[i][j] for i in range(n) for j in range(n)), (n, n))
        t.Linv = DD((R[i][j] for i in range(n) for j in range(n)), (n, n))
        t.logdet = DD([logdet], ())
        t.z = DD(z)
        t.nll = DD([nll], ())
        t.alpha = DD(alpha)
        t.mean = DD(mean)
        t.var = DD(var)
        t.w_mp = wm
        t.s_pred = float(s_pred)
        return t


def factor_extended(t: Truth, perm):
    """L, L^-1 and z of the truth Gram with its points reordered by ``perm``, in numpy's
    extended precision (x87: 64-bit significand, eps 1.1e-19), by the same column Cholesky and
    forward substitution.  Its own error is eps_ext / eps = 1/2048 of an fp64 restatement's,
    whatever the conditioning: the yardstick of the permuted ensemble members, which a 50-digit
    factorisation per ordering (0.9 s each at n = 130) would make too slow for a test."""
    ld = np.longdouble
    if np.finfo(ld).eps > 2.0 ** -63:
        raise RuntimeError("numpy's longdouble has no 64-bit significand on this platform: the "
                           "yardstick of the permuted L, L^-1, z would be no better than fp64")
    perm = np.asarray(perm)
    A = (t.A.hi.astype(ld) + t.A.lo.astype(ld))[np.ix_(perm, perm)]
    w = (np.array([float(v) for v in t.w_mp], dtype=np.float64)[perm]).astype(ld)
    n = t.n
    L = np.zeros((n, n), dtype=ld)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Linv = np.zeros((n, n), dtype=ld)
    eye = np.eye(n, dtype=ld)
    for i in range(n):
        Linv[i] = (eye[i] - L[i, :i] @ Linv[:i]) / L[i, i]
    return L, Linv, Linv @ w


def _err_ext(x, ref) -> float:
    e = np.abs(np.asarray(x, dtype=np.float64).astype(np.longdouble) - ref)
    return float(np.max(e)) if e.size else 0.0


# ---------------------------------------------------------------------------- device's order
def device_acc(XA, XB, beta):
    """ardse_kernel's weighted distance, without the fma: sq = sqrt(beta), dt_k = sq_k xa_k -
    sq_k xb_k, acc = (((dt_0^2) + dt_1^2) + ...).  Returns (acc, dt) with dt (na, nb, d)."""
    XA = np.asarray(XA, dtype=np.float64)
    XB = np.asarray(XB, dtype=np.float64)
    sq = np.sqrt(np.asarray(beta, dtype=np.float64).reshape(-1))
    dt = (XA * sq)[:, None, :] - (XB * sq)[None, :, :]
    acc = np.zeros(dt.shape[:2])
    for k in range(dt.shape[2]):
        acc = acc + dt[:, :, k] * dt[:, :, k]
    return acc, dt


def device_values(XA, XB, beta, s):
    """s exp(-acc) in the device's order.  Results that may leave the normal range are rounded
    once from an extended-range product, as the kernels' ldexp of (s p) does."""
    acc, _ = device_acc(XA, XB, beta)
    v = s * np.exp(-acc)
    deep = acc > 600.0
    if np.any(deep):
        ext = np.longdouble(s) * np.exp(-acc[deep].astype(np.longdouble))
        v[deep] = ext.astype(np.float64)
    return v


def device_gram(X, beta, s, delta):
    G = device_values(X, X, beta, s)
    G[np.diag_indices_from(G)] = s + delta
    return G


def bound_rel(XA, XB, beta):
    """Bound on the relative error of a kernel value formed in the device's order, (na, nb):

        eps ( sum_k |dt_k| sq_k (|xa_k| + |xb_k|) + (2 + d/2) acc + 2 )

    With u = eps / 2: sq_k xa_k and sq_k xb_k are each rounded once (u sq_k |x| absolute each,
    entering acc through 2 |dt_k|: the first term); the root's and the subtraction's relative
    errors are common factors of dt_k (2 u each on dt_k^2: 4 u acc = 2 eps acc); the chain of d
    squares and sums adds at most d u acc = eps d/2 acc; exp turns acc's absolute error into a
    relative one; exp itself (1 ulp) and the scale by s are the final 2 eps.  Results in the
    subnormal range carry 2^-1074 absolute besides."""
    acc, dt = device_acc(XA, XB, beta)
    sq = np.sqrt(np.asarray(beta, dtype=np.float64).reshape(-1))
    XA = np.abs(np.asarray(XA, dtype=np.float64))
    XB = np.abs(np.asarray(XB, dtype=np.float64))
    first = np.sum(np.abs(dt) * sq * (XA[:, None, :] + XB[None, :, :]), axis=2)
    d = dt.shape[2]
    return EPS * (first + (2.0 + d / 2.0) * acc + 2.0)


# ----------------------------------------------------------------------------------- regimes
class Problem:
    """One regime at one size: X (n, d), Xs (m, d), w (n,), beta (d,), s, delta, s_pred."""


def _design(n: int, d: int, grid: bool):
    rng = np.random.default_rng(n)
    X = rng.random((n, d))
    if grid:
        X = np.linspace(1.0 / 8.0, 7.0 / 8.0, n).reshape(n, 1)
    beta_u = rng.random(d)
    u = rng.random(d)
    w = np.sin(X @ u)
    ntr = min(6, n)
    tr = rng.choice(n, size=ntr, replace=False)
    pairs = [(i, j) for i in range(n) for j in range(i)]
    npair = min(6, len(pairs))
    pick = rng.choice(len(pairs), size=npair, replace=False) if npair else []
    mids = np.array([0.5 * (X[pairs[p][0]] + X[pairs[p][1]]) for p in pick]).reshape(npair, d)
    Xs = np.concatenate([X[tr], mids, rng.random((12, d))], axis=0)
    return X, Xs, w, beta_u, ntr


@functools.lru_cache(maxsize=None)
def problem(regime: str, n: int) -> Problem:
    d = {"grid": 1, "d12": 12, "d32": 32}.get(regime, 8)
    X, Xs, w, bu, ntr = _design(n, d, regime == "grid")
    mid = 0.5 + 4.5 * bu
    beta, s, delta = {
        "mid": (mid, 1.0, 1e-4),
        "flat": (np.zeros(8), 1.0 / 0.3, 2e-5),
        "sharp": (np.full(8, 40.0), 1.0, 1e-5),
        "mixed": (np.array([0.0, 0.0, 30.0, 1e-3, 2.0, 0.0, 12.0, 0.1]), 0.2, 3e-5),
        "grid": (np.array([3.0]), 1.0, 1e-7),
        "d12": (mid * 8.0 / 12.0, 1.0, 1e-4),
        "d32": (bu, 1.0, 1e-6),
    }[regime]
    p = Problem()
    p.regime, p.n, p.d, p.m, p.ntrain = regime, n, d, Xs.shape[0], ntr
    p.X, p.Xs, p.w = X, Xs, w
    p.beta, p.s, p.delta = np.asarray(beta, dtype=np.float64), float(s), float(delta)
    p.s_pred = p.s + 0.01
    for a in (p.X, p.Xs, p.w, p.beta):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def truth_of(regime: str, n: int) -> Truth:
    p = problem(regime, n)
    return truth(p.X, p.Xs, p.w, p.beta, p.s, p.delta, p.s_pred)


def permutations(n: int):
    """The ensemble's orderings: the design as given, then NPERM seeded permutations."""
    out = [np.arange(n)]
    for k in range(NPERM):
        out.append(np.random.default_rng(1000 + k).permutation(n))
    return out


# --------------------------------------------------------------------------------- fp64 chain
def restate(G, Ks, w, s_pred):
    """oracle.gp_ref's formulas on a given Gram and cross-covariance (m, n): a dict of the
    chain's quantities in fp64 (LAPACK Cholesky and triangular solves)."""
    n = G.shape[0]
    L = np.linalg.cholesky(G)
    Linv = sla.solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    z = sla.solve_triangular(L, w, lower=True, check_finite=False)
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    alpha = sla.cho_solve((L, True), w)
    V = sla.solve_triangular(L, Ks.T, lower=True, check_finite=False) if Ks.shape[0] else \
        np.zeros((n, 0))
    return {"L": L, "Linv": Linv, "logdet": logdet, "z": z, "nll": 0.5 * z @ z + 0.5 * logdet,
            "alpha": alpha, "mean": Ks @ alpha, "var": s_pred - np.einsum("ij,ij->j", V, V)}


def members(p: Problem, perm):
    """The two restatements of the design reordered by ``perm``: the oracle's Gram and the
    device-order Gram."""
    X, w = p.X[perm], p.w[perm]
    yield restate(gp_ref.gram_ardse(X, p.beta, p.s, p.delta),
                  gp_ref.cross_ardse(p.Xs, X, p.beta, p.s), w, p.s_pred)
    yield restate(device_gram(X, p.beta, p.s, p.delta),
                  device_values(p.Xs, X, p.beta, p.s), w, p.s_pred)


def floor_of(quantity: str, t: Truth) -> float:
    if quantity == "var":
        return 4.0 * EPS * t.s_pred
    if quantity in ("logdet", "nll"):
        return 4.0 * EPS * t.n * max(1.0, abs(float(t.logdet.hi)) / t.n)
    return 4.0 * EPS * getattr(t, quantity).scale()


@functools.lru_cache(maxsize=None)
def _noise_invariant(regime: str, n: int):
    """Largest ensemble error of the order-independent quantities (no floor yet)."""
    p, t = problem(regime, n), truth_of(regime, n)
    worst = {q: 0.0 for q in QUANTITIES if q not in ORDER_DEPENDENT}
    for perm in permutations(n):
        inv = np.argsort(perm)
        for r in members(p, perm):
            for q in worst:
                x = r[q][inv] if q == "alpha" else r[q]
                worst[q] = max(worst[q], getattr(t, q).err(x))
    return worst


@functools.lru_cache(maxsize=None)
def _noise_ordered(regime: str, n: int):
    """Largest ensemble error of L, L^-1, z: the design as given against the 50-digit truth,
    every permuted ordering against its own extended-precision factors."""
    p, t = problem(regime, n), truth_of(regime, n)
    worst = {q: 0.0 for q in ORDER_DEPENDENT}
    for k, perm in enumerate(permutations(n)):
        ext = None if k == 0 else dict(zip(ORDER_DEPENDENT, factor_extended(t, perm)))
        for r in members(p, perm):
            for q in ORDER_DEPENDENT:
                e = getattr(t, q).err(r[q]) if ext is None else _err_ext(r[q], ext[q])
                worst[q] = max(worst[q], e)
    return worst


def noise(quantity: str, regime: str, n: int) -> float:
    """What fp64 delivers for ``quantity`` (max-abs error) in this regime at this size."""
    raw = (_noise_ordered if quantity in ORDER_DEPENDENT else _noise_invariant)(regime, n)
    return max(raw[quantity], floor_of(quantity, truth_of(regime, n)))


# --------------------------------------------------- the library's explicit-inverse arithmetic
# libgpfit's factorisation never back-substitutes: it inverts each diagonal block and multiplies
# (chol.hip: L_ik = A_ik D_k^T with D_k = L_kk^-1, X_kc = D_k R_kc; 64 x 64 blocks, and 16 x 16
# blocks inside a 64 x 64 one in the persistent kernel), and everything downstream is a product
# with the explicit L^-1 (z = L^-1 w, alpha = L^-T z, V = L^-1 K*).  A product with a computed
# inverse is not backward stable: L_ik = fl(A_ik D_k^T) solves (L_ik + dL) L_kk^T = A_ik only
# with |dL| <= c eps |A_ik| |D_k^T| |L_kk^T| |D_k^T|, a factor kappa(L_kk) above the
# substitution's c eps |L_ik| |L_kk^T| |D_k^T|.  Where the diagonal blocks are themselves
# ill-conditioned (the 1-D grid: kappa(L_kk) ~ 1e4) that factor shows in every quantity; where
# they are not it stays inside the margin.  explicit_inverse_term gives the closed form and the
# sharper evaluated one: the same arithmetic carried out in fp64 numpy on the ensemble's
# orderings, in the two blockings the library has.
BLOCKINGS = ((64,), (64, 16))


def explicit_factor(A, sizes):
    """Right-looking blocked Cholesky with L^-1 alongside, every panel a product with the
    explicit inverse of its diagonal block; ``sizes`` the nested block sizes (the innermost
    block is factored by LAPACK and inverted by substitution)."""
    n = A.shape[0]
    while sizes and n <= sizes[0]:
        sizes = sizes[1:]
    if not sizes:
        L = np.linalg.cholesky(A)
        return L, sla.solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    nb = sizes[0]
    A = A.copy()
    L, X, R = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        Lkk, Dk = explicit_factor(A[k0:k1, k0:k1], sizes[1:])
        L[k0:k1, k0:k1], X[k0:k1, k0:k1] = Lkk, Dk
        X[k0:k1, :k0] = Dk @ R[k0:k1, :k0]
        if k1 < n:
            L[k1:, k0:k1] = A[k1:, k0:k1] @ Dk.T
            A[k1:, k1:] -= L[k1:, k0:k1] @ L[k1:, k0:k1].T
            R[k1:, :k1] -= L[k1:, k0:k1] @ X[k0:k1, :k1]
    return L, X


def restate_explicit(G, Ks, w, s_pred, sizes):
    """The chain as the library forms it: blocked explicit-inverse factors, then products."""
    L, X = explicit_factor(G, sizes)
    z = X @ w
    V = X @ Ks.T
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    return {"L": L, "Linv": X, "logdet": logdet, "z": z, "nll": 0.5 * z @ z + 0.5 * logdet,
            "alpha": X.T @ z, "mean": V.T @ z, "var": s_pred - np.einsum("ij,ij->j", V, V)}


@functools.lru_cache(maxsize=None)
def _explicit_errors(regime: str, n: int):
    p, t = problem(regime, n), truth_of(regime, n)
    worst = {q: 0.0 for q in QUANTITIES}
    for k, perm in enumerate(permutations(n)):
        ext = None if k == 0 else dict(zip(ORDER_DEPENDENT, factor_extended(t, perm)))
        inv = np.argsort(perm)
        X = p.X[perm]
        G = device_gram(X, p.beta, p.s, p.delta)
        Ks = device_values(p.Xs, X, p.beta, p.s)
        for sizes in BLOCKINGS:
            r = restate_explicit(G, Ks, p.w[perm], p.s_pred, sizes)
            for q in QUANTITIES:
                if q in ORDER_DEPENDENT and ext is not None:
                    e = _err_ext(r[q], ext[q])
                else:
                    e = getattr(t, q).err(r[q][inv] if q == "alpha" else r[q])
                worst[q] = max(worst[q], e)
    return worst


# The (quantity, regime, n) entries at which the device was measured above MARGIN x noise (MI355X,
# DESIGN.md section 7): the 1-D grid from one full 64-block on.  Only these carry the extra term;
# everything else is held to MARGIN x noise alone.
FINDINGS = frozenset(
    [(q, "grid", 64) for q in ("L", "alpha", "mean", "var")] +
    [(q, "grid", 65) for q in ("L", "Linv", "z", "alpha", "mean", "var")] +
    [(q, "grid", 130) for q in QUANTITIES])


@functools.lru_cache(maxsize=None)
def block_condition(regime: str, n: int) -> float:
    """The largest 2-norm condition number of a diagonal block L_kk of the true factor, over the
    64 x 64 and the 16 x 16 blocks: the factor by which a product with fl(L_kk^-1) may exceed
    a substitution's error (see the derivation above)."""
    L = truth_of(regime, n).L.hi
    worst = 1.0
    for nb in (64, 16):
        for k0 in range(0, n, nb):
            worst = max(worst, float(np.linalg.cond(L[k0:k0 + nb, k0:k0 + nb])))
    return worst


def explicit_inverse_term(quantity: str, regime: str, n: int) -> float:
    """What the explicit-inverse arithmetic adds to the noise level at a documented finding, 0
    anywhere else.  Closed form: a substitution's error is the noise, a product with the
    computed inverse of L_kk carries up to cond(L_kk) times that, so the term is at most
    (block_condition - 1) x noise.  That is a worst case over error directions, 50 ... 500 times
    what the arithmetic does on these matrices, so the term used is the sharper of the two: the
    largest error of the numpy restatement over the ensemble's orderings and both blockings,
    less the noise, capped by the closed form (tests/test_mp_ref_cpu.py asserts the order)."""
    if (quantity, regime, n) not in FINDINGS:
        return 0.0
    nz = noise(quantity, regime, n)
    emulated = max(0.0, _explicit_errors(regime, n)[quantity] - nz)
    return min(emulated, (block_condition(regime, n) - 1.0) * nz)


def limit(quantity: str, regime: str, n: int) -> float:
    """The tests' bound on a device quantity's error against the truth: MARGIN x noise, plus
    MARGIN x the explicit-inverse term at the documented findings."""
    return MARGIN * (noise(quantity, regime, n) + explicit_inverse_term(quantity, regime, n))
