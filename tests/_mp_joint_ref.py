"""The joint predictive covariance, its Cholesky factor and the joint draws at 50 digits, with the
fp64 noise level of each (built on tests/_mp_ref.py, which stays as it is).

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.

* ``truth_cov``: C = K** + (s_pred + jitter - s) I - V^T V, V = L^-1 K*, at ``mp.dps = 50`` from
  the exact binary values of the fp64 inputs (Gram, column Cholesky, V by forward substitution,
  then prior - V^T V), kept as a ``DD``.
* ``points``: the test-point sets.  ``"std"`` is ``problem(...).Xs`` (m = 24: 6 training points,
  6 midpoints, 12 random points); ``"wide65"`` / ``"wide130"`` hold, in seeded and then shuffled
  equal quarters, training points taken exactly, training points moved by 2^-20 N(0, 1) per
  coordinate, fresh random points and exact repeats of those: every way C_ij can be the small
  difference of two numbers of size s; ``"one"`` is m = 1 (a training point).  m = 65 is the
  first size on gp_predict_cov's 128-tiles, m = 130 has two tiles per side (the mirrored
  off-diagonal tile and a partly filled last tile), m = 24 and m = 1 are on its 64-tiles.
* ``noise_cov``: the largest error of prior - V^T V against the truth over the ensemble of
  ``_mp_ref.members`` (the design as given and 8 permutations of the training points, C does not
  depend on their order; each with the oracle's Gram and with the device-order Gram; LAPACK
  Cholesky and triangular solve; the prior from ``device_values``), never below 4 eps s_pred,
  the project's floor for ``var``.  A test asks ``error <= limit_cov = MARGIN (noise + explicit
  term)``, the explicit-inverse term being non-zero only at ``FINDINGS_COV``.
* ``truth_factor`` / ``noise_factor``: the 50-digit Cholesky factor and log-determinant of an
  exact fp64 matrix, and LAPACK's error on the same matrix (floors 4 eps max|R| and the chain's
  log-determinant floor).
* ``normals_mp`` / ``truth_draws``: gp_realize's normal stream and mean + tril(R) xi at 50 digits.
* ``bound_rel_epilogue``: the bound on a prior value formed in jc_syrk_kernel's order.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla
from mpmath import mp, mpf

from oracle import gp_ref, rng_ref

import _mp_ref as M
from _mp_ref import (BLOCKINGS, DD, EPS, MARGIN, SIZES, _chol_mp, device_gram, device_values,
                     explicit_factor, kernel_exp, permutations, problem)

DPS = M.DPS
WIDE = {"wide65": 65, "wide130": 130}
WIDE_N = (5, 65, 130)
ONE_N = (1, 130)
# every (regime-independent) case the device is held to: (n, pts)
CASES = ([(n, "std") for n in SIZES] + [(n, w) for n in WIDE_N for w in WIDE] +
         [(n, "one") for n in ONE_N])

# The (regime, n) entries (every point set) at which the bound carries the explicit-inverse term:
# the 1-D grid from one full 64-block on, the place _mp_ref.FINDINGS documents for var (V = L^-1 K*
# is a product with an explicit inverse whose diagonal blocks have cond ~ 1e4 there; C inherits
# V's error through V^T V).  Everything else is held to MARGIN x noise alone.
FINDINGS_COV = frozenset(("grid", n) for n in (64, 65, 130))


# ------------------------------------------------------------------------------- test points
@functools.lru_cache(maxsize=None)
def points(regime: str, n: int, pts: str) -> np.ndarray:
    """The (m, d) test points of a set.  The seeds do not depend on the regime, so the four d = 8
    regimes share them as they share X."""
    p = problem(regime, n)
    if pts == "std":
        return p.Xs
    if pts == "one":
        out = p.Xs[:1].copy()
    else:
        m = WIDE[pts]
        rng = np.random.default_rng([n, m, 11])
        q = m // 4
        fresh = m - 3 * q
        exact = p.X[rng.choice(n, size=q, replace=n < q)]
        moved = p.X[rng.choice(n, size=q, replace=n < q)] + \
            2.0 ** -20 * rng.standard_normal((q, p.d))
        rnd = rng.random((fresh, p.d))
        if regime == "grid":
            rnd = 0.125 + 0.75 * rnd
        out = np.concatenate([exact, moved, rnd, rnd[:q]], axis=0)[rng.permutation(m)]
    out.setflags(write=False)
    return out


def params(regime: str, n: int, jitter: float = 0.0, nugget: bool = True):
    """(s_pred in force, fl(s_pred + jitter): the diagonal of the prior as the device forms it)."""
    p = problem(regime, n)
    sp = p.s_pred if nugget else p.s
    return sp, sp + float(jitter)


# ------------------------------------------------------------------------------------- truth
_CHOL, _CORE, _TRUTH = {}, {}, {}


def _mp_rows(a):
    return [[mpf(v) for v in row] for row in np.asarray(a, dtype=np.float64).tolist()]


def gram_chol_mp(X, beta, s, delta):
    """(rows of X, beta, s as mpf, the 50-digit column Cholesky factor of the Gram as rows of
    mpf) from fp64 arrays taken as exact; call under ``mp.workdps(DPS)``."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    Xm = _mp_rows(X) if n else []
    bt = [mpf(float(v)) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
    sm, dm = mpf(float(s)), mpf(float(delta))
    A = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            A[i][j] = sm * kernel_exp(Xm[i], Xm[j], bt)
        A[i][i] = sm + dm
    return Xm, bt, sm, _chol_mp(A)


def cov_core_mp(chol, Xs):
    """(Q, vv): Q[i][j] = s k(xs_i, xs_j) - v_i . v_j off the diagonal (the diagonal left 0) and
    vv[i] = v_i . v_i, v_i = L^-1 k*(xs_i) by forward substitution: everything of C that does not
    depend on s_pred or the jitter, as mpf.  ``chol`` from ``gram_chol_mp``; n = 0 leaves the
    prior.  Call under ``mp.workdps(DPS)``."""
    Xm, bt, sm, L = chol
    n = len(Xm)
    Xsm = _mp_rows(Xs)
    m = len(Xsm)
    V = []
    for q in range(m):
        k = [sm * kernel_exp(Xsm[q], Xm[i], bt) for i in range(n)]
        v = [mpf(0)] * n
        for i in range(n):
            v[i] = (k[i] - mp.fdot(L[i][:i], v[:i])) / L[i][i]
        V.append(v)
    Q = [[mpf(0)] * m for _ in range(m)]
    for i in range(m):
        for j in range(i):
            Q[i][j] = Q[j][i] = sm * kernel_exp(Xsm[i], Xsm[j], bt) - mp.fdot(V[i], V[j])
    return Q, [mp.fdot(V[i], V[i]) for i in range(m)]


def diag_mp(vv, top, jitter):
    """The diagonal (top + jitter) - v_i . v_i, the sum of the two fp64 values taken exactly."""
    t = mpf(float(top)) + mpf(float(jitter))
    return [t - v for v in vv]


def truth_cov_mp(X, Xs, beta, s, delta, s_pred, jitter=0.0):
    """C as rows of mpf from fp64 arrays: the steps ``truth_cov`` takes (``gram_chol_mp``,
    ``cov_core_mp``, ``diag_mp``) without its caches.  X with no rows gives the prior."""
    with mp.workdps(DPS):
        Q, vv = cov_core_mp(gram_chol_mp(X, beta, s, delta), Xs)
        for i, v in enumerate(diag_mp(vv, s_pred, jitter)):
            Q[i][i] = v
        return Q


def _chol_of(regime: str, n: int):
    """The 50-digit Gram factor of the regime's training design, as rows of mpf."""
    key = (regime, n)
    if key not in _CHOL:
        p = problem(regime, n)
        with mp.workdps(DPS):
            _CHOL[key] = gram_chol_mp(p.X, p.beta, p.s, p.delta)
    return _CHOL[key]


def _core(regime: str, n: int, pts: str):
    """(DD of ``cov_core_mp``'s Q, its vv as mpf) of a case, computed once."""
    key = (regime, n, pts)
    if key not in _CORE:
        with mp.workdps(DPS):
            Q, vv = cov_core_mp(_chol_of(regime, n), points(regime, n, pts))
            m = len(vv)
            _CORE[key] = (DD((Q[i][j] for i in range(m) for j in range(m)), (m, m)), vv)
    return _CORE[key]


def truth_cov(regime: str, n: int, pts: str, jitter: float = 0.0, nugget: bool = True) -> DD:
    """C (m, m) at 50 digits; s_pred + jitter (s + jitter without the nugget) minus v_i . v_i on
    the diagonal, the sum taken exactly.  n = 0 (with "std": the regime's 12 random test points)
    gives the prior, s_pred + jitter itself on the diagonal."""
    key = (regime, n, pts, float(jitter), bool(nugget))
    if key not in _TRUTH:
        off, vv = _core(regime, n, pts)
        sp, _ = params(regime, n, 0.0, nugget)
        with mp.workdps(DPS):
            diag = DD(diag_mp(vv, sp, jitter))
        out = DD.__new__(DD)
        out.hi, out.lo = off.hi.copy(), off.lo.copy()
        idx = np.diag_indices(out.hi.shape[0])
        out.hi[idx], out.lo[idx] = diag.hi, diag.lo
        _TRUTH[key] = out
    return _TRUTH[key]


# ------------------------------------------------------------------------------------- noise
def _prior_fp64(regime, n, pts, jitter, nugget):
    p, Xs = problem(regime, n), points(regime, n, pts)
    K = device_values(Xs, Xs, p.beta, p.s)
    K[np.diag_indices_from(K)] = params(regime, n, jitter, nugget)[1]
    return K


def _orderings(regime, n, pts):
    """(G, K* (m, n)) of every ensemble member's training order and Gram."""
    p, Xs = problem(regime, n), points(regime, n, pts)
    for perm in permutations(n):
        X = p.X[perm]
        yield "oracle", gp_ref.gram_ardse(X, p.beta, p.s, p.delta), \
            gp_ref.cross_ardse(Xs, X, p.beta, p.s)
        yield "device", device_gram(X, p.beta, p.s, p.delta), device_values(Xs, X, p.beta, p.s)


@functools.lru_cache(maxsize=None)
def _noise_raw(regime, n, pts, jitter, nugget):
    t = truth_cov(regime, n, pts, jitter, nugget)
    prior = _prior_fp64(regime, n, pts, jitter, nugget)
    worst = 0.0
    for _, G, Ks in _orderings(regime, n, pts):
        L = np.linalg.cholesky(G)
        V = sla.solve_triangular(L, Ks.T, lower=True, check_finite=False)
        worst = max(worst, t.err(prior - V.T @ V))
    return worst


def noise_cov(regime: str, n: int, pts: str, jitter: float = 0.0, nugget: bool = True) -> float:
    """What fp64 delivers for C (max-abs error) in this regime, size and point set."""
    sp, _ = params(regime, n, 0.0, nugget)
    return max(_noise_raw(regime, n, pts, float(jitter), bool(nugget)), 4.0 * EPS * sp)


@functools.lru_cache(maxsize=None)
def explicit_error_cov(regime, n, pts, jitter=0.0, nugget=True) -> float:
    """The largest error of C formed as the library does (V = X K*^T with the blocked
    explicit-inverse X of ``explicit_factor``, both blockings, the device-order Gram) over the
    ensemble's orderings."""
    t = truth_cov(regime, n, pts, jitter, nugget)
    prior = _prior_fp64(regime, n, pts, jitter, nugget)
    worst = 0.0
    for kind, G, Ks in _orderings(regime, n, pts):
        if kind != "device":
            continue
        for sizes in BLOCKINGS:
            _, X = explicit_factor(G, sizes)
            V = X @ Ks.T
            worst = max(worst, t.err(prior - V.T @ V))
    return worst


def explicit_cap_cov(regime, n, pts, jitter=0.0, nugget=True) -> float:
    """The closed form of ``_mp_ref.explicit_inverse_term``: (block_condition - 1) x noise."""
    return (M.block_condition(regime, n) - 1.0) * noise_cov(regime, n, pts, jitter, nugget)


def explicit_term_cov(regime, n, pts, jitter=0.0, nugget=True) -> float:
    """What the explicit-inverse arithmetic adds to the noise at a documented finding, 0 anywhere
    else: the evaluated error less the noise, capped by the closed form."""
    if (regime, n) not in FINDINGS_COV:
        return 0.0
    nz = noise_cov(regime, n, pts, jitter, nugget)
    emulated = max(0.0, explicit_error_cov(regime, n, pts, float(jitter), bool(nugget)) - nz)
    return min(emulated, explicit_cap_cov(regime, n, pts, jitter, nugget))


def limit_cov(regime, n, pts, jitter=0.0, nugget=True) -> float:
    return MARGIN * (noise_cov(regime, n, pts, jitter, nugget) +
                     explicit_term_cov(regime, n, pts, jitter, nugget))


# -------------------------------------------------------------- the epilogue's prior values
def bound_rel_epilogue(XA, XB, beta):
    """Bound on the relative error of a prior value formed in jc_syrk_kernel's order, (na, nb):

        eps ( (3/2 + d/2) acc + 2 )

    The epilogue subtracts the unscaled coordinates, t_k = xa_k - xb_k, and accumulates
    dist = fma(beta_k t_k, t_k, dist).  With u = eps / 2: t_k carries one rounding relative to
    itself (2 u on t_k^2; ardse_kernel's order rounds sq_k xa_k and sq_k xb_k before it subtracts,
    which is _mp_ref.bound_rel's first term and has no counterpart here), beta_k t_k one more
    (u), so each term is within 3 u of beta_k t_k^2: 3 u acc = 3/2 eps acc; the d roundings of
    the fma chain add at most d u acc = eps d/2 acc; exp turns acc's absolute error into a
    relative one; exp_neg (1 ulp) and the scale by s are the final 2 eps.  Results in the
    subnormal range carry 2^-1074 absolute besides."""
    XA = np.asarray(XA, dtype=np.float64)
    XB = np.asarray(XB, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    t = XA[:, None, :] - XB[None, :, :]
    acc = np.sum(beta * t * t, axis=2)
    return EPS * ((1.5 + beta.size / 2.0) * acc + 2.0)


# ------------------------------------------------------------------------------- the factor
_FACTOR = {}


def truth_factor(C):
    """(R, logdet): the 50-digit lower Cholesky factor (zeros above the diagonal) of the exact
    fp64 matrix C (its lower triangle), and log det C = 2 sum log R_ii, both as ``DD``."""
    C = np.ascontiguousarray(np.asarray(C, dtype=np.float64))
    key = (C.shape, C.tobytes())
    if key not in _FACTOR:
        m = C.shape[0]
        with mp.workdps(DPS):
            R, logdet = factor_mp(C)
            _FACTOR[key] = (DD((R[i][j] for i in range(m) for j in range(m)), (m, m)),
                            DD([logdet], ()))
    return _FACTOR[key]


def factor_mp(C):
    """``truth_factor``'s values before they are split into pairs: (rows of mpf, logdet); call
    under ``mp.workdps(DPS)``."""
    R = _chol_mp(_mp_rows(C))
    return R, 2 * mp.fsum(mp.log(R[i][i]) for i in range(len(R)))


def noise_factor(C):
    """(noise of R, noise of logdet): the error of np.linalg.cholesky on the same matrix against
    ``truth_factor``, never below 4 eps max|R| and the chain's log-determinant floor
    4 eps m max(1, |logdet| / m).  The log-determinant does not depend on the order of the
    rows and columns, so its noise is the largest error over C as given and the ensemble's 8
    symmetric permutations of it (a single run on a matrix of cond 1e10 is a sample of one);
    R does depend on the order and keeps the run on C as given."""
    C = np.asarray(C, dtype=np.float64)
    m = C.shape[0]
    R, logdet = truth_factor(C)
    L = np.linalg.cholesky(C)
    worst_ld = 0.0
    for perm in permutations(m):
        Lp = np.linalg.cholesky(C[np.ix_(perm, perm)])
        worst_ld = max(worst_ld, logdet.err(2.0 * np.sum(np.log(np.diag(Lp)))))
    floor_ld = 4.0 * EPS * m * max(1.0, abs(float(logdet.hi)) / m)
    return max(R.err(L), 4.0 * EPS * R.scale()), max(worst_ld, floor_ld)


# -------------------------------------------------------------------------------- the draws
@functools.lru_cache(maxsize=None)
def _normals_mp(start: int, stop: int, seed: int, offset: int):
    j = np.arange(start >> 1, (stop + 1) >> 1, dtype=np.uint64)
    ctr = np.stack([(j & rng_ref.MASK32).astype(np.uint32),
                    (j >> np.uint64(32)).astype(np.uint32),
                    np.full(j.size, offset & 0xFFFFFFFF, dtype=np.uint32),
                    np.full(j.size, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint32)], axis=1)
    words = rng_ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).tolist()
    pair = {}
    with mp.workdps(DPS):
        scale = mpf(2) ** -53
        for jj, w in zip(j.tolist(), words):
            u1 = mpf(((w[0] << 32) | w[1]) >> 11) * scale
            u2 = mpf(((w[2] << 32) | w[3]) >> 11) * scale
            r = mp.sqrt(-2 * mp.log(1 - u1))
            pair[jj] = (r * mp.cospi(2 * u2), r * mp.sinpi(2 * u2))
        return tuple(pair[e >> 1][e & 1] for e in range(start, stop))


def normals_mp(N: int, seed: int, offset: int = 0, start: int = 0):
    """Elements start .. N - 1 of gp_realize's stream at 50 digits, from the Philox words of
    oracle.rng_ref: element e uses counter (e >> 1, offset), u1 and u2 the top 53 bits of words
    (0, 1) and (2, 3) times 2^-53, sqrt(-2 log(1 - u1)) times cospi(2 u2) for even e and
    sinpi(2 u2) for odd e."""
    return list(_normals_mp(int(start), int(N), int(seed), int(offset)))


def normals_rel_error(N: int, seed: int, offset: int = 0, start: int = 0) -> float:
    """The worst relative error of oracle.rng_ref.normals against ``normals_mp`` over elements
    start .. N - 1 (what an fp64 restatement of the stream delivers)."""
    z = rng_ref.normals(N, seed, offset)[start:]
    worst = 0.0
    with mp.workdps(DPS):
        for got, t in zip(z.tolist(), normals_mp(N, seed, offset, start)):
            if t != 0:
                worst = max(worst, float(abs(mpf(got) - t) / abs(t)))
    return worst


def normals_abs_error(N: int, seed: int, offset: int = 0, start: int = 0) -> np.ndarray:
    """|oracle.rng_ref.normals - normals_mp| per element start .. N - 1: each normal's own fp64
    noise (large relative to the normal only where cos / sin(2 pi u2) sits next to a zero)."""
    z = rng_ref.normals(N, seed, offset)[start:]
    with mp.workdps(DPS):
        return np.array([float(abs(mpf(got) - t))
                         for got, t in zip(z.tolist(), normals_mp(N, seed, offset, start))])


def truth_draws(R, mean, seed: int, offset: int, nsamp: int, unit0: int = 0):
    """(DD (batch, nsamp, m) of mean_b + tril(R_b) xi, fp64 (batch, nsamp, m) of
    sum_k |R_ik xi_k|, fp64 (batch, nsamp, m) of sum_k |R_ik| max(e_k, 4 eps |xi_k|) with e_k the
    fp64 stream's own error of that normal) from fp64 R (logical [b, i, k]) and mean and the
    50-digit normals, element ((unit0 + b) nsamp + r) m + k of the stream.  The last is never
    above max(worst relative error, 4 eps) times the second."""
    R = np.asarray(R, dtype=np.float64)
    batch, m, _ = R.shape
    lo, hi = unit0 * nsamp * m, (unit0 + batch) * nsamp * m
    xi = normals_mp(hi, seed, offset, lo)
    xerr = normals_abs_error(hi, seed, offset, lo)
    vals, mag, magerr = [], np.zeros((batch, nsamp, m)), np.zeros((batch, nsamp, m))
    with mp.workdps(DPS):
        for b in range(batch):
            rows = _mp_rows(R[b])
            mu = [mpf(0)] * m if mean is None else [mpf(float(v)) for v in mean[b]]
            absr = np.abs(np.tril(R[b]))
            for r in range(nsamp):
                x = xi[(b * nsamp + r) * m:(b * nsamp + r + 1) * m]
                for i in range(m):
                    vals.append(mu[i] + mp.fdot(rows[i][:i + 1], x[:i + 1]))
                # the magnitude only scales a bound: fp64 of the 50-digit normals is enough
                ax = np.abs(np.array([float(v) for v in x]))
                mag[b, r] = absr @ ax
                e = xerr[(b * nsamp + r) * m:(b * nsamp + r + 1) * m]
                magerr[b, r] = absr @ np.maximum(e, 4.0 * EPS * ax)
        return DD(vals, (batch, nsamp, m)), mag, magerr


# ------------------------------------------------- positive definiteness: the derived jitter
def potrf_backward(m: int, cmax: float) -> float:
    """F: the 2-norm of the backward error of an m x m Cholesky in fp64.  Higham, Accuracy and
    Stability of Numerical Algorithms (2nd ed.), Theorem 10.3: R R^T = C + dC with |dC| <=
    gamma_{m+1} |R| |R^T|, gamma_k = k u / (1 - k u), u = eps / 2, in any order of summation; and
    (eq. 10.7 and the proof of Theorem 10.7) || |R| |R^T| ||_2 <= m ||C||_2 / (1 - m gamma_{m+1})
    with ||C||_2 <= m max C_ii.  Written as F = c m eps max C_ii: c = m (m + 1) / 2 up to the
    (1 - ...) denominators, kept here."""
    u = EPS / 2.0
    g = (m + 1) * u / (1.0 - (m + 1) * u)
    return m * g / (1.0 - m * g) * m * cmax


def sufficient_jitter(regime: str, n: int, pts: str) -> float:
    """J = 2 (m E + F) without the nugget: the device's C differs from the truth C_t + J I by dC
    with ||dC||_2 <= m E (E = limit_cov, a max-abs bound), so lambda_min(C) >= lambda_min(C_t) +
    J - m E >= m E + 2 F (C_t is positive semi-definite) and a Cholesky with backward error F
    cannot meet a non-positive pivot.  E depends on J through the rounding of s + J, so it is
    evaluated at J and the larger of the two taken."""
    p = problem(regime, n)
    m = points(regime, n, pts).shape[0]
    E = limit_cov(regime, n, pts, 0.0, False)
    J = 0.0
    for _ in range(2):
        F = potrf_backward(m, p.s + J)
        J = 2.0 * (m * E + F)
        E = max(E, limit_cov(regime, n, pts, J, False))
    return 2.0 * (m * E + potrf_backward(m, p.s + J))


def lambda_min(regime: str, n: int, pts: str) -> float:
    """The smallest eigenvalue of the truth C without the nugget (fp64 eigvalsh of the rounded
    truth: its own error, ~ m eps s, is inside F)."""
    return float(np.linalg.eigvalsh(truth_cov(regime, n, pts, 0.0, False).hi)[0])
