"""gp_xval at 50 digits (mpmath) on the regimes of tests/_mp_ref.py, its fp64 noise level per
(quantity, regime, n, plan), the fold plans, and the condition under which a power-of-two
scaling of its inputs is exact.

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.

Quantities: ``xmean`` = E[w_F | w outside F]; ``xvar`` = diag Cov(w_F | rest) - shift with
shift = s + delta - s_pred (what gp_predict reports at a new point placed there); ``xq`` = the
same with no shift: 1/q for a singleton fold, diag(Q_FF^-1) for a larger one.  On the 1-D grid
xq ~ 1e-7 under a shift of 1e-2, so an error of xq is invisible in xvar: it is held on its own
scale.

Truth, two layers.

* ``chain_truth``: from L^-1 and z as mpf (``factor_mp``: ``_mp_ref``'s own column Cholesky and
  substitution on the same problems, carried at 65 digits because inverting Q_FF costs cond(A)
  of them; ``_mp_ref.truth_of`` keeps only double-double pairs): per fold Q_FF = P_F^T P_F,
  alpha_F = P_F^T z, an mp Cholesky of the f x f system, mean_F = w_F - Q_FF^-1 alpha_F and
  diag(Q_FF^-1).  What Gram -> factorisation -> gp_xval together owe.
* ``kernel_truth``: the same formulas at 50 digits on a *given* fp64 L^-1, w and shift taken as
  exact binary inputs: what gp_xval alone owes once the factorisation's error is set aside.

Noise (the project's rule: what fp64 itself delivers, never the device's output).

* ``chain_noise``: the largest error against the chain truth of tests/_xval_ref.closed_form on
  the oracle's Gram and on the device-order Gram, over ``_mp_ref.permutations(n)`` (fold indices
  mapped through the permutation, results un-permuted).
* ``kernel_noise``: the largest error against the kernel truth over fp64 restatements from the
  same fp64 L^-1: Q_FF = P^T P inverted by ``inv``, by ``cho_solve`` and by ``solve``, with each
  fold as given, sorted and reversed.
* floors: 4 eps max|truth| for xmean and xq (4 eps max|w| where the mean's truth is 0: the
  whole-design folds), 4 eps s_pred for xvar.

A test asks error <= MARGIN x noise.  ``FINDINGS`` lists the chain-layer entries on the 1-D grid
at which the device was measured above that; only they carry ``explicit_inverse_term`` (the
closed form on ``_mp_ref.explicit_factor``'s L^-1, see there).  The kernel layer has no findings.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla
from mpmath import mp, mpf

from oracle import gp_ref

import _mp_ref as M
import _xval_ref

DD, EPS, MARGIN, DPS = M.DD, M.EPS, M.MARGIN, M.DPS
REGIMES, SIZES, GROUPS = M.REGIMES, M.SIZES, M.GROUPS
problem, truth_of = M.problem, M.truth_of
QUANTITIES = ("xmean", "xvar", "xq")
GUARD_DIGITS = 15                 # the chain truth is carried at DPS + 15 to be good to DPS


# --------------------------------------------------------------------------------- fold plans
def _alternate(parts):
    """Every other fold sorted, the others in the permutation's order."""
    return [[int(i) for i in (np.sort(F) if k % 2 else F)] for k, F in enumerate(parts)]


def _cut(perm, sizes):
    out, at = [], 0
    for f in sizes:
        out.append(perm[at:at + f])
        at += f
    return out, perm[at:]


@functools.lru_cache(maxsize=None)
def plans(n: int):
    """{name: folds} of one size, deterministic; None is leave-one-out (``folds=None``)."""
    if n == 1:
        return {"loo": None, "one": [[0]]}
    if n == 5:
        return {"loo": None, "pair_triple": [[0, 1], [2, 3, 4]], "whole": [[4, 0, 2, 1, 3]]}
    rng = np.random.default_rng([n, 77])
    if n == 64:
        # T = 1 below, at and above one 16-tile, a pair, and the rest as singletons
        parts, rest = _cut(rng.permutation(64), (15, 16, 17, 2))
        return {"loo": None, "whole": [list(range(64))],
                "tiles": _alternate(parts) + [[int(i)] for i in rest]}
    if n == 65:
        # the fold of 33 or of 32 that holds index 64 stages the row pair (64, 65)
        parts, _ = _cut(rng.permutation(65), (33, 32))
        return {"loo": None, "tail64": [list(range(1, 65))], "head64": [list(range(64))],
                "split": _alternate(parts)}
    if n == 130:
        big, _ = _cut(rng.permutation(130), (64, 63, 2, 1))
        mid, _ = _cut(rng.permutation(130), (49, 48, 33))
        thirds = [[i for i in range(130) if i % 3 == k] for k in range(3)]
        # folds wholly in rows >= 64: minima at 64, at 80 (79 in late_pair) and at 112, so the
        # r0 = min(F) & ~15 skip starts at 64, 80 / 64 and 112, and the 64-row chunks from there
        # end in the odd-column pair (127, 129) or in the last pair (128, 129): two plans, since
        # the library takes an index in one fold only and both pairs hold 129
        pool = rng.permutation(np.arange(81, 112))
        late = [np.concatenate([[64], pool[:16]]), np.concatenate([pool[16:], [80]]),
                rng.permutation(np.arange(112, 127)), np.array([127, 129])]
        pool = rng.permutation(np.concatenate([np.arange(65, 79), np.arange(80, 112)]))
        high = pool[pool > 79]
        f16 = np.concatenate([high[:15], [79]])
        f17 = np.concatenate([[64], np.setdiff1d(pool, f16, assume_unique=True)[:16]])
        late_pair = [f17, f16, rng.permutation(np.arange(112, 128))[:15], np.array([128, 129])]
        return {"loo": None, "big": _alternate(big), "mid": _alternate(mid), "thirds": thirds,
                "late": _alternate(late) + [[128]], "late_pair": _alternate(late_pair)}
    raise ValueError(f"no fold plans for n = {n}")


CASES = [(g, n, name) for g in GROUPS for n in SIZES for name in plans(n)]
REGIME_CASES = [(r, n, name) for r in REGIMES for n in SIZES for name in plans(n)]


def folds_of(n: int, plan: str):
    return plans(n)[plan]


def listed(folds, n: int):
    """The folds as a list of index lists (leave-one-out spelt out)."""
    return [[i] for i in range(n)] if folds is None else [list(F) for F in folds]


def covered(folds, n: int):
    """Sorted indices that some fold covers."""
    return np.array(sorted(i for F in listed(folds, n) for i in F), dtype=int)


def shift_of(p) -> float:
    """The shift the device is handed: fl(fl(s + delta) - s_pred)."""
    return float(np.float64(p.s) + np.float64(p.delta) - np.float64(p.s_pred))


# -------------------------------------------------------------------------------------- truth
def _fold_mp(cols, z, w, F):
    """(mean_F, diag Q_FF^-1) as lists of mpf, from the columns of L^-1 (cols[j][i] = (L^-1)[i][j],
    zero above the diagonal), z and w.  Call under ``mp.workdps``."""
    f = len(F)
    Q = [[mpf(0)] * f for _ in range(f)]
    for a in range(f):
        for b in range(a + 1):
            r = max(F[a], F[b])
            Q[a][b] = mp.fdot(cols[F[a]][r:], cols[F[b]][r:])
    alpha = [mp.fdot(cols[j][j:], z[j:]) for j in F]
    R = M._chol_mp(Q)
    C = M._linv_mp(R)                                   # C[a][k] = (R^-1)[k][a]
    y = [mp.fdot([C[a][k] for a in range(k + 1)], alpha[:k + 1]) for k in range(f)]
    x = [mp.fdot(C[a][a:], y[a:]) for a in range(f)]
    diag = [mp.fdot(C[a][a:], C[a][a:]) for a in range(f)]
    return [w[F[a]] - x[a] for a in range(f)], diag


class XTruth:
    """xmean, xvar, xq as DD over ``idx`` (the covered indices, sorted); ``mp`` the same as
    lists of mpf."""

    def err(self, quantity: str, x) -> float:
        return getattr(self, quantity).err(np.asarray(x, dtype=np.float64)[self.idx])

    def full(self, quantity: str):
        """The truth rounded to fp64 as an (n,) array, NaN where no fold covers."""
        out = np.full(self.n, np.nan)
        out[self.idx] = getattr(self, quantity).hi
        return out


def _truth_from(cols, z, w, folds, shift, n, guard=0):
    with mp.workdps(DPS + guard):
        mean, diag = {}, {}
        for F in listed(folds, n):
            m, d = _fold_mp(cols, z, w, F)
            for i, mi, di in zip(F, m, d):
                mean[i], diag[i] = mi, di
        t = XTruth()
        t.n = n
        t.idx = np.array(sorted(mean), dtype=int)
        t.mp = {"xmean": [mean[i] for i in t.idx], "xq": [diag[i] for i in t.idx],
                "xvar": [diag[i] - shift for i in t.idx]}
        for q in QUANTITIES:
            setattr(t, q, DD(t.mp[q]))
        return t


def _gram_mp(X, beta, s, delta):
    """The Gram matrix as rows of mpf from fp64 inputs taken exactly (``_mp_ref.truth``'s)."""
    Xm = M._rows(X)
    bt = [mpf(float(v)) for v in np.asarray(beta, dtype=np.float64).reshape(-1)]
    n = len(Xm)
    A = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            A[i][j] = A[j][i] = mpf(float(s)) * M.kernel_exp(Xm[i], Xm[j], bt)
        A[i][i] = mpf(float(s)) + mpf(float(delta))
    return A, Xm, bt


@functools.lru_cache(maxsize=None)
def factor_mp(regime: str, n: int):
    """(columns of L^-1, z, w) of one problem as mpf, by ``_mp_ref``'s column Cholesky and
    forward substitution at DPS + GUARD_DIGITS (see ``chain_truth``)."""
    p = problem(regime, n)
    with mp.workdps(DPS + GUARD_DIGITS):
        A, _, _ = _gram_mp(p.X, p.beta, p.s, p.delta)
        wm = [mpf(float(v)) for v in p.w.tolist()]
        _, C, _, z = M._factor_truth(A, wm)
        return C, z, wm


@functools.lru_cache(maxsize=None)
def chain_truth(regime: str, n: int, plan: str) -> XTruth:
    """The chain's truth.  The shift is the exact s + delta - s_pred of the fp64 hyperparameters
    (so a whole-design fold has xvar = s_pred).

    Carried at DPS + GUARD_DIGITS = 65 digits from the Gram matrix on, so that the result is good
    to 50: inverting Q_FF from a 50-digit L^-1 loses cond(A) ~ 5e8 on the 1-D grid (measured:
    6e-44 against the prior at n = 64), which would leave the truth short of the 1e-45 its own
    test asks.  The L^-1 here rounds to ``truth_of(regime, n).Linv.hi`` (asserted on the CPU)."""
    p = problem(regime, n)
    C, z, wm = factor_mp(regime, n)
    with mp.workdps(DPS + GUARD_DIGITS):
        shift = mpf(p.s) + mpf(p.delta) - mpf(p.s_pred)
    return _truth_from(C, z, wm, folds_of(n, plan), shift, n, GUARD_DIGITS)


def kernel_truth(Linv, w, folds, shift) -> XTruth:
    """gp_xval's own truth: the fp64 array ``Linv`` (logical [i][j], only its lower triangle is
    read), ``w`` and ``shift`` (None for 0) as exact binary inputs."""
    Linv = np.asarray(Linv, dtype=np.float64)
    n = Linv.shape[0]
    with mp.workdps(DPS):
        cols = [[mpf(0)] * j + [mpf(v) for v in Linv[j:, j].tolist()] for j in range(n)]
        wm = [mpf(v) for v in np.asarray(w, dtype=np.float64).tolist()]
        z = [mp.fdot([cols[k][i] for k in range(i + 1)], wm[:i + 1]) for i in range(n)]
        sh = mpf(0) if shift is None else mpf(float(shift))
    return _truth_from(cols, z, wm, folds, sh, n)


@functools.lru_cache(maxsize=None)
def kernel_truth_hi(regime: str, n: int, plan: str) -> XTruth:
    """``kernel_truth`` of the truth's L^-1 rounded to fp64 (``truth_of(...).Linv.hi``)."""
    p = problem(regime, n)
    return kernel_truth(truth_of(regime, n).Linv.hi, p.w, folds_of(n, plan), shift_of(p))


def refit_mp(regime: str, n: int, folds):
    """(xmean, xvar) as {index: mpf} by brute force: for every fold the GP refitted on the
    design without F and predicting at X[F] with s_pred, by ``_mp_ref.truth``'s formulas (Gram,
    column Cholesky, V = L^-1 K*, mean = V^T z, var = s_pred - |V|^2) at DPS + GUARD_DIGITS; an
    empty remainder predicts the prior.  Call the results' comparison under the same workdps."""
    p = problem(regime, n)
    mean, var = {}, {}
    with mp.workdps(DPS + GUARD_DIGITS):
        sm, spm = mpf(p.s), mpf(p.s_pred)
        for F in listed(folds, n):
            rest = np.setdiff1d(np.arange(n), F)
            if rest.size == 0:
                for i in F:
                    mean[i], var[i] = mpf(0), spm
                continue
            A, Xm, bt = _gram_mp(p.X[rest], p.beta, p.s, p.delta)
            L = M._chol_mp(A)
            Xf = M._rows(p.X[F])
            cols = [[sm * M.kernel_exp(xf, xr, bt) for xr in Xm] for xf in Xf] + \
                   [[mpf(float(v)) for v in p.w[rest].tolist()]]
            sol = []
            for c in cols:                                   # forward substitution L v = c
                v = []
                for i in range(len(c)):
                    v.append((c[i] - mp.fdot(L[i][:i], v)) / L[i][i])
                sol.append(v)
            for k, i in enumerate(F):
                mean[i] = mp.fdot(sol[k], sol[-1])
                var[i] = spm - mp.fdot(sol[k], sol[k])
    return mean, var


def refit_dd(regime: str, n: int, F):
    """(mean, var) DD of one fold by ``_mp_ref.truth`` itself on the design without F."""
    p = problem(regime, n)
    rest = np.setdiff1d(np.arange(n), F)
    t = M.truth(p.X[rest], p.X[np.asarray(F, dtype=int)], p.w[rest], p.beta, p.s, p.delta,
                p.s_pred)
    return t.mean, t.var


# -------------------------------------------------------------------------------------- noise
def floor_of(quantity: str, t: XTruth, p) -> float:
    if quantity == "xvar":
        return 4.0 * EPS * p.s_pred
    scale = getattr(t, quantity).scale()
    wmax = float(np.max(np.abs(p.w)))
    if quantity == "xmean" and scale <= 2.0 ** -100 * wmax:
        scale = wmax         # the whole design left out: the truth is 0 (to its last digits)
    return 4.0 * EPS * scale


def _mapped(folds, inv, n):
    return [[int(inv[i]) for i in F] for F in listed(folds, n)]


def chain_members(p, folds, perm):
    """(xmean, xq, xvar), each (n,) in the design's own order, of the two fp64 restatements of
    the design reordered by ``perm``: _xval_ref.closed_form on the oracle's Gram and on the
    device-order Gram."""
    inv = np.argsort(perm)
    X, w = p.X[perm], p.w[perm]
    fp = _mapped(folds, inv, p.n)
    for A in (gp_ref.gram_ardse(X, p.beta, p.s, p.delta), M.device_gram(X, p.beta, p.s, p.delta)):
        mean, xq = _xval_ref.closed_form(A, w, fp, 0.0)
        yield mean[inv], xq[inv], xq[inv] - shift_of(p)


def _worst(t: XTruth, members):
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for mean, xq, xvar in members:
        for q, x in (("xmean", mean), ("xq", xq), ("xvar", xvar)):
            worst[q] = max(worst[q], t.err(q, x))
    return worst


@functools.lru_cache(maxsize=None)
def _chain_raw(regime: str, n: int, plan: str):
    p, t = problem(regime, n), chain_truth(regime, n, plan)
    folds = folds_of(n, plan)
    return _worst(t, (m for perm in M.permutations(n) for m in chain_members(p, folds, perm)))


def chain_noise(quantity: str, regime: str, n: int, plan: str) -> float:
    t = chain_truth(regime, n, plan)
    return max(_chain_raw(regime, n, plan)[quantity], floor_of(quantity, t, problem(regime, n)))


ORDERS = (lambda F: list(F), sorted, lambda F: list(F)[::-1])


def _inverse_by(how: str, Q, al):
    """(Q^-1 al, diag Q^-1); ``cho`` raises LinAlgError where Q does not factor."""
    eye = np.eye(Q.shape[0])
    if how == "inv":
        C = np.linalg.inv(Q)
        return C @ al, np.diag(C).copy()
    if how == "cho":
        c = sla.cho_factor(Q, lower=True, check_finite=False)
        return sla.cho_solve(c, al), np.diag(sla.cho_solve(c, eye)).copy()
    return np.linalg.solve(Q, al), np.diag(np.linalg.solve(Q, eye)).copy()


def kernel_members(Linv, w, folds, shift):
    """The nine fp64 restatements from one fp64 L^-1: three fold orders x three inversions."""
    Lt = np.tril(np.asarray(Linv, dtype=np.float64))
    w = np.asarray(w, dtype=np.float64)
    n = Lt.shape[0]
    z = Lt @ w
    sh = 0.0 if shift is None else float(shift)
    every = listed(folds, n)
    single = np.array([F[0] for F in every if len(F) == 1], dtype=int)
    q1 = np.einsum("ij,ij->j", Lt[:, single], Lt[:, single])
    al1 = Lt[:, single].T @ z
    for order in ORDERS:
        for how in ("inv", "cho", "solve"):
            mean, xq = np.full(n, np.nan), np.full(n, np.nan)
            # the singleton folds at once, each inversion as LAPACK does it at 1 x 1
            if how == "inv":
                xq[single] = 1.0 / q1
                mean[single] = w[single] - xq[single] * al1
            elif how == "cho":
                r = np.sqrt(q1)
                xq[single] = 1.0 / r / r
                mean[single] = w[single] - al1 / r / r
            else:
                xq[single] = 1.0 / q1
                mean[single] = w[single] - al1 / q1
            for F in every:
                if len(F) == 1:
                    continue
                F = np.asarray(order(F), dtype=int)
                P = Lt[:, F]
                x, d = _inverse_by(how, P.T @ P, P.T @ z)
                mean[F], xq[F] = w[F] - x, d
            yield mean, xq, xq - sh


def kernel_noise(Linv, w, folds, shift, t: XTruth, p) -> dict:
    """{quantity: noise} of the kernel layer for this fp64 L^-1 against its kernel truth ``t``."""
    raw = _worst(t, kernel_members(Linv, w, folds, shift))
    return {q: max(raw[q], floor_of(q, t, p)) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def kernel_noise_hi(regime: str, n: int, plan: str) -> dict:
    p = problem(regime, n)
    return kernel_noise(truth_of(regime, n).Linv.hi, p.w, folds_of(n, plan), shift_of(p),
                        kernel_truth_hi(regime, n, plan), p)


def every_q_factors(regime: str, n: int, plan: str) -> int:
    """LAPACK's Cholesky of every fold's Q_FF in every fp64 restatement of both layers (raises
    LinAlgError where one does not factor); returns how many were factored."""
    p = problem(regime, n)
    folds, count = folds_of(n, plan), 0
    for perm in M.permutations(n):
        inv = np.argsort(perm)
        X = p.X[perm]
        for A in (gp_ref.gram_ardse(X, p.beta, p.s, p.delta),
                  M.device_gram(X, p.beta, p.s, p.delta)):
            L = np.linalg.cholesky(A)
            Li = sla.solve_triangular(L, np.eye(n), lower=True)
            Q = Li.T @ Li
            for F in _mapped(folds, inv, n):
                np.linalg.cholesky(Q[np.ix_(F, F)])
                count += 1
    Lt = np.tril(truth_of(regime, n).Linv.hi)
    for F in listed(folds, n):
        for order in ORDERS:
            P = Lt[:, np.asarray(order(F), dtype=int)]
            np.linalg.cholesky(P.T @ P)
            count += 1
    return count


# ------------------------------------------------------- the explicit-inverse term (chain layer)
# (quantity, regime, n, plan) at which the device's chain was measured above MARGIN x noise
# (MI355X): only on the 1-D grid from one full 64-block on, where the
# factorisation's products with explicit block inverses (see _mp_ref.explicit_inverse_term)
# carry cond(L_kk) into L^-1 and so into everything gp_xval forms from it.  Everything else,
# and the whole kernel layer, is held to MARGIN x noise alone.
FINDINGS = frozenset(
    [(q, "grid", 64, "loo") for q in QUANTITIES] +
    [(q, "grid", 65, plan) for q in QUANTITIES for plan in ("loo", "split")] +
    [("xmean", "grid", 130, plan) for plan in ("loo", "big", "mid", "thirds", "late",
                                                "late_pair")] +
    [("xvar", "grid", 130, plan) for plan in ("loo", "big", "mid", "thirds", "late",
                                               "late_pair")] +
    [("xq", "grid", 130, plan) for plan in ("loo", "big", "mid", "thirds", "late_pair")])


@functools.lru_cache(maxsize=None)
def _explicit_errors(regime: str, n: int, plan: str):
    """The closed form applied to ``_mp_ref.explicit_factor``'s L^-1 of the device-order Gram,
    over the ensemble's orderings and both blockings: largest error against the chain truth."""
    p, t = problem(regime, n), chain_truth(regime, n, plan)
    folds = folds_of(n, plan)

    def members():
        for perm in M.permutations(n):
            inv = np.argsort(perm)
            G = M.device_gram(p.X[perm], p.beta, p.s, p.delta)
            w = p.w[perm]
            for sizes in M.BLOCKINGS:
                _, Xi = M.explicit_factor(G, sizes)
                Q = Xi.T @ Xi
                alpha = Xi.T @ (Xi @ w)
                mean, xq = np.full(n, np.nan), np.full(n, np.nan)
                for F in _mapped(folds, inv, n):
                    C = np.linalg.inv(Q[np.ix_(F, F)])
                    mean[F], xq[F] = w[F] - C @ alpha[F], np.diag(C)
                yield mean[inv], xq[inv], xq[inv] - shift_of(p)
    return _worst(t, members())


def explicit_inverse_term(quantity: str, regime: str, n: int, plan: str) -> float:
    """What the factorisation's explicit-inverse arithmetic adds to the chain's noise at a
    documented finding, 0 anywhere else: the emulated error less the noise, capped by the closed
    form (block_condition - 1) x noise, exactly as ``_mp_ref.explicit_inverse_term``."""
    if (quantity, regime, n, plan) not in FINDINGS:
        return 0.0
    nz = chain_noise(quantity, regime, n, plan)
    emulated = max(0.0, _explicit_errors(regime, n, plan)[quantity] - nz)
    return min(emulated, (M.block_condition(regime, n) - 1.0) * nz)


def chain_limit(quantity: str, regime: str, n: int, plan: str) -> float:
    return MARGIN * (chain_noise(quantity, regime, n, plan) +
                     explicit_inverse_term(quantity, regime, n, plan))


# ------------------------------------------------------------------------------ exact scaling
# w -> 2^j w and L^-1 -> 2^-k L^-1 (with shift -> 4^k shift) are exact on the device as long as
# no intermediate of the kernels leaves the normal range with room for its rounding: a sum of
# fp64 numbers is a multiple of its smallest term's ulp, and a product carries the product of the
# ulps, so if every leaf and every product term keeps its magnitude inside [2^-GUARD, 2^GUARD]
# after the scaling (GUARD = 960 leaves 2^62 to the normal range's ends: 52 bits for a term's
# ulp and 10 for the differing summation orders), every intermediate is either normal or exactly
# representable and rounds as the unscaled one does.  ``magnitudes`` restates the kernels'
# intermediates in numpy, each with its degree (dL, dw) in L^-1 and in w: a scaling by
# (2^-k, 2^j) multiplies it by 2^(-k dL + j dw).
GUARD = 960
K_W, K_LINV = 300, 100            # the exponents the device test uses: the issue's aim


def magnitudes(Linv, w, folds, shift):
    """{(dL, dw): (smallest non-zero, largest) magnitude} over gp_xval's intermediates."""
    Lt = np.tril(np.asarray(Linv, dtype=np.float64))
    w = np.asarray(w, dtype=np.float64)
    n = Lt.shape[0]
    out = {}

    def put(deg, a):
        a = np.abs(np.asarray(a, dtype=np.float64)).ravel()
        a = a[a > 0]
        if a.size:
            lo, hi = out.get(deg, (np.inf, 0.0))
            out[deg] = (min(lo, float(a.min())), max(hi, float(a.max())))

    z = Lt @ w
    put((1, 0), Lt)
    put((0, 1), w)
    put((1, 1), Lt * w[None, :])
    put((1, 1), z)
    if shift is not None:
        put((-2, 0), [shift])
    for F in listed(folds, n):
        P = Lt[:, F]
        Q, al = P.T @ P, P.T @ z
        put((2, 0), P[:, :, None] * P[:, None, :])
        put((2, 0), Q)
        put((2, 1), P * z[:, None])
        put((2, 1), al)
        R = np.linalg.cholesky(Q)
        Mi = sla.solve_triangular(R, np.eye(len(F)), lower=True)
        C = Mi.T @ Mi
        y = Mi @ al
        put((1, 0), R)
        put((2, 0), R[:, None, :] * R[None, :, :])
        put((-1, 0), Mi)
        put((0, 0), R[:, :, None] * Mi[None, :, :])
        put((1, 1), Mi * al[None, :])
        put((1, 1), y)
        put((0, 1), Mi * y[:, None])
        put((0, 1), Mi.T @ y)
        put((0, 1), w[F] - Mi.T @ y)
        put((-2, 0), Mi * Mi)
        put((-2, 0), np.diag(C))
        if shift is not None:
            put((-2, 0), np.diag(C) - shift)
    return out


def scaling_allowed(mags, k: int, j: int) -> bool:
    """Every intermediate stays in [2^-GUARD, 2^GUARD] under L^-1 -> 2^-k L^-1, w -> 2^j w."""
    for (dL, dw), (lo, hi) in mags.items():
        e = -k * dL + j * dw
        if np.log2(lo) + e < -GUARD or np.log2(hi) + e > GUARD:
            return False
    return True


def largest_k(mags, which: str, cap: int) -> int:
    """The largest K <= cap with both +K and -K allowed (0 needs the unscaled run allowed)."""
    if not scaling_allowed(mags, 0, 0):
        return -1
    K = 0
    while K < cap:
        nxt = K + 1
        ok = all(scaling_allowed(mags, *((sg * nxt, 0) if which == "Linv" else (0, sg * nxt)))
                 for sg in (1, -1))
        if not ok:
            break
        K = nxt
    return K
