"""The PCA front end at 80 digits (mpmath), its regimes, and the fp64 noise level per regime.

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.  The companion of
tests/_mp_ref.py (the GP chain) for everything that chain consumes: the column statistics, the
symmetric eigensolver, the randomized SVD, the basis K and the PC weights.

* Truth (``mp.dps = 80``: B B^T squares the grading, so 50 digits would leave too few below the
  smallest eigenvalue; inputs are the exact binary values of the fp64 arrays): ``stats``,
  ``eig``, ``rsvd``, ``basis``, ``weights``.  ``rsvd`` is the reference's algorithm in exact
  arithmetic -- Y = X Omega, q power steps, any orthonormal basis Q of range(Y), B = Q^T X,
  eigsy(B B^T), S, U = Q U_B, Vh = S^-1 U_B^T B.  S, U and Vh depend on range(Y) only, so this
  is the truth for any correct implementation; vectors are fixed up to sign, and up to a rotation
  inside a cluster.  Results are ``_mp_ref.DD`` pairs.
* ``ensemble``: X = U diag(sigma) V^T + 1e-3 sigma_min noise (the noise of unit 2-norm and
  orthogonal to the signal's left and right subspaces), seeded,
  for the regimes of ``REGIMES``; ``stats_ensemble`` and ``eig_input`` the inputs of the
  statistics and eigensolver tests.
* ``noise``: the largest error against the truth over fp64 restatements built from
  ``oracle.gp_ref`` alone (the data as given, 8 row permutations of X un-permuted afterwards, 8
  column permutations of Omega, which leave range(Y) unchanged; 8 symmetric permutations for the
  eigensolver), never below 4 eps of the quantity's scale.  A test asks
  ``error <= MARGIN * noise``.
* ``FINDINGS``: where the device was measured above that and the cause is the library's
  documented arithmetic (svd.py: S and Vh from the eigendecomposition of B B^T; Q from CholeskyQR3
  or its staged rank-revealing fallback), the bound is ``MARGIN * (noise + build_term)``; see the
  derivation above ``build_arithmetic_svd``.
"""
from __future__ import annotations

import functools

import numpy as np
from mpmath import mp, mpf

from oracle import gp_ref

from _mp_ref import DD, EPS, MARGIN

DPS = 80
NPERM = 8
SHAPE = (40, 300, 12)                           # n, ny, p
REGIMES = ("d2", "d4", "d6", "cluster", "deficient", "centred16")
SVD_CASES = REGIMES + ("d4k",)                  # d4 once more with k = None (r = 2p = 24)
RANK_DEFICIENT = 8
GAP = 1e-6                                      # relative gap below which vectors form a cluster
RESOLVED = 1e-2                                 # noise(S_i) <= RESOLVED S_i: S_i is resolved


# ---------------------------------------------------------------------------- mpmath helpers
def _mat(a):
    return [[mpf(v) for v in row] for row in np.asarray(a, dtype=np.float64).tolist()]


def _tr(A):
    return [list(c) for c in zip(*A)]


def _mmt(A, Bt):
    """A B with B given by its transpose's rows (= its columns)."""
    return [[mp.fdot(r, c) for c in Bt] for r in A]


def _mm(A, B):
    return _mmt(A, _tr(B))


def _dd(rows):
    rows = [list(r) for r in rows]
    return DD((v for r in rows for v in r), (len(rows), len(rows[0]) if rows else 0))


def wide(t: DD):
    """hi + lo in numpy's extended precision (projectors and residuals are formed in it)."""
    return t.hi.astype(np.longdouble) + t.lo.astype(np.longdouble)


# ------------------------------------------------------------------------------------- truth
def stats(Y, floor):
    """mu, sd (ddof = 1, floored; a single row has no sample deviation and yields the floor, as
    gpfit.h documents) and y_std = (Y - mu) / sd, as DD arrays."""
    Y = np.asarray(Y, dtype=np.float64)
    n, ny = Y.shape
    with mp.workdps(DPS):
        cols = _tr(_mat(Y)) if ny else []
        fl = mpf(float(floor))
        mu, sd, ys = [], [], []
        for c in cols:
            m = mp.fsum(c) / n
            v = mp.sqrt(mp.fsum((x - m) ** 2 for x in c) / (n - 1)) if n > 1 else mpf(0)
            v = fl if v < fl else v
            mu.append(m)
            sd.append(v)
            ys.append([(x - m) / v for x in c])
        return DD(mu), DD(sd), _dd(_tr(ys)) if ny else DD([], (n, 0))


def eig(A):
    """Eigenvalues of the symmetric fp64 matrix A, descending (mp.eigsy)."""
    A = np.asarray(A, dtype=np.float64)
    with mp.workdps(DPS):
        if A.shape[0] == 0:
            return DD([])
        E = mp.eigsy(mp.matrix(_mat(A)), eigvals_only=True)
        return DD(sorted((E[i] for i in range(A.shape[0])), reverse=True))


class SVDTruth:
    """S (p), U (n, p), Vh (p, ny) as DD; ``resid`` = ||X - U S Vh||_F; ``r`` the sketch width."""


def _rsvd_mp(Xm, Om, n, p, k, q):
    """The algorithm on rows of mpf (call under workdps): S, rows of U^T, rows of Vh, resid."""
    r = p + (p if k is None else k)
    Xt = _tr(Xm)
    Y = _mm(Xm, Om)                                           # n x r
    for _ in range(q):
        Y = _mm(Xm, _mm(Xt, Y))                               # X (X^T Y)
    if r > n:
        Y, r = [row[:n] for row in Y], n
    Q = mp.qr(mp.matrix(Y), mode="skinny")[0]                 # n x r, orthonormal
    Qt = [[Q[i, j] for i in range(n)] for j in range(r)]
    B = _mm(Qt, Xm)                                           # r x ny
    E, UB = mp.eigsy(mp.matrix(_mmt(B, B)))
    order = sorted(range(r), key=lambda i: -E[i])[:p]
    S = [mp.sqrt(E[i]) if E[i] > 0 else mpf(0) for i in order]
    UBt = [[UB[a, i] for a in range(r)] for i in order]       # rows: eigenvectors of B B^T
    Ut = _mmt(UBt, _tr(Qt))                                   # rows of (Q U_B)^T
    tiny = S[0] * mpf(10) ** -60
    Vh = [[v / s if s > tiny else mpf(0) for v in row] for s, row in zip(S, _mm(UBt, B))]
    # U_p S_p Vh_p = U_p U_p^T X, an orthogonal projection of X: the residual by Pythagoras
    tot = mp.fsum(v * v for row in Xm for v in row)
    resid = mp.sqrt(max(tot - mp.fsum(s * s for s in S), mpf(0)))
    return S, Ut, Vh, resid, r


def rsvd(X, omega, p, k, q):
    X = np.asarray(X, dtype=np.float64)
    with mp.workdps(DPS):
        S, Ut, Vh, resid, r = _rsvd_mp(_mat(X), _mat(omega), X.shape[0], p, k, q)
        t = SVDTruth()
        t.S, t.U, t.Vh, t.resid, t.r = DD(S), _dd(_tr(Ut)), _dd(Vh), float(resid), r
        return t


def basis(S, Vh, p, n):
    """K = diag(S[:p]) Vh[:p] / sqrt(n) (DD, p x ny)."""
    with mp.workdps(DPS):
        s, v = _mat(np.asarray(S).reshape(1, -1))[0], _mat(Vh)
        rt = mp.sqrt(mpf(n))
        return _dd([[s[i] * x / rt for x in v[i]] for i in range(p)])


def weights(y_std, K):
    """(w_hat, LamSim) = (y_std K^T (K K^T)^-1, diag(K K^T)) as DD, (n, p) and (p,)."""
    with mp.workdps(DPS):
        Km, Ym = _mat(K), _mat(y_std)
        G = _mmt(Km, Km)
        R = _mmt(Ym, Km)                                      # n x p
        p = len(Km)
        Gi = mp.inverse(mp.matrix(G))                         # 80 digits against cond(G) <= 1e24
        cols = [[Gi[i, j] for i in range(p)] for j in range(p)]
        return _dd(_mmt(R, cols)), DD([G[i][i] for i in range(p)])


# --------------------------------------------------------------------------------- ensembles
def _orthonormal(rng, rows, cols):
    return np.linalg.qr(rng.standard_normal((rows, cols)))[0]


def sigma_of(regime, p):
    if regime in ("d2", "d4", "d6"):
        return np.logspace(0.0, -float(regime[1]), p)
    if regime == "cluster":
        return np.concatenate([[3.0, 2.0], 1.0 + 1e-9 * np.arange(4), 2.0 ** -np.arange(1, p - 5)])
    if regime == "centred16":
        return np.logspace(0.0, -2.0, p)
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def ensemble(regime, n=SHAPE[0], ny=SHAPE[1], p=SHAPE[2]):
    """X (n, ny), read-only.  ``deficient``: a product of small-integer factors (n x 8)(8 x ny),
    exact in fp64, so X has rank 8 exactly and no noise term; ``centred16``: the column means
    subtracted (rank n - 1 up to the subtraction's rounding)."""
    rng = np.random.default_rng(sum(map(ord, regime)) + 7 * n)
    if regime == "deficient":
        X = rng.integers(-8, 9, (n, RANK_DEFICIENT)).astype(np.float64) @ \
            rng.integers(-8, 9, (RANK_DEFICIENT, ny)).astype(np.float64) / 64.0
    else:
        sig = sigma_of(regime, p)
        U, V = _orthonormal(rng, n, p), _orthonormal(rng, ny, p)
        N = rng.standard_normal((n, ny))
        N -= U @ (U.T @ N)                # the noise lies outside the signal's two subspaces, so
        N -= (N @ V) @ V.T                # it does not move sigma (the cluster keeps its gaps)
        X = (U * sig) @ V.T + 1e-3 * sig.min() * N / np.linalg.norm(N, 2)
        if regime == "centred16":
            X = X - X.mean(axis=0)
    X.setflags(write=False)
    return X


def case_params(case):
    """(regime, n, ny, p, k) of a randomized-SVD case."""
    n, ny, p = SHAPE
    if case == "d4k":
        return "d4", n, ny, p, None
    if case == "centred16":
        return case, 16, ny, 16, 0
    return case, n, ny, p, 0


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(X, Omega float32 (ny, r), p, k, q = 1)."""
    regime, n, ny, p, k = case_params(case)
    X = ensemble(regime, n, ny, p)
    r = 2 * p if k is None else p + k
    om = np.random.default_rng(99 + r).standard_normal((ny, r)).astype(np.float32)
    om.setflags(write=False)
    return X, om, p, k, 1


def compared(case):
    """How many leading singular triplets the case defines: the numerical rank where it is
    below p (the rest belong to zero singular values and are arbitrary)."""
    regime, n, _, p, _ = case_params(case)
    return RANK_DEFICIENT if regime == "deficient" else (n - 1 if regime == "centred16" else p)


STAT_KINDS = ("offset", "unit", "constant", "one_off", "below_floor", "above_floor")


@functools.lru_cache(maxsize=None)
def stats_ensemble(n, ny, floor=1e-6):
    """Y (n, ny), read-only, whose column c is of kind STAT_KINDS[c % 6]: mean 1e8 with sd 1e-3; mean 0 with
    sd 1; constant; constant but for one element (which walks down the rows); a +a / -a / 0
    pattern whose deviation is the floor less, and plus, about one ulp."""
    rng = np.random.default_rng(1000 * n + ny)
    Y = np.empty((n, ny))
    pat = np.zeros(n)
    pat[: n - n % 2] = np.tile([1.0, -1.0], n // 2)
    spread = np.sqrt((n - n % 2) / max(n - 1, 1))        # sd of the pattern
    for c in range(ny):
        kind = STAT_KINDS[c % 6]
        if kind == "offset":
            Y[:, c] = 1e8 + 1e-3 * rng.standard_normal(n)
        elif kind == "unit":
            Y[:, c] = rng.standard_normal(n)
        elif kind in ("constant", "one_off"):
            Y[:, c] = rng.uniform(-3.0, 3.0)
            if kind == "one_off":
                Y[(c // 6) % n, c] += 0.5
        else:
            a = floor * (1.0 + (-2.0 if kind == "below_floor" else 2.0) * EPS)
            Y[:, c] = pat * (a / spread if spread else a)
    Y.setflags(write=False)
    return Y


EIG_KINDS = ("graded", "cluster", "indefinite", "diagonal", "diagonal_tiny",
             "diagonal_tiny_live", "zero")


@functools.lru_cache(maxsize=None)
def eig_input(kind, r):
    """Symmetric r x r fp64 input (read-only): Q Lambda Q^T rounded, or the diagonal kinds."""
    rng = np.random.default_rng(31 * r + EIG_KINDS.index(kind))
    i = np.arange(r)
    if kind == "zero":
        A = np.zeros((r, r))
    elif kind.startswith("diagonal"):
        rng = np.random.default_rng(31 * r)                               # one diagonal for all
        A = np.diag(rng.choice([3.0, -1.0, 0.5, 2.0, 0.0, 7.25], r))     # unsorted, repeats
        if kind != "diagonal" and r > 1:
            A[0, r - 1] = A[r - 1, 0] = 1e-200        # theta^2 overflows: the identity rotation
        if kind == "diagonal_tiny_live" and r >= 4:
            # one off-diagonal of 1e-200 alone squares to 0 and the solve stops before any
            # rotation; a second, live pivot makes the sweeps reach the tiny one
            A[0, 0], A[r - 1, r - 1] = 3.0, -1.0
            A[1, 2] = A[2, 1] = 0.25
    else:
        lam = {"graded": 10.0 ** (-14.0 * i / max(r - 1, 1)),
               "cluster": 1.0 + i * 2.0 ** -40,
               "indefinite": np.linspace(-1.0, 1.0, r) if r > 1 else np.array([-1.0])}[kind]
        Q = _orthonormal(rng, r, r)
        A = (Q * rng.permutation(lam)) @ Q.T
        A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def eig_truth(kind, r):
    return eig(eig_input(kind, r))


# ------------------------------------------------------------------------------------- noise
def _perms(n, base):
    return [np.random.default_rng(base + s).permutation(n) for s in range(NPERM)]


def _align(x, ref, axis):
    """x with each vector (along ``axis``) given the sign of its truth."""
    sgn = np.sign(np.sum(x * ref, axis=axis, keepdims=True))
    sgn[sgn == 0] = 1.0
    return x * sgn


def vector_errors(U, Vh, t: SVDTruth):
    """Per-triplet max-abs error of the sign-aligned columns of U and rows of Vh."""
    eu = np.max(np.abs((_align(U, t.U.hi, 0) - t.U.hi) - t.U.lo), axis=0)
    ev = np.max(np.abs((_align(Vh, t.Vh.hi, 1) - t.Vh.hi) - t.Vh.lo), axis=1)
    return eu, ev


def projector_error(Z, T, idx, rows):
    """max |P - P_truth| of the projector on the vectors ``idx`` (columns of Z, T when ``rows``
    is False, rows otherwise), formed in extended precision."""
    ld = np.longdouble
    Z, T = np.asarray(Z, dtype=np.float64).astype(ld), wide(T)
    if rows:
        Z, T = Z.T, T.T
    Z, T = Z[:, idx], T[:, idx]
    return float(np.max(np.abs(Z @ Z.T - T @ T.T)))


def residual(X, U, S, Vh):
    """||X - U diag(S) Vh||_F in extended precision."""
    ld = np.longdouble
    R = np.asarray(X).astype(ld) - (np.asarray(U).astype(ld) * np.asarray(S).astype(ld)) @ \
        np.asarray(Vh).astype(ld)
    return float(np.sqrt(np.sum(R * R)))


def _svd_members(X, om, p, k, q, fn):
    """fn on the data as given, on NPERM row permutations of X (U un-permuted) and on NPERM
    column permutations of Omega."""
    yield fn(X, p, k, q, om)
    for perm in _perms(X.shape[0], 2000):
        U, S, Vh = fn(X[perm], p, k, q, om)
        yield U[np.argsort(perm)], S, Vh
    for perm in _perms(om.shape[1], 3000):
        yield fn(X, p, k, q, om[:, perm])


def _ref_svd(X, p, k, q, om):
    return gp_ref.randomized_svd(X, p, k=k, q=q, omega=om)


@functools.lru_cache(maxsize=None)
def svd_truth(case):
    X, om, p, k, q = case_inputs(case)
    return rsvd(X, om, p, k, q)


def _svd_errors(case, fn):
    """Largest error over the members of ``fn``: S, U, Vh per triplet; UtU and resid scalars."""
    X, om, p, k, q = case_inputs(case)
    t = svd_truth(case)
    w = {"S": np.zeros(p), "U": np.zeros(p), "Vh": np.zeros(p), "UtU": 0.0, "resid": 0.0}
    members = []
    for U, S, Vh in _svd_members(X, om, p, k, q, fn):
        U, S, Vh = (np.asarray(a, dtype=np.float64) for a in (U, S, Vh))
        members.append((U, S, Vh))
        w["S"] = np.maximum(w["S"], np.abs((S - t.S.hi) - t.S.lo))
        eu, ev = vector_errors(U, Vh, t)
        w["U"], w["Vh"] = np.maximum(w["U"], eu), np.maximum(w["Vh"], ev)
        w["UtU"] = max(w["UtU"], float(np.max(np.abs(U.T @ U - np.eye(p)))))
        w["resid"] = max(w["resid"], abs(residual(X, U, S, Vh) - t.resid))
    return w, members


@functools.lru_cache(maxsize=None)
def _svd_noise(case):
    w, members = _svd_errors(case, _ref_svd)
    t = svd_truth(case)
    s0 = float(t.S.hi[0])
    w["S"] = np.maximum(w["S"], 4.0 * EPS * s0)
    w["U"], w["Vh"] = np.maximum(w["U"], 4.0 * EPS), np.maximum(w["Vh"], 4.0 * EPS)
    w["UtU"], w["resid"] = max(w["UtU"], 4.0 * EPS), max(w["resid"], 4.0 * EPS * s0)
    ident, clusters = classify(case, w["S"])
    w["VVt"] = 4.0 * EPS
    for c, idx in enumerate(clusters):
        w[f"PU{c}"] = w[f"PV{c}"] = 4.0 * EPS
    for U, S, Vh in members:
        V = Vh[ident]
        w["VVt"] = max(w["VVt"], float(np.max(np.abs(V @ V.T - np.eye(len(ident))))))
        for c, idx in enumerate(clusters):
            w[f"PU{c}"] = max(w[f"PU{c}"], projector_error(U, t.U, idx, False))
            w[f"PV{c}"] = max(w[f"PV{c}"], projector_error(Vh, t.Vh, idx, True))
    return w


def classify(case, noise_S=None):
    """(identifiable indices, clusters) among the case's compared triplets.  S_i is resolved when
    noise(S_i) <= 1e-2 S_i; resolved neighbours closer than a relative 1e-6 form a cluster
    (compared by projector); a resolved vector whose gap to both neighbours exceeds 1e-6 is
    identifiable (compared after sign alignment); the rest are left out."""
    if noise_S is None:
        noise_S = _svd_noise(case)["S"]
    S = svd_truth(case).S.hi
    m = compared(case)
    ok = [bool(noise_S[i] <= RESOLVED * S[i]) for i in range(m)]
    near = [abs(S[i] - S[i + 1]) <= GAP * max(S[i], S[i + 1]) for i in range(len(S) - 1)]
    ident, clusters, run = [], [], []
    for i in range(m):
        left = i > 0 and near[i - 1]
        right = i + 1 < len(S) and near[i]
        if ok[i] and not left and not right:
            ident.append(i)
        if ok[i] and (left or right):
            run.append(i)
        if run and (not ok[i] or not right or i == m - 1):
            if len(run) > 1:
                clusters.append(run)
            run = []
    return ident, clusters


def noise(quantity, case):
    """What fp64 delivers for ``quantity`` in a randomized-SVD case: per triplet for S, U, Vh;
    scalars for UtU, VVt (identifiable rows), resid and the cluster projectors PU<c> / PV<c>."""
    return _svd_noise(case)[quantity]


def eig_noise(kind, r):
    """(eigenvalue noise, |V^T V - I| level, |A V - V W| level) of np.linalg.eigh over A and its
    NPERM symmetric permutations; floors 4 eps ||A||_2, 4 eps r, 4 eps r ||A||_2."""
    return _eig_noise(kind, r)


@functools.lru_cache(maxsize=None)
def _eig_noise(kind, r):
    A, t = eig_input(kind, r), eig_truth(kind, r)
    nrm = float(np.max(np.abs(t.hi))) if r else 0.0
    ev, orth, res = 0.0, 0.0, 0.0
    for perm in [np.arange(r)] + _perms(r, 4000):
        Ap = A[np.ix_(perm, perm)]
        w, V = np.linalg.eigh(Ap)
        ev = max(ev, t.err(w[::-1]))
        orth = max(orth, float(np.max(np.abs(V.T @ V - np.eye(r)))))
        res = max(res, eig_residual(Ap, w, V))
    return max(ev, 4.0 * EPS * nrm), max(orth, 4.0 * EPS * r), max(res, 4.0 * EPS * r * nrm)


def eig_residual(A, w, V):
    """max |A V - V diag(w)| in extended precision."""
    ld = np.longdouble
    A, w, V = (np.asarray(a, dtype=np.float64).astype(ld) for a in (A, w, V))
    return float(np.max(np.abs(A @ V - V * w))) if A.size else 0.0


def stats_noise(Y, floor, truth=None):
    """Per-column noise of (mu, sd) and per-entry-column noise of y_std: gp_ref.standardize on
    the rows as given and on NPERM row permutations, floors 4 eps of the column's own scale
    (max|y|, the truth's sd, max|y_std| + max|y| / sd)."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    mu_t, sd_t, ys_t = truth if truth is not None else stats(Y, floor)
    e_mu = 4.0 * EPS * np.max(np.abs(Y), axis=0)
    e_sd = 4.0 * EPS * sd_t.hi
    # y_std = (y - mu) / sd inherits mu's floor over sd besides its own rounding
    e_ys = 4.0 * EPS * (np.max(np.abs(ys_t.hi), axis=0) + np.max(np.abs(Y), axis=0) / sd_t.hi)
    for perm in [np.arange(n)] + _perms(n, 5000):
        if n > 1:
            mu, sd, ys = gp_ref.standardize(Y[perm], floor)
        else:
            mu = Y[0].copy()
        if n == 1:                       # numpy: NaN; the build (and the truth): the floor
            sd = np.full_like(mu, floor)
            ys = (Y[perm] - mu) / sd
        e_mu = np.maximum(e_mu, np.abs((mu - mu_t.hi) - mu_t.lo))
        e_sd = np.maximum(e_sd, np.abs((sd - sd_t.hi) - sd_t.lo))
        e_ys = np.maximum(e_ys, np.max(np.abs((ys[np.argsort(perm)] - ys_t.hi) - ys_t.lo), axis=0))
    return e_mu, e_sd, e_ys


def weights_noise(y_std, K, truth):
    """Noise of (w_hat per PC column, LamSim per PC): gp_ref.pc_weights on y_std as given, on
    NPERM row permutations (un-permuted) and NPERM column permutations of both operands (the
    locations reordered: the same weights); floors 4 eps of each column's scale."""
    w_t, lam_t = truth
    e_w = 4.0 * EPS * np.max(np.abs(w_t.hi), axis=0)
    e_l = 4.0 * EPS * lam_t.hi
    n, ny = y_std.shape
    for perm in [np.arange(n)] + _perms(n, 6000):
        w = gp_ref.pc_weights(y_std[perm], K)[np.argsort(perm)]
        e_w = np.maximum(e_w, np.max(np.abs((w - w_t.hi) - w_t.lo), axis=0))
    for perm in [np.arange(ny)] + _perms(ny, 7000):
        Kp = K[:, perm]
        w = gp_ref.pc_weights(y_std[:, perm], Kp)
        e_w = np.maximum(e_w, np.max(np.abs((w - w_t.hi) - w_t.lo), axis=0))
        e_l = np.maximum(e_l, np.abs((np.einsum("ij,ij->i", Kp, Kp) - lam_t.hi) - lam_t.lo))
    return e_w, e_l


# ------------------------------------------------------ the library's own arithmetic (svd.py)
# gladsgp_amd/svd.py departs from the reference's LAPACK calls in two documented places.
#
# (1) svd(B), B = Q^T X (r x ny), comes from the eigendecomposition of the r x r Gram G = B B^T:
# S = sqrt(eig(G)), U_B = its eigenvectors, Vh = S^-1 U_B^T B.  LAPACK's svd(B) is backward stable
# on B itself: dS_i ~ eps S_0, and u_i, v_i are disturbed by eps S_0 / gap(S).  Forming G rounds
# every entry by up to (ny / 2) eps |B||B^T|, and a symmetric eigensolver adds r eps ||G||:
# dG <= delta = (ny / 2 + r) r eps S_0^2 in norm (the factor r bounds ||B||_F^2 / S_0^2).  Hence
#     lambda_i = S_i^2 moves by delta      ->  dS_i <= delta / (sqrt(S_i^2 + delta) + S_i),
# eps S_0^2 / S_i instead of eps S_0: the small singular values lose S_0 / S_i digits;
#     u_B,i turns by delta / gap_i(lambda)  (gap_i the distance of S_i^2 to the other S_j^2),
# and Vh_i = u_B,i^T B / S_i picks up every other right vector S_j v_j with the weight of that
# turn, and the relative error of S_i:  dVh_i <= (delta / gap_i) S_0 / S_i + dS_i / S_i.
#
# (2) Q comes from shifted CholeskyQR3 and, where Y is too ill-conditioned for it, from the
# staged rank-revealing fallback (eigen-directions of R^T R above 1e-5 ||R||, CholeskyQR3,
# deflation R <- (I - Q1 Q1^T) R, again on what is left).  Every deflation rounds R by
# eps ||R|| on top of the eps ||Y|| that the products forming Y left in it, where Householder QR
# commits one backward error of that size in all.  A direction of Y at sigma_i(Y) = (S_i / S_0)^(2q+1)
# ||Y|| is then held to an angle psi_i <= c eps ||Y|| / sigma_i(Y), c = ny + 8 sqrt(n r) (the
# products' inner length and the fallback's own floor), and a direction of X off range(Q) by psi
# is captured as S_i cos(psi):  dS_i <= S_i psi_i^2 / 2, second order, so a constant of 2 in the
# rounding shows as 4 in S; the truncation residual sqrt(||X||^2 - sum S_i^2) moves by
# sum S_i dS_i / resid.
#
# Those closed forms are worst cases over error directions.  The term used is the sharper of the
# two, as in _mp_ref.explicit_inverse_term: the same arithmetic carried out in fp64 numpy
# (build_arithmetic_svd) on the noise ensemble's members, less the noise, capped by the closed
# form.  It is 0 outside FINDINGS.
_U = 2.0 ** -53


def _chol_qr(Y, shift):
    n, r = Y.shape
    G = Y.T @ Y
    if shift:
        G = G + 11.0 * (n * r + r * (r + 1)) * _U * np.trace(G) * np.eye(r)
    L = np.linalg.cholesky(G)                               # LinAlgError on a pivot <= 0
    return np.linalg.solve(L, Y.T).T


def _chol_qr3(Y):
    return _chol_qr(_chol_qr(_chol_qr(Y, True), False), False)


def _project_off(Pm, Z):
    for _ in range(2):
        Z = Z - Pm @ (Pm.T @ Z)
    return Z


def build_orthonormalize(Y, rel_tol=1e-10, seed=0x5EED):
    """svd.py's orthonormalize in numpy: shifted CholeskyQR3, else the staged fallback."""
    n, r = Y.shape
    try:
        return _chol_qr3(Y)
    except np.linalg.LinAlgError:
        pass
    Q, R, floor = np.zeros((n, 0)), Y, None
    while Q.shape[1] < r:
        lam, V = np.linalg.eigh(R.T @ R)
        lam, V = lam[::-1], V[:, ::-1]
        top = float(lam[0])
        if floor is None:
            floor = 64.0 * n * r * _U * _U * max(top, 0.0)
        if not top > floor:
            break
        k = min(int(np.sum(lam > max(rel_tol * top, floor))), r - Q.shape[1])
        Q1 = _chol_qr3(R @ V[:, :k])
        if Q.shape[1]:
            Q1 = _chol_qr(_chol_qr(_project_off(Q, Q1), False), False)
        Q = np.concatenate([Q, Q1], axis=1)
        R = _project_off(Q1, R)
    if Q.shape[1] < r:
        Z = _project_off(Q, np.random.default_rng(seed).standard_normal((r - Q.shape[1], n)).T)
        Q = np.concatenate([Q, _chol_qr(_chol_qr(Z, False), False)], axis=1)
    return Q


def build_arithmetic_svd(X, p, k, q, om):
    """svd.py's documented arithmetic in numpy: Y = X (X^T Y) power steps, its orthonormalize,
    B = Q^T X, eigh(B B^T), S = sqrt, Vh = S^-1 U_B^T B."""
    if k is None:
        k = p
    om = np.asarray(om).astype(np.float32).astype(np.float64)
    Y = X @ om
    for _ in range(q):
        Y = X @ (X.T @ Y)
    Q = build_orthonormalize(Y[:, : X.shape[0]])
    B = Q.T @ X
    lam, UB = np.linalg.eigh(B @ B.T)
    lam, UB = lam[::-1], UB[:, ::-1]
    S = np.sqrt(np.maximum(lam, 0.0))
    with np.errstate(all="ignore"):
        Vh = np.where(S[:, None] != 0.0, (UB.T @ B) / S[:, None], 0.0)
    return (Q @ UB)[:, :p], S[:p], Vh[:p]


# The (quantity, case) pairs at which the device was measured above MARGIN x noise (MI355X,
# DESIGN.md section 7): the smallest singular value of d4 with k = None (r = 24), which the
# reference's Householder QR resolves to 25 eps S_0 while Y's last signal direction sits at
# 1e-12 ||Y|| and takes the staged fallback, and the truncation residual that follows it.  Only
# these carry the extra term.
FINDINGS = frozenset([("S", "d4k"), ("resid", "d4k")])


def gram_delta(case):
    X, om, p, k, q = case_inputs(case)
    t = svd_truth(case)
    return (X.shape[1] / 2.0 + t.r) * t.r * EPS * float(t.S.hi[0]) ** 2


def closed_form(quantity, case):
    """The closed-form worst cases derived above: per triplet for S, U, Vh (inf where a gap is
    0), a scalar for resid."""
    X, om, p, k, q = case_inputs(case)
    t = svd_truth(case)
    S = t.S.hi
    d = gram_delta(case)
    n, ny = X.shape
    with np.errstate(all="ignore"):
        psi = np.minimum(1.0, (ny + 8.0 * np.sqrt(n * t.r)) * EPS * (S[0] / S) ** (2 * q + 1))
        dS = d / (np.sqrt(S * S + d) + S) + 0.5 * S * psi * psi
        if quantity == "S":
            return dS
        if quantity == "resid":
            return float(np.sum(S * dS) / t.resid) if t.resid > 0 else float("inf")
        lam = S * S
        gap = np.array([np.min(np.abs(np.delete(lam, i) - lam[i])) if len(S) > 1 else np.inf
                        for i in range(len(S))])
        turn = np.where(gap > 0, d / gap, np.inf) + psi
        if quantity == "U":
            return turn
        return np.where(S > 0, turn * S[0] / S + dS / S, np.inf)


@functools.lru_cache(maxsize=None)
def _build_errors(case):
    return _svd_errors(case, build_arithmetic_svd)[0]


def build_term(quantity, case):
    """What the library's own arithmetic adds to the noise at a documented finding (S, U, Vh:
    per triplet; resid: a scalar), 0 anywhere else."""
    if (quantity, case) not in FINDINGS:
        return 0.0 * noise(quantity, case)
    emulated = np.maximum(0.0, _build_errors(case)[quantity] - noise(quantity, case))
    return np.minimum(emulated, closed_form(quantity, case))


def limit(quantity, case):
    """The tests' bound: MARGIN x noise, plus MARGIN x the build's term at the findings."""
    return MARGIN * (noise(quantity, case) + build_term(quantity, case))


# ---------------------------------------------------------- gp_syevj's stop rule, restated
def stop_rule_converged(A, tol=1e-15, normalise=True):
    """eig.hip's convergence test on the input (sweep 0): off <= tol^2 tot over sums of squares
    of the entries, each first scaled by 2^-e, e the exponent of max|a| (clamped to the normal
    range), when ``normalise``; the bare squares otherwise (the rule before the normaliser)."""
    A = np.asarray(A, dtype=np.float64)
    s = 1.0
    if normalise:
        m = float(np.max(np.abs(A))) if A.size else 0.0
        e = int(np.frexp(m)[1]) - 1 if 0.0 < m < np.inf else 0
        s = float(np.ldexp(1.0, -max(e, -1022)))
    with np.errstate(all="ignore"):
        B = A * s
        sq = B * B
        tot = float(np.sum(sq))
        off = float(np.sum(np.where(np.eye(A.shape[0], dtype=bool), 0.0, sq)))
        return bool(off <= tol * tol * tot)
