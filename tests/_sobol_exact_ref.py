"""References for gp_sobol_exact, written from the formulas, not from the kernel.

A unit u has beta_u (d,), s_u and alpha_u (n,); its mean is f_u(x) = s_u sum_n alpha_un prod_k
exp(-beta_uk (x_k - X_nk)^2).  Inputs are uniform on prod_k [lo_k, hi_k], w_k = hi_k - lo_k:

    I_k(u,n)        = sqrt(pi) / (2 r w_k) [erf(r (hi_k - X_nk)) - erf(r (lo_k - X_nk))],
                      r = sqrt(beta_uk)
    J_k(u,n; v,n')  = exp(-(b b'/B) (a - a')^2) sqrt(pi) / (2 sqrt(B) w_k)
                      [erf(sqrt(B) (hi_k - c)) - erf(sqrt(B) (lo_k - c))]
                      b = beta_uk, b' = beta_vk, B = b + b', a = X_nk, a' = X_n'k,
                      c = (b a + b' a') / B
    E_u             = s_u sum_n alpha_un prod_k I_k(u,n)
    Q_tot(u,v)      = s_u s_v sum_nn' alpha_un alpha_vn' prod_k J_k
    Q_main_i(u,v)   = s_u s_v sum_nn' alpha_un alpha_vn' J_i prod_{k != i} I_k(u,n) I_k(v,n')
    Q_not_i(u,v)    = s_u s_v sum_nn' alpha_un alpha_vn' I_i(u,n) I_i(v,n') prod_{k != i} J_k

Two implementations:
  * :func:`np_moments`   numpy / scipy fp64, the bracket sign-aware (erfc(|near|) - erfc(|far|)
                         when both arguments have one sign);
  * :func:`mp_moments`   mpmath at 50 digits (``mp.erf``), the truth; :func:`mp_quad_check`
                         compares its one-dimensional integrals with ``mp.quad``.
Both return E (U,), Q (G, M, M, 2 d + 1) in the order [tot, main_0.., not_0..] and the positive
majorants AE, AQ: the same sums with |alpha_un| and |alpha_un alpha_vn'| (every other factor is
positive), the scale of the rounding error of any fp64 evaluation.

The limit the device is held to (the project's rule, 16 x what fp64 itself delivers):
    tiny cases    16 max(|np - truth|, C0 eps A)
    larger cases  16 C0 eps A   against the restatement
C0 is the restatement's own worst error over the tiny cases in units of eps A, measured once
(tests/test_sobol_exact_ref_cpu.py::test_restatement_against_truth prints it per regime and
asserts it stays below C0), rounded up; it is not taken from the kernel.
"""
import math

import numpy as np

EPS = 2.0 ** -52
# worst |restatement - truth| / (eps A) over TINY_CASES x REGIMES x seeds (0, 1): 2.70 (E,
# widebox), 5.70 (Q, subbox); rounded up
C0 = 6.0
HALF_SQRT_PI = math.sqrt(math.pi) / 2.0

REGIMES = ("plain", "flat", "sharp", "subbox", "widebox", "mixed")
TINY_CASES = [  # (n, d, G, M)
    (1, 1, 1, 1), (7, 1, 1, 2), (5, 2, 2, 1), (24, 3, 1, 2), (13, 3, 1, 1), (9, 2, 1, 2)]


# ------------------------------------------------------------------------------------ the cases
def make_case(n, d, U, regime="plain", seed=0):
    """X on [0,1]^d, beta (U, d), s (U,), alpha (U, n), lo, hi (d,) or None.

    plain    beta in [0.5, 5], the unit box
    flat     beta = 1e-6 in every dimension: V -> 0, Q and E^2 cancel
    sharp    beta = 1e4 in dimension 0: J_0 underflows for most point pairs
    subbox   the box [0.3, 0.6]^d, the design on [0,1]^d: same-sign brackets
    widebox  the box [-1, 2]^d
    mixed    beta differing by 1e4 between consecutive units"""
    rng = np.random.default_rng([seed, n, d, U, REGIMES.index(regime)])
    X = rng.random((n, d))
    beta = rng.uniform(0.5, 5.0, (U, d))
    s = rng.uniform(0.5, 2.0, U)
    alpha = rng.standard_normal((U, n)) * rng.uniform(0.1, 10.0, (U, 1))
    lo = hi = None
    if regime == "flat":
        beta[:] = 1e-6
    elif regime == "sharp":
        beta[:, 0] = 1e4
    elif regime == "subbox":
        lo, hi = np.full(d, 0.3), np.full(d, 0.6)
    elif regime == "widebox":
        lo, hi = np.full(d, -1.0), np.full(d, 2.0)
    elif regime == "mixed":
        beta[1::2] *= 1e4 / 5.0
        beta[0::2] /= 5.0
    return X, beta, s, alpha, lo, hi


def gp_alpha(X, beta, s, delta, w):
    """alpha = (s R + delta I)^-1 w of one unit, R_ij = exp(-sum_k beta_k (X_ik - X_jk)^2)."""
    D = X[:, None, :] - X[None, :, :]
    K = s * np.exp(-np.einsum("ijk,k->ij", D * D, beta)) + delta * np.eye(X.shape[0])
    return np.linalg.solve(K, w)


def conditioned_case(n, d, U, seed=0, delta=1e-4):
    """A well-conditioned GP per unit (the C2 recipe: beta in [0.5, 5], delta >= 1e-4): alpha
    from a smooth response, so the indices are meaningful."""
    rng = np.random.default_rng([seed, n, d, U, 77])
    X = rng.random((n, d))
    beta = rng.uniform(0.5, 5.0, (U, d))
    s = rng.uniform(0.5, 2.0, U)
    c = rng.uniform(0.0, 3.0, d) * (0.5 ** np.arange(d))
    w = np.sin(X @ c) + 0.3 * X[:, 0] * X[:, -1]
    alpha = np.stack([gp_alpha(X, beta[u], s[u], delta, w * (1 + 0.1 * u)) for u in range(U)])
    return X, beta, s, alpha


def _box(lo, hi, d):
    lo = np.zeros(d) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,))
    hi = np.ones(d) if hi is None else np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,))
    return lo, hi


# ------------------------------------------------------------------------------------- numpy
def erf_diff(p, q):
    """erf(p) - erf(q) for p > q, sign-aware."""
    from scipy.special import erf, erfc
    flip = p <= 0
    p2, q2 = np.where(flip, -q, p), np.where(flip, -p, q)
    same = q2 >= 0
    with np.errstate(under="ignore"):
        return np.where(same, erfc(np.where(same, q2, 0.0)) - erfc(np.where(same, p2, 0.0)),
                        erf(p2) - erf(q2))


def _loo(F):
    """prod over the last axis leaving one out, by exclusive prefix / suffix products."""
    one = np.ones(F.shape[:-1] + (1,))
    pre = np.concatenate([one, np.cumprod(F[..., :-1], axis=-1)], axis=-1)
    suf = np.concatenate([np.cumprod(F[..., :0:-1], axis=-1)[..., ::-1], one], axis=-1)
    return pre * suf


def np_one_point(X, beta, lo, hi):
    """I (U, n, d)."""
    r = np.sqrt(beta)[:, None, :]
    x = X[None]
    return HALF_SQRT_PI / (r * (hi - lo)) * erf_diff(r * (hi - x), r * (lo - x))


def np_two_point(X, bu, bv, lo, hi):
    """J (n, n', d) of the unit pair with beta bu, bv."""
    B = bu + bv
    rB = np.sqrt(B)
    a, a2 = X[:, None, :], X[None, :, :]
    dl = a - a2
    with np.errstate(under="ignore"):
        ex = np.exp(-(bu * bv / B) * dl * dl)
    c = (bu / B) * a + (bv / B) * a2
    return ex * (HALF_SQRT_PI / (rB * (hi - lo))) * erf_diff(rB * (hi - c), rB * (lo - c))


def np_moments(X, alpha, beta, s, M=1, lo=None, hi=None):
    X, alpha, beta, s = (np.asarray(v, dtype=np.float64) for v in (X, alpha, beta, s))
    n, d = X.shape
    U = alpha.shape[0]
    G = U // M
    lo, hi = _box(lo, hi, d)
    I = np_one_point(X, beta, lo, hi) if n else np.ones((U, 0, d))
    LI = _loo(I)
    PI = I.prod(-1)
    E = s * (alpha * PI).sum(-1)
    AE = s * (np.abs(alpha) * PI).sum(-1)
    Q = np.zeros((G, M, M, 2 * d + 1))
    AQ = np.zeros_like(Q)
    for g in range(G):
        for a in range(M):
            for b in range(a, M):
                u, v = g * M + a, g * M + b
                J = np_two_point(X, beta[u], beta[v], lo, hi)
                LJ = _loo(J)
                terms = np.empty((n, n, 2 * d + 1))
                terms[..., 0] = J.prod(-1)
                terms[..., 1:1 + d] = J * LI[u][:, None, :] * LI[v][None, :, :]
                terms[..., 1 + d:] = I[u][:, None, :] * I[v][None, :, :] * LJ
                gw = np.outer(alpha[u], alpha[v])[..., None]
                ss = s[u] * s[v]
                Q[g, a, b] = Q[g, b, a] = ss * (gw * terms).sum((0, 1))
                AQ[g, a, b] = AQ[g, b, a] = ss * (np.abs(gw) * terms).sum((0, 1))
    return dict(E=E, Q=Q, AE=AE, AQ=AQ)


def np_indices(E, Q, M=1):
    """(mean (G,), variance (G,), first (G, d), total (G, d)) of each group's mean function."""
    E = np.asarray(E)
    Q = np.asarray(Q)
    d = (Q.shape[-1] - 1) // 2
    Eb = E.reshape(-1, M).mean(-1)
    Qb = Q.reshape(-1, M, M, 2 * d + 1).mean((1, 2))
    V = Qb[:, 0] - Eb ** 2
    first = (Qb[:, 1:1 + d] - (Eb ** 2)[:, None]) / V[:, None]
    total = (Qb[:, :1] - Qb[:, 1 + d:]) / V[:, None]
    return Eb, V, first, total


def index_tolerance(ref, M, lim):
    """First-order propagation of |dE| <= lim AE, |dQ| <= lim AQ (lim in absolute units of the
    majorant, e.g. 16 C0 eps) through S_i = (Qm_i - Eb^2) / V and T_i = (Qt - Qn_i) / V:
    (tol_first (G, d), tol_total (G, d)), computed from the reference's values alone."""
    Eb, V, first, total = np_indices(ref["E"], ref["Q"], M)
    d = first.shape[1]
    dE = lim * ref["AE"].reshape(-1, M).mean(-1)
    dQ = lim * ref["AQ"].reshape(-1, M, M, 2 * d + 1).mean((1, 2))
    dE2 = 2 * np.abs(Eb) * dE
    dV = dQ[:, 0] + dE2
    aV = np.abs(V)[:, None]
    tf = (dQ[:, 1:1 + d] + dE2[:, None]) / aV + np.abs(first) * dV[:, None] / aV
    tt = (dQ[:, :1] + dQ[:, 1 + d:]) / aV + np.abs(total) * dV[:, None] / aV
    return tf, tt


# ------------------------------------------------------------------------------------ mpmath
def mp_moments(X, alpha, beta, s, M=1, lo=None, hi=None, dps=50):
    """The truth: object arrays of mpf, the layout of :func:`np_moments`."""
    import mpmath as mp
    with mp.workdps(dps):
        X = np.asarray(X, dtype=np.float64)
        n, d = X.shape
        U = len(alpha)
        G = U // M
        lo, hi = _box(lo, hi, d)
        f = mp.mpf
        Xm = [[f(float(X[i, k])) for k in range(d)] for i in range(n)]
        lom, him = [f(float(v)) for v in lo], [f(float(v)) for v in hi]
        bm = [[f(float(beta[u][k])) for k in range(d)] for u in range(U)]
        am = [[f(float(alpha[u][i])) for i in range(n)] for u in range(U)]
        sm = [f(float(v)) for v in s]
        hsp = mp.sqrt(mp.pi) / 2

        def one(b, x, k):
            r = mp.sqrt(b)
            return hsp / (r * (him[k] - lom[k])) * (mp.erf(r * (him[k] - x)) -
                                                    mp.erf(r * (lom[k] - x)))

        def two(b, b2, x, x2, k):
            B = b + b2
            r = mp.sqrt(B)
            c = (b * x + b2 * x2) / B
            return (mp.exp(-(b * b2 / B) * (x - x2) ** 2) * hsp / (r * (him[k] - lom[k])) *
                    (mp.erf(r * (him[k] - c)) - mp.erf(r * (lom[k] - c))))

        def loo(v, i):
            p = f(1)
            for k, x in enumerate(v):
                if k != i:
                    p *= x
            return p

        I = [[[one(bm[u][k], Xm[i][k], k) for k in range(d)] for i in range(n)] for u in range(U)]
        E = np.empty(U, dtype=object)
        AE = np.empty(U, dtype=object)
        for u in range(U):
            pr = [loo(I[u][i], -1) for i in range(n)]
            E[u] = sm[u] * mp.fsum(am[u][i] * pr[i] for i in range(n))
            AE[u] = sm[u] * mp.fsum(abs(am[u][i]) * pr[i] for i in range(n))
        nq = 2 * d + 1
        Q = np.empty((G, M, M, nq), dtype=object)
        AQ = np.empty((G, M, M, nq), dtype=object)
        for g in range(G):
            for a in range(M):
                for b in range(a, M):
                    u, v = g * M + a, g * M + b
                    acc = [f(0)] * nq
                    aacc = [f(0)] * nq
                    for i in range(n):
                        for j in range(n):
                            J = [two(bm[u][k], bm[v][k], Xm[i][k], Xm[j][k], k) for k in range(d)]
                            t = [loo(J, -1)]
                            t += [J[k] * loo(I[u][i], k) * loo(I[v][j], k) for k in range(d)]
                            t += [I[u][i][k] * I[v][j][k] * loo(J, k) for k in range(d)]
                            gw = am[u][i] * am[v][j]
                            for q in range(nq):
                                acc[q] += gw * t[q]
                                aacc[q] += abs(gw) * t[q]
                    ss = sm[u] * sm[v]
                    for q in range(nq):
                        Q[g, a, b, q] = Q[g, b, a, q] = ss * acc[q]
                        AQ[g, a, b, q] = AQ[g, b, a, q] = ss * aacc[q]
        return dict(E=E, Q=Q, AE=AE, AQ=AQ)


def mp_quad_check(b, b2, x, x2, lo, hi, dps=50):
    """The truth's own check: the closed forms of I_k and J_k against ``mp.quad`` of their
    integrands; returns the two relative differences."""
    import mpmath as mp
    with mp.workdps(dps):
        b, b2, x, x2, lo, hi = (mp.mpf(float(v)) for v in (b, b2, x, x2, lo, hi))
        hsp = mp.sqrt(mp.pi) / 2
        r = mp.sqrt(b)
        I = hsp / (r * (hi - lo)) * (mp.erf(r * (hi - x)) - mp.erf(r * (lo - x)))
        B = b + b2
        rB = mp.sqrt(B)
        c = (b * x + b2 * x2) / B
        J = (mp.exp(-(b * b2 / B) * (x - x2) ** 2) * hsp / (rB * (hi - lo)) *
             (mp.erf(rB * (hi - c)) - mp.erf(rB * (lo - c))))
        pts = sorted({lo, hi} | {p for p in (x, x2, c) if lo < p < hi})
        Iq = mp.quad(lambda t: mp.exp(-b * (t - x) ** 2), pts) / (hi - lo)
        Jq = mp.quad(lambda t: mp.exp(-b * (t - x) ** 2 - b2 * (t - x2) ** 2), pts) / (hi - lo)
        return float(abs(I - Iq) / Iq), float(abs(J - Jq) / Jq)


def to_float(a):
    return np.array([float(v) for v in np.asarray(a, dtype=object).reshape(-1)]).reshape(
        np.shape(a))


def err_ratio(got, truth, A):
    """max |got - truth| / (eps A) with the difference taken at the truth's precision."""
    import mpmath as mp
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    truth = np.asarray(truth, dtype=object).reshape(-1)
    A = np.asarray(A, dtype=object).reshape(-1)
    worst = 0.0
    with mp.workdps(50):
        for g, t, a in zip(got, truth, A):
            if a == 0:
                assert g == 0, (g, t)
                continue
            worst = max(worst, float(abs(mp.mpf(float(g)) - t) / (mp.mpf(EPS) * a)))
    return worst


def abs_err(got, truth):
    """|got - truth| per element as float64, the difference taken at the truth's precision."""
    import mpmath as mp
    got = np.asarray(got, dtype=np.float64)
    flat = np.asarray(truth, dtype=object).reshape(-1)
    with mp.workdps(50):
        out = [float(abs(mp.mpf(float(g)) - t)) for g, t in zip(got.reshape(-1), flat)]
    return np.array(out).reshape(got.shape)


# ----------------------------------------------------------------------- quadrature (CPU check)
def quad_moments(X, alpha, beta, s, M=1, lo=None, hi=None, m=40):
    """E and Q by tensor Gauss-Legendre quadrature of f, E[f | x_i] and E[f | x_~i] themselves
    (d <= 3): nothing of the closed form enters."""
    X, alpha, beta, s = (np.asarray(v, dtype=np.float64) for v in (X, alpha, beta, s))
    n, d = X.shape
    U = alpha.shape[0]
    G = U // M
    lo, hi = _box(lo, hi, d)
    z, w = np.polynomial.legendre.leggauss(m)
    nodes = [lo[k] + (hi[k] - lo[k]) * (z + 1) / 2 for k in range(d)]
    wt = w / 2                                             # weights of the uniform density
    F = []
    for u in range(U):
        fac = [np.exp(-beta[u, k] * (nodes[k][None, :] - X[:, k][:, None]) ** 2) for k in range(d)]
        letters = "abc"[:d]
        f = np.einsum(",".join("n" + c for c in letters) + ",n->" + letters, *fac, alpha[u])
        F.append(s[u] * f)

    def integ(f, axes):
        for ax in sorted(axes, reverse=True):
            f = np.tensordot(f, wt, axes=([ax], [0]))
        return f

    E = np.array([integ(f, range(d)) for f in F])
    Q = np.zeros((G, M, M, 2 * d + 1))
    for g in range(G):
        for a in range(M):
            for b in range(M):
                fu, fv = F[g * M + a], F[g * M + b]
                Q[g, a, b, 0] = integ(fu * fv, range(d))
                for i in range(d):
                    others = [k for k in range(d) if k != i]
                    Q[g, a, b, 1 + i] = integ(integ(fu, others) * integ(fv, others), [0])
                    Q[g, a, b, 1 + d + i] = integ(integ(fu, [i]) * integ(fv, [i]),
                                                  range(d - 1))
    return dict(E=E, Q=Q)


# ------------------------------------------------------------- the small emulator (surface tests)
SALTELLI_SEED = 20240611          # the design's and the resampling's seed of the consistency case
SALTELLI_M = 12
SALTELLI_RESAMPLES = 999
SALTELLI_MARGIN = 6.0             # bootstrap standard errors


def small_emulator(n=64, d=3, P=2, S=4, ny=12, seed=3):
    """Everything that defines the small emulator of the surface tests, in numpy: the design t
    (n, d), the ensemble y (n, ny), a fixed PCA basis K (P, ny) (the leading right singular
    vectors of the standardised ensemble, scaled as src/model.py:101), pcvar (P,) and a samples
    dict of S posterior draws.  The device builds its EmulatorModel from (t, y, K); the CPU twin
    uses oracle.gp_ref on the same arrays."""
    rng = np.random.default_rng(seed)
    t = rng.random((n, d))
    modes = rng.standard_normal((P + 1, ny)) * (0.5 ** np.arange(P + 1))[:, None]
    coef = np.stack([np.sin(2.0 * t[:, 0] + k) + (0.6 - 0.2 * k) * t[:, 1] ** 2 +
                     0.4 * t[:, 0] * t[:, -1] for k in range(P + 1)], 1)
    y = 3.0 + coef @ modes + 1e-3 * rng.standard_normal((n, ny))
    mu = y.mean(0)
    sd = y.std(0, ddof=1)
    _, sv, Vh = np.linalg.svd((y - mu) / sd, full_matrices=False)
    K = np.diag(sv[:P]) @ Vh[:P] / np.sqrt(n)
    pcvar = sv[:P] ** 2 / np.sum(sv ** 2)
    samples = {"betaU": rng.uniform(0.5, 5.0, (S, (d + 1) * P)),
               "lamUz": rng.uniform(0.5, 2.0, (S, P)),
               "lamWs": rng.uniform(2000, 10000, (S, P)),
               "lamWOs": rng.uniform(500, 2000, (S, 1))}
    return dict(t=t, y=y, K=K, pcvar=pcvar, samples=samples, n=n, d=d, P=P, S=S)


def group_by_pc(a, S, P):
    """Units (sample, PC) in sample-major order -> the S samples of a PC consecutive."""
    a = np.asarray(a)
    return np.ascontiguousarray(np.swapaxes(a.reshape((S, P) + a.shape[1:]), 0, 1)).reshape(
        (P * S,) + a.shape[1:])


def within_margin(exact, estimate, se, margin=SALTELLI_MARGIN):
    """|exact - estimate| / se, and whether every one lies within the margin."""
    z = np.abs(np.asarray(exact) - np.asarray(estimate)) / np.asarray(se)
    return z, bool((z <= margin).all())
