"""The 50-digit reference itself (tests/_mp_ref.py): truth against the fp64 oracle, every regime
factorisable under LAPACK, the device-order emulation inside its derived bound, the noise level
finite and above its floor.  No GPU."""
import numpy as np
import pytest
import scipy.linalg as sla
from mpmath import mp, mpf

from oracle import gp_ref

import _mp_ref as M

EPS = M.EPS
CASES = [(r, n) for r in M.REGIMES for n in M.SIZES]


@pytest.mark.parametrize("n", M.SIZES)
def test_truth_agrees_with_oracle_mid(n):
    """The truth and oracle.gp_ref at the mid regime: 16 eps of each quantity's scale (the
    regime's condition number is ~1e3 and the oracle is backward stable, so this is loose only
    by the factor the noise tests measure)."""
    p, t = M.problem("mid", n), M.truth_of("mid", n)
    G = gp_ref.gram_ardse(p.X, p.beta, p.s, p.delta)
    L, info = gp_ref.cholesky(G)
    assert info == 0
    Linv = sla.solve_triangular(L, np.eye(n), lower=True)
    z = sla.solve_triangular(L, p.w, lower=True)
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    alpha = sla.cho_solve((L, True), p.w)
    mean, var = gp_ref.predict(p.X, p.Xs, p.w, p.beta, p.s, p.delta, p.s_pred)
    nll = 0.5 * z @ z + 0.5 * logdet
    got = {"A": G, "L": L, "Linv": Linv, "logdet": logdet, "z": z, "nll": nll, "alpha": alpha,
           "mean": mean, "var": var}
    for q, x in got.items():
        tq = getattr(t, q)
        scale = {"var": p.s_pred, "logdet": max(n, abs(float(t.logdet.hi))),
                 "nll": max(n, abs(float(t.logdet.hi)))}.get(q, tq.scale())
        assert tq.err(x) <= 16 * EPS * scale, (q, tq.err(x) / (EPS * scale))


def test_truth_is_self_consistent():
    """L L^T = A, L^-1 L = I and A alpha = w far below fp64 (the truth's own 50 digits), from
    the double-double pairs at n = 5."""
    t = M.truth_of("grid", 5)
    ld = np.longdouble
    A, L, Li = (x.hi.astype(ld) + x.lo.astype(ld) for x in (t.A, t.L, t.Linv))
    al = t.alpha.hi.astype(ld) + t.alpha.lo.astype(ld)
    w = np.array([float(v) for v in t.w_mp])
    assert np.max(np.abs(L @ L.T - A)) <= 1e-18
    assert np.max(np.abs(Li @ L - np.eye(5))) <= 1e-18 * np.max(np.abs(Li))
    assert np.max(np.abs(A @ al - w)) <= 1e-18 * np.max(np.abs(al))


@pytest.mark.parametrize("regime,n", CASES)
def test_every_regime_factorises(regime, n):
    """No regime may be left out on the GPU for being indefinite in fp64: LAPACK factorises the
    design as given and its 8 permutations, with the oracle's Gram and the device-order one."""
    p = M.problem(regime, n)
    for perm in M.permutations(n):
        X = p.X[perm]
        np.linalg.cholesky(gp_ref.gram_ardse(X, p.beta, p.s, p.delta))
        np.linalg.cholesky(M.device_gram(X, p.beta, p.s, p.delta))


def test_regimes_are_what_the_table_says():
    for n in M.SIZES:
        d8 = [M.problem(r, n) for r in M.D8]
        for p in d8[1:]:
            assert p.X is not None and np.array_equal(p.X, d8[0].X)
            assert np.array_equal(p.Xs, d8[0].Xs) and np.array_equal(p.w, d8[0].w)
        assert M.problem("d32", n).d == 32 and M.problem("d12", n).d == 12
        g = M.problem("grid", n)
        assert g.d == 1 and np.array_equal(g.X[:, 0], np.linspace(1 / 8, 7 / 8, n))
        assert d8[0].m == min(6, n) + min(6, n * (n - 1) // 2) + 12
        assert np.all(M.problem("flat", n).beta == 0) and M.problem("flat", n).s == 1 / 0.3
        for p in d8:
            assert p.s_pred == p.s + 0.01
    # the first test points are training points: the variance's cancelling regime
    p = M.problem("mid", 65)
    assert all(any(np.array_equal(x, row) for row in p.X) for x in p.Xs[:6])


def _sweep_pairs(rng, count, lo, hi):
    """Pairs of d-vectors (d drawn in 1 .. 32) whose weighted distance lands in [lo, hi]: a
    random direction, then the first coordinate's gap sets what the others leave."""
    out = []
    while len(out) < count:
        d = int(rng.integers(1, 33))
        beta = rng.uniform(0.0, 1.0, d) * 10.0 ** rng.uniform(-2, 2.6)
        beta[rng.random(d) < 0.2] = 0.0
        beta[0] = 10.0 ** rng.uniform(-1, 2.6)
        a, b = rng.uniform(-1, 1, d), rng.uniform(-1, 1, d)
        rest = float(np.sum(beta[1:] * (a[1:] - b[1:]) ** 2))
        target = rng.uniform(lo, hi)
        if rest >= target:
            b[1:] = a[1:] + (b[1:] - a[1:]) * np.sqrt(0.5 * target / rest)
            rest = float(np.sum(beta[1:] * (a[1:] - b[1:]) ** 2))
        b[0] = a[0] + np.sqrt((target - rest) / beta[0])
        out.append((a, b, beta, float(2.0 ** rng.integers(-20, 21))))
    return out


@pytest.mark.parametrize("kind,lo,hi", [("normal", 0.0, 700.0), ("subnormal", 708.4, 745.1),
                                         ("underflow", 745.2, 1300.0)])
def test_device_order_emulation_inside_bound(kind, lo, hi):
    """The numpy restatement of ardse_kernel's arithmetic (no fma) stays within bound_rel of the
    50-digit kernel value, + 2^-1074 for a subnormal result, over a seeded sweep constructed to
    land in the normal range, in the subnormal window of exp and past underflow."""
    rng = np.random.default_rng({"normal": 1, "subnormal": 2, "underflow": 3}[kind])
    worst, seen = 0.0, 0
    for a, b, beta, s in _sweep_pairs(rng, 700, lo, hi):
        got = M.device_values(a[None], b[None], beta, s)[0, 0]
        bnd = M.bound_rel(a[None], b[None], beta)[0, 0]
        with mp.workdps(M.DPS):
            e = M.kernel_values(a[None], b[None], beta, 1.0)[0][0]
            t = mpf(s) * e
            in_kind = {"normal": e >= mpf(2) ** -1022,
                       "subnormal": mpf(2) ** -1075 < e < mpf(2) ** -1022,
                       "underflow": e < mpf(2) ** -1075}[kind]
            seen += bool(in_kind)
            err = abs(mpf(float(got)) - t)
            lim = mpf(float(bnd)) * t + mpf(2) ** -1074
            assert err <= lim, (kind, float(err), float(lim), s)
            if t >= mpf(2) ** -1000:
                worst = max(worst, float(err / (mpf(float(bnd)) * t)))
        assert got >= 0.0 and not np.signbit(got)
    assert seen >= 600, (kind, seen)
    assert worst <= 1.0


def test_extended_factors_track_the_truth():
    """factor_extended (the yardstick of the permuted ensemble members for L, L^-1, z) on the
    design as given agrees with the 50-digit factors to 1 % of the regime's noise + 1 eps."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63     # a 64-bit significand, not a double
    for regime in ("mid", "flat", "grid"):
        t = M.truth_of(regime, 65)
        L, Li, z = M.factor_extended(t, np.arange(65))
        for q, x in (("L", L), ("Linv", Li), ("z", z)):
            tq = getattr(t, q)
            ref = tq.hi.astype(np.longdouble) + tq.lo.astype(np.longdouble)
            err = float(np.max(np.abs(x - ref)))
            lim = 0.01 * M.noise(q, regime, 65) + 2.0 ** -60 * tq.scale()
            assert err <= lim, (regime, q, err)


@pytest.mark.parametrize("regime,n", CASES)
def test_noise_is_finite_and_above_floor(regime, n):
    t = M.truth_of(regime, n)
    for q in M.QUANTITIES:
        v = M.noise(q, regime, n)
        assert np.isfinite(v) and v > 0.0, (q, v)
        assert v >= M.floor_of(q, t), (q, v)
    if regime == "sharp" and n > 1:
        assert M.noise("var", regime, n) == M.floor_of("var", t)   # exact: the floor is needed


def test_explicit_inverse_restatement():
    """The numpy restatement of the library's explicit-inverse blocked factorisation is right on
    a benign matrix in both blockings (L L^T = A, L^-1 L = I at rounding level); on the 1-D grid,
    whose diagonal blocks are as ill-conditioned as the matrix, its error is well above the
    noise and below the closed form cond(L_kk) x noise."""
    p = M.problem("mid", 130)
    G = gp_ref.gram_ardse(p.X, p.beta, p.s, p.delta)
    for sizes in M.BLOCKINGS:
        L, X = M.explicit_factor(G, sizes)
        assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(X, 1) == 0)
        assert np.max(np.abs(L @ L.T - G)) <= 64 * EPS
        assert np.max(np.abs(X @ L - np.eye(130))) <= 1e-11
    for q in ("L", "Linv", "alpha", "mean", "var"):
        assert M.explicit_inverse_term(q, "grid", 65) >= 10 * M.noise(q, "grid", 65), q
    for n in (64, 65, 130):
        kappa = M.block_condition("grid", n)
        assert 1e3 <= kappa <= 1e5, kappa
        for q in M.QUANTITIES:
            assert M._explicit_errors("grid", n)[q] <= kappa * M.noise(q, "grid", n), (q, n)
    assert M.block_condition("sharp", 130) <= 1.01 and M.block_condition("mid", 130) <= 10


def test_limit_is_margin_times_noise_outside_the_findings():
    """The extra term exists only at the documented findings: everywhere else the bound is
    16 x noise exactly, and at a finding it is finite and at most 16 cond(L_kk) x noise."""
    assert M.MARGIN == 16.0
    assert all(r == "grid" and n >= 64 for _, r, n in M.FINDINGS)
    for regime in M.REGIMES:
        for n in M.SIZES:
            for q in M.QUANTITIES:
                lim, nz = M.limit(q, regime, n), M.noise(q, regime, n)
                if (q, regime, n) in M.FINDINGS:
                    assert 16.0 * nz < lim <= 16.0 * M.block_condition(regime, n) * nz
                else:
                    assert M.explicit_inverse_term(q, regime, n) == 0.0 and lim == 16.0 * nz
