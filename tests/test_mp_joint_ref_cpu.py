"""The 50-digit reference of the joint covariance, its factor and the draws itself
(tests/_mp_joint_ref.py): the truth against the numpy closed form and against an independent
mpmath route, its diagonal against the chain's 50-digit variance, the factor and the normal
stream self-consistent, the explicit-inverse term ordered and confined to the documented
findings, and the numpy restatement of the library's arithmetic inside the bound the device is
held to.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import rng_ref

import _joint_ref
import _mp_joint_ref as J
import _mp_ref as M
import _xval_ref

EPS = M.EPS
ALL = [(r, n, pts) for r in M.REGIMES for n, pts in J.CASES]


def _ld(x):
    return x.hi.astype(np.longdouble) + x.lo.astype(np.longdouble)


def test_point_sets_are_what_the_design_says():
    for regime in ("mid", "grid", "d32"):
        for n in J.WIDE_N:
            p = M.problem(regime, n)
            for pts, m in J.WIDE.items():
                Xs = J.points(regime, n, pts)
                assert Xs.shape == (m, p.d)
                on = sum(any(np.array_equal(x, row) for row in p.X) for x in Xs)
                assert on >= m // 4                               # taken exactly
                near = sum(0 < np.min(np.max(np.abs(p.X - x), axis=1)) < 2.0 ** -16 for x in Xs)
                assert near >= m // 4 - 1                         # moved by 2^-20 N(0, 1)
                uniq = np.unique(Xs, axis=0).shape[0]
                assert uniq <= m - m // 4                         # exact repeats
                if regime == "grid":
                    assert Xs.min() >= 0.125 - 2.0 ** -15 and Xs.max() <= 0.875 + 2.0 ** -15
    for r in M.D8[1:]:
        for n, pts in J.CASES:
            assert np.array_equal(J.points(r, n, pts), J.points("mid", n, pts))
    assert J.points("mid", 130, "one").shape == (1, 8)
    assert J.points("mid", 65, "std") is M.problem("mid", 65).Xs


@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("n,pts", [(5, "std"), (65, "std"), (65, "wide65")])
def test_truth_against_the_closed_form(regime, n, pts):
    """tests/_joint_ref.closed_form (LAPACK, the oracle's Gram) is one member of the ensemble's
    kind, so it sits within MARGIN x noise of the truth; the truth is symmetric to its last bit."""
    p, Xs = M.problem(regime, n), J.points(regime, n, pts)
    t = J.truth_cov(regime, n, pts, 2.0 ** -30 * p.s)
    C = _joint_ref.closed_form(p.X, Xs, p.beta, p.s, p.delta, p.s_pred, 2.0 ** -30 * p.s)
    err, nz = t.err(C), J.noise_cov(regime, n, pts, 2.0 ** -30 * p.s)
    print(f"{regime} n={n} {pts}: |closed form - truth| = {err:.3e}, noise {nz:.3e}")
    assert err <= M.MARGIN * nz
    assert np.array_equal(t.hi, t.hi.T) and np.array_equal(t.lo, t.lo.T)


def test_truth_against_lu_solve_at_17_5():
    """test_joint_cpu.py's route (mp.lu_solve of the Gram, no Cholesky, no V) at (n, m) = (17, 5)
    on the same inputs: the two 50-digit results agree to 1e-45 s."""
    n, m, d = 17, 5, 3
    p = _xval_ref.problem(n, d, 0)
    Xs = _joint_ref.test_points(n, m, d)
    X, beta, s, delta, sp = p["X"], p["beta"], p["s"], p["delta"], p["s_pred"]
    with mp.workdps(M.DPS):
        Xm, Xsm = J._mp_rows(X), J._mp_rows(Xs)
        bt = [mpf(float(v)) for v in beta]
        sm = mpf(float(s))
        A = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                A[i, j] = sm * M.kernel_exp(Xm[i], Xm[j], bt) + (mpf(float(delta)) if i == j else 0)
        Ks = mp.matrix(n, m)
        for i in range(n):
            for j in range(m):
                Ks[i, j] = sm * M.kernel_exp(Xm[i], Xsm[j], bt)
        Sol = mp.matrix(n, m)
        for j in range(m):
            Sol[:, j] = mp.lu_solve(A, Ks[:, j])
        Q = Ks.T * Sol
        # truth_cov's own steps (gram_chol_mp, cov_core_mp, diag_mp) on the same arrays
        T = J.truth_cov_mp(X, Xs, beta, s, delta, sp, 1e-3)
        for i in range(m):
            for j in range(m):
                pr = (mpf(float(sp)) + mpf(1e-3)) if i == j else \
                    sm * M.kernel_exp(Xsm[i], Xsm[j], bt)
                assert abs(T[i][j] - (pr - Q[i, j])) <= mpf(10) ** -45 * sm, (i, j)
        C = _joint_ref.closed_form(X, Xs, beta, s, delta, sp, 1e-3)
        worst = max(abs(T[i][j] - mpf(float(C[i, j]))) for i in range(m) for j in range(m))
    assert worst <= 1e-11 * s


@pytest.mark.parametrize("regime,n,pts", [("mixed", 5, "wide65"), ("grid", 65, "std"),
                                          ("d12", 1, "one"), ("flat", 0, "std")])
def test_truth_cov_is_truth_cov_mp_of_the_regime_arrays(regime, n, pts):
    """The cached, regime-keyed truth_cov (what the GPU tests consume) is the array-level
    function the lu_solve test checks, on the regime's arrays: a double-double holds 2^-105 of
    an entry, the comparison asks 2^-100 of s_pred."""
    p, Xs = M.problem(regime, n), J.points(regime, n, pts)
    jit = 2.0 ** -30 * p.s
    T = J.truth_cov_mp(p.X, Xs, p.beta, p.s, p.delta, p.s, jit)
    t = J.truth_cov(regime, n, pts, jit, nugget=False)
    m = Xs.shape[0]
    with mp.workdps(M.DPS):
        worst = max(abs(T[i][j] - (mpf(float(t.hi[i, j])) + mpf(float(t.lo[i, j]))))
                    for i in range(m) for j in range(m))
        assert worst <= mpf(2) ** -100 * mpf(p.s_pred)


@pytest.mark.parametrize("regime,n", [(r, n) for r in M.REGIMES for n in M.SIZES])
def test_diagonal_is_the_chain_variance(regime, n):
    """For "std" the diagonal of truth_cov and truth_of(...).var are the same 50-digit quantity
    by two routes (forward substitution here, the explicit 50-digit L^-1 there)."""
    t, var = J.truth_cov(regime, n, "std"), M.truth_of(regime, n).var
    idx = np.diag_indices(t.hi.shape[0])
    diff = (t.hi[idx].astype(np.longdouble) - var.hi) + (t.lo[idx].astype(np.longdouble) - var.lo)
    # a double-double holds 2^-105 of the value: that is what this comparison can resolve
    assert float(np.max(np.abs(diff))) <= 2.0 ** -100 * M.problem(regime, n).s_pred


@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("n", [1, 5])
def test_diagonal_is_the_chain_variance_at_50_digits(regime, n):
    """The same two routes compared on the mpf values themselves: 1e-45."""
    p = M.problem(regime, n)
    _, vv = J._core(regime, n, "std")
    Xm, bt, sm, L = J._chol_of(regime, n)
    with mp.workdps(M.DPS):
        Cc = M._linv_mp(L)                                  # columns of L^-1
        for q, xs in enumerate(J._mp_rows(p.Xs)):
            k = [sm * M.kernel_exp(xs, Xm[i], bt) for i in range(n)]
            v = [mp.fsum(Cc[j][i] * k[j] for j in range(i + 1)) for i in range(n)]
            assert abs(mp.fdot(v, v) - vv[q]) <= mpf(10) ** -45


def test_symmetry_jitter_and_no_training_points():
    p = M.problem("mixed", 5)
    t0, tj = J.truth_cov("mixed", 5, "wide65"), J.truth_cov("mixed", 5, "wide65", 0.25)
    off = ~np.eye(65, dtype=bool)
    assert np.array_equal(t0.hi[off], tj.hi[off]) and np.array_equal(t0.lo[off], tj.lo[off])
    d = (_ld(tj) - _ld(t0))[np.diag_indices(65)]
    assert np.max(np.abs(d - 0.25)) <= 2.0 ** -60
    tn = J.truth_cov("mixed", 5, "wide65", 0.0, nugget=False)
    assert np.max(np.abs((_ld(t0) - _ld(tn))[np.diag_indices(65)] - (p.s_pred - p.s))) <= 2.0 ** -60
    # n = 0: the prior, s_pred + jitter itself on the diagonal, in every regime
    for regime in M.REGIMES:
        p0 = M.problem(regime, 0)
        assert p0.X.shape == (0, p0.d) and p0.m == 12
        pr = J.truth_cov(regime, 0, "std", 0.25)
        want = _joint_ref.prior(p0.Xs, p0.beta, p0.s, p0.s_pred, 0.25)
        assert np.array_equal(np.diag(pr.hi), np.diag(want))
        assert not pr.lo[np.diag_indices(12)].any()
        assert pr.err(want) <= 16 * EPS * p0.s
        assert np.array_equal(pr.hi, pr.hi.T)
        assert J.noise_cov(regime, 0, "std", 0.25) == 4 * EPS * p0.s_pred


@pytest.mark.parametrize("regime,pts", [("mid", "std"), ("grid", "wide65"), ("flat", "one")])
def test_truth_factor_reproduces_its_matrix(regime, pts):
    C = J.truth_cov(regime, 65 if pts != "one" else 130, pts).hi
    R, logdet = J.truth_factor(C)
    Rl = _ld(R)
    assert np.all(np.triu(R.hi, 1) == 0) and np.all(np.triu(R.lo, 1) == 0)
    # longdouble carries 2^-64: the product of the double-double factor returns C to that
    assert np.max(np.abs(Rl @ Rl.T - C)) <= 2.0 ** -55 * np.max(C)
    with mp.workdps(M.DPS):
        m = C.shape[0]
        rows = [[mpf(float(R.hi[i, j])) + mpf(float(R.lo[i, j])) for j in range(m)]
                for i in range(m)]
        worst = max(abs(mp.fdot(rows[i], rows[j]) - mpf(float(C[i, j])))
                    for i in range(m) for j in range(i + 1))
        # the pairs themselves hold 2^-105 of an entry
        assert worst <= mpf(2) ** -95 * mpf(float(np.max(C)))
        ld = 2 * mp.fsum(mp.log(rows[i][i]) for i in range(m))
        assert abs(ld - (mpf(float(logdet.hi)) + mpf(float(logdet.lo)))) <= mpf(2) ** -90 * m
    nR, nld = J.noise_factor(C)
    assert nR >= 4 * EPS * R.scale() and np.isfinite(nR) and np.isfinite(nld) and nld > 0


@pytest.mark.parametrize("regime,n,pts", [("grid", 5, "std"), ("mid", 65, "wide65")])
def test_truth_factor_at_50_digits(regime, n, pts):
    """R R^T = C to 1e-45 on truth_factor's own mpf values (factor_mp: what it splits into
    pairs), here on the nearly singular matrix without the nugget at its derived jitter."""
    C = J.truth_cov(regime, n, pts, J.sufficient_jitter(regime, n, pts), nugget=False).hi
    with mp.workdps(M.DPS):
        R, _ = J.factor_mp(C)
        m = C.shape[0]
        worst = max(abs(mp.fdot(R[i][:j + 1], R[j][:j + 1]) - mpf(float(C[i, j])))
                    for i in range(m) for j in range(i + 1))
        assert worst <= mpf(10) ** -45
    got, _ = J.truth_factor(C)
    assert got.err(np.array([[float(R[i][j]) for j in range(m)] for i in range(m)])) <= \
        2.0 ** -52 * got.scale()


def test_normals_against_the_fp64_stream():
    """oracle.rng_ref.normals against the 50-digit stream.  numpy rounds 2 pi u2 (up to 2 pi:
    half an ulp is 2 eps, and fl(2 pi) is off by 1.1 eps at u2 = 1) before the cosine, so an
    element r cos(.) owes the truth 4 eps r absolute from the angle, and 4 eps of itself from
    log, sqrt, cos and the product: within a few ulp of its own size wherever |cos| is not
    small, and within 4 eps of its radius r (this pair's own, r^2 = z_even^2 + z_odd^2) next
    to a zero.  The draw bound uses the worst relative error, printed here, and each element's
    own error."""
    N, seed, offset = 4096, 2024, 5
    z = rng_ref.normals(N, seed, offset)
    zm = J.normals_mp(N, seed, offset)
    rel, absolute = 0.0, 0.0
    with mp.workdps(M.DPS):
        for e_idx, (got, t) in enumerate(zip(z.tolist(), zm)):
            e = abs(mpf(got) - t)
            absolute = max(absolute, float(e))
            rel = max(rel, float(e / abs(t)))
            r = mp.sqrt(zm[e_idx & ~1] ** 2 + zm[e_idx | 1] ** 2)
            assert e <= 4 * EPS * abs(t) + 4 * EPS * r, (got, float(e))
    print(f"normals: worst relative error {rel:.3e} = {rel / EPS:.1f} eps, absolute "
          f"{absolute:.3e}")
    assert rel == J.normals_rel_error(N, seed, offset)
    assert float(np.max(J.normals_abs_error(N, seed, offset))) == absolute
    assert J.normals_mp(N, seed, offset, start=1001) == zm[1001:]
    assert J.normals_mp(7, seed, offset) == zm[:7]
    # the moments of a standard normal, to 5 standard errors
    assert abs(z.mean()) <= 5 / np.sqrt(N) and abs(z.var() - 1) <= 5 * np.sqrt(2 / N)


def test_truth_draws_layout():
    rng = np.random.default_rng(5)
    R, mean = rng.standard_normal((2, 4, 4)), rng.standard_normal((2, 4))
    t, mag, magerr = J.truth_draws(R, mean, 11, 3, 3, unit0=1)
    want, wmag = _joint_ref.draws(R, mean, 11, 3, 3, unit0=1)
    assert t.err(want) <= 16 * EPS * np.max(wmag)
    assert np.max(np.abs(mag + np.abs(mean)[:, None, :] - wmag)) <= 16 * EPS * np.max(wmag)
    # the per-element weighting is never above the worst relative error's, never below 4 eps
    rel = max(J.normals_rel_error(3 * 3 * 4, 11, 3, 3 * 4), 4 * EPS)
    assert np.all(magerr <= rel * mag * (1 + 8 * EPS))
    assert np.all(magerr >= 4 * EPS * mag * (1 - 8 * EPS))


@pytest.mark.parametrize("n", [64, 65, 130])
def test_explicit_term_is_ordered_at_the_findings(n):
    """The closed-form cap (block_condition - 1) x noise is never below the evaluated error."""
    for _, pts in [c for c in J.CASES if c[0] == n]:
        nz = J.noise_cov("grid", n, pts)
        ev = J.explicit_error_cov("grid", n, pts)
        cap = J.explicit_cap_cov("grid", n, pts)
        term = J.explicit_term_cov("grid", n, pts)
        print(f"grid n={n} {pts}: noise {nz:.3e}, explicit {ev / nz:.3g}, cap {cap / nz:.3g}")
        assert max(0.0, ev - nz) <= cap
        assert term == max(0.0, ev - nz)
        assert J.limit_cov("grid", n, pts) == M.MARGIN * (nz + term)


def test_no_finding_hides_a_failure():
    """FINDINGS_COV is the grid from one full 64-block on and nothing else: 3 of the 5 sizes of
    1 of the 7 regimes."""
    assert J.FINDINGS_COV == {("grid", 64), ("grid", 65), ("grid", 130)}
    flagged = [c for c in ALL if (c[0], c[1]) in J.FINDINGS_COV]
    grid = [c for c in ALL if c[0] == "grid" and c[1] in (64, 65, 130)]
    assert flagged == grid and len(flagged) <= len(grid)
    for regime, n, pts in ALL:
        if (regime, n) not in J.FINDINGS_COV:
            assert J.explicit_term_cov(regime, n, pts) == 0.0
            assert J.limit_cov(regime, n, pts) == M.MARGIN * J.noise_cov(regime, n, pts)


@pytest.mark.parametrize("regime,n,pts", ALL)
def test_restatement_inside_the_bound(regime, n, pts):
    """The numpy restatement of the library's arithmetic (blocked explicit inverse, V = X K*^T,
    both blockings, every ordering) is within the bound the device will be held to: outside the
    findings that is MARGIN x noise alone."""
    nz, lim = J.noise_cov(regime, n, pts), J.limit_cov(regime, n, pts)
    ev = J.explicit_error_cov(regime, n, pts)
    p = M.problem(regime, n)
    print(f"{regime} n={n} {pts}: noise {nz / (EPS * p.s_pred):.3g} eps s_pred, restatement "
          f"{ev / nz:.3g} x noise")
    assert np.isfinite(nz) and nz >= 4 * EPS * p.s_pred
    assert ev <= lim
    if (regime, n) not in J.FINDINGS_COV:
        assert ev <= M.MARGIN * nz


def test_epilogue_bound_holds_for_its_numpy_restatement():
    """fma-free numpy in jc_syrk_kernel's order (t = xa - xb, dist += (beta t) t) against the
    50-digit kernel value, inside bound_rel_epilogue over the normal range."""
    rng = np.random.default_rng(9)
    for d in (1, 8, 9, 17, 32):
        A, B = rng.random((40, d)), rng.random((30, d))
        A[:, 0] += rng.uniform(0, 25, 40)
        beta = rng.uniform(0.0, 3.0, d)
        beta[0] = 1.0
        t = A[:, None, :] - B[None, :, :]
        acc = np.zeros((40, 30))
        for k in range(d):
            acc = acc + (beta[k] * t[:, :, k]) * t[:, :, k]
        got = 2.0 ** 20 * np.exp(-acc)
        bound = J.bound_rel_epilogue(A, B, beta)
        truth = M.kernel_values(A, B, beta, 2.0 ** 20)
        with mp.workdps(M.DPS):
            for i in range(40):
                for j in range(30):
                    assert abs(mpf(float(got[i, j])) - truth[i][j]) <= \
                        mpf(float(bound[i, j])) * truth[i][j]


def test_derived_jitter():
    """J = 2 (m E + F): F from Higham's Theorem 10.3, E the max-abs bound on C."""
    m = 130
    F = J.potrf_backward(m, 1.0)
    assert m * (m + 1) / 2 * m * EPS <= F <= 1.01 * m * (m + 1) / 2 * m * EPS
    for regime in ("mid", "grid"):
        p = M.problem(regime, 130)
        jit = J.sufficient_jitter(regime, 130, "wide130")
        E = J.limit_cov(regime, 130, "wide130", jit, False)
        assert jit >= 2 * (m * E + J.potrf_backward(m, p.s)) > 0
        lam = J.lambda_min(regime, 130, "wide130")
        assert abs(lam) <= J.potrf_backward(m, p.s)          # singular: the exact repeats
        print(f"{regime}: derived jitter {jit / p.s:.3e} s, default 1e-8 s, lambda_min "
              f"{lam / p.s:.2e} s")
