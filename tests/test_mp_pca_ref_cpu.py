"""The 80-digit PCA reference itself (tests/_mp_pca_ref.py): the exact-arithmetic randomized SVD
on a constructed rank-p matrix, the unit pieces, the identifiability caps of every regime from
the reference restatements alone, the rank-deficient path, and gp_syevj's stop rule restated with
and without its normaliser.  No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import gp_ref

import _mp_pca_ref as P
from _mp_ref import DD

EPS = P.EPS


def _gram_schmidt(cols):
    """Orthonormal columns (lists of mpf) by two passes of modified Gram-Schmidt."""
    out = []
    for v in cols:
        for _ in range(2):
            for u in out:
                d = mp.fdot(u, v)
                v = [a - d * b for a, b in zip(v, u)]
        nv = mp.sqrt(mp.fdot(v, v))
        out.append([a / nv for a in v])
    return out


def test_rsvd_recovers_a_constructed_rank_p_matrix():
    """X = U diag(sigma) V^T built in mpmath and left unrounded, rank p exactly: range(X Omega)
    is range(X), so the exact-arithmetic algorithm returns sigma itself and orthonormal right
    vectors, to 1e-60."""
    n, ny, p = 9, 14, 4
    rng = np.random.default_rng(5)
    sig = [3.0, 1.0, 1e-3, 1e-9]
    with mp.workdps(P.DPS):
        U = _gram_schmidt(P._mat(rng.standard_normal((p, n))))       # p rows of length n
        V = _gram_schmidt(P._mat(rng.standard_normal((p, ny))))
        Xm = [[mp.fsum(mpf(s) * U[j][a] * V[j][b] for j, s in enumerate(sig)) for b in range(ny)]
              for a in range(n)]
        Om = P._mat(rng.standard_normal((ny, p)).astype(np.float32))
        S, Ut, Vh, resid, r = P._rsvd_mp(Xm, Om, n, p, 0, 1)
        assert r == p
        for s, ref in zip(S, sig):
            assert abs(s - mpf(ref)) <= mpf(10) ** -60 * mpf(ref), (float(s), ref)
        G = P._mmt(Vh, Vh)
        H = P._mmt(Ut, Ut)
        for i in range(p):
            for j in range(p):
                assert abs(G[i][j] - (i == j)) <= mpf(10) ** -60, (i, j)
                assert abs(H[i][j] - (i == j)) <= mpf(10) ** -60, (i, j)
        assert resid <= mpf(10) ** -30                     # the square root of a 1e-80 residue


def test_dd_round_trip():
    with mp.workdps(P.DPS):
        vals = [mp.pi, -mp.e * mpf(10) ** -30, mpf(1) / 3, mpf(0)]
        d = DD(vals)
        for v, hi, lo in zip(vals, d.hi, d.lo):
            assert abs(mpf(float(hi)) + mpf(float(lo)) - v) <= abs(v) * mpf(2) ** -104
        assert d.err(d.hi) <= np.max(np.abs(d.hi)) * EPS and d.err(d.hi) == np.max(np.abs(d.lo))


def test_eig_truth_closed_form():
    """[[a, b], [b, c]]: (a + c) / 2 +- sqrt(((a - c) / 2)^2 + b^2), at a graded 2 x 2."""
    a, b, c = 1.0, 1e-7, 1e-14
    t = P.eig(np.array([[a, b], [b, c]]))
    with mp.workdps(P.DPS):
        h = mp.sqrt(((mpf(a) - mpf(c)) / 2) ** 2 + mpf(b) ** 2)
        for got_hi, got_lo, ref in zip(t.hi, t.lo, ((mpf(a) + mpf(c)) / 2 + h,
                                                    (mpf(a) + mpf(c)) / 2 - h)):
            assert abs(mpf(float(got_hi)) + mpf(float(got_lo)) - ref) <= mpf(2) ** -104   # a DD pair
    assert t.hi[0] >= t.hi[1]


def test_stats_truth_small():
    """Integers: mean 2, variance 5/2 exactly; a constant column takes the floor; one row too."""
    Y = np.array([[0.0, 7.0], [1.0, 7.0], [2.0, 7.0], [3.0, 7.0], [4.0, 7.0]])
    mu, sd, ys = P.stats(Y, 1e-6)
    assert list(mu.hi) == [2.0, 7.0] and sd.hi[1] == 1e-6
    assert abs(sd.hi[0] - np.sqrt(2.5)) <= EPS * 2 and np.all(ys.hi[:, 1] == 0.0)
    mu, sd, ys = P.stats(Y[:1], 1e-6)
    assert list(sd.hi) == [1e-6, 1e-6] and np.all(ys.hi == 0.0)


@pytest.mark.parametrize("case", P.SVD_CASES)
def test_noise_above_floor_and_caps(case):
    """Noise is finite and never below 4 eps of the scale; the vectors left out of the signed
    comparison stay under the caps: none in d2, d4 (both widths) and centred16 (its first n - 1),
    the 8 separated vectors plus one projector in cluster, at least 9 of 12 in d6, the 8 of the
    exact rank in deficient."""
    t = P.svd_truth(case)
    s0 = float(t.S.hi[0])
    for q, fl in (("S", 4 * EPS * s0), ("U", 4 * EPS), ("Vh", 4 * EPS), ("UtU", 4 * EPS),
                  ("VVt", 4 * EPS), ("resid", 4 * EPS * s0)):
        v = np.asarray(P.noise(q, case))
        assert np.all(np.isfinite(v)) and np.all(v >= fl), (q, case)
    ident, clusters = P.classify(case)
    regime, n, ny, p, k = P.case_params(case)
    want = {"d2": (p, 0), "d4": (p, 0), "centred16": (n - 1, 0), "cluster": (8, 1),
            "deficient": (P.RANK_DEFICIENT, 0)}
    if regime == "d6":
        assert len(ident) >= 9 and not clusters, (ident, clusters)
    else:
        assert (len(ident), len(clusters)) == want[regime], (case, ident, clusters)
    if regime == "cluster":
        assert clusters == [[2, 3, 4, 5]]
        assert P.noise("PU0", case) >= 4 * EPS and P.noise("PV0", case) >= 4 * EPS
    for q in ("S", "U", "Vh"):                          # no finding, no term
        if (q, case) not in P.FINDINGS:
            assert np.array_equal(P.limit(q, case), P.MARGIN * P.noise(q, case))


def test_deficient_hits_rank_deficiency_in_the_reference():
    """deficient is exactly rank 8 in fp64 (integer factors): numpy's restatement returns
    S[8:] below 1e-12 S_0, and the truth has exact zeros there."""
    X, om, p, k, q = P.case_inputs("deficient")
    assert np.linalg.matrix_rank(X) == P.RANK_DEFICIENT
    _, S, _ = gp_ref.randomized_svd(X, p, k=k, q=q, omega=om)
    assert np.all(S[P.RANK_DEFICIENT:] <= 1e-12 * S[0]) and S[P.RANK_DEFICIENT - 1] > 0.1 * S[0]
    t = P.svd_truth("deficient")
    assert np.all(t.S.hi[P.RANK_DEFICIENT:] <= 1e-30)
    Xc = P.case_inputs("centred16")[0]
    assert np.max(np.abs(Xc.mean(axis=0))) <= 4 * EPS and Xc.shape == (16, 300)


def test_build_arithmetic_is_right_on_a_benign_case():
    """The numpy restatement of svd.py's B B^T arithmetic agrees with the truth at d2 within 16x
    the noise; the closed form of its extra term is eps S_0^2 / S_i up to its constant, so above
    the reference's eps S_0 by the grading."""
    w = P._build_errors("d2")
    for q in ("S", "U", "Vh"):
        assert np.all(w[q] <= 16 * P.noise(q, "d2")), q
    S = P.svd_truth("d6").S.hi
    assert np.all(P.closed_form("S", "d6") >= EPS * S[0] ** 2 / S)
    assert np.all(np.isfinite(P.closed_form("Vh", "d6")))


def test_findings_carry_a_term_and_nothing_else_does():
    """At a finding the bound is above 16 x noise by the emulated term and below the closed
    form's; the emulation (numpy, svd.py's staged fallback) shows the same excess the device was
    measured at: the smallest singular value of d4 at r = 24 about 20 x the reference's noise."""
    assert P.FINDINGS == {("S", "d4k"), ("resid", "d4k")}
    for q, case in P.FINDINGS:
        nz, lim = np.asarray(P.noise(q, case)), np.asarray(P.limit(q, case))
        assert np.all(lim >= 16 * nz) and np.any(lim > 16 * nz)
        assert np.all(lim <= 16 * (nz + P.closed_form(q, case)))
    ratio = P._build_errors("d4k")["S"] / P.noise("S", "d4k")
    assert np.all(ratio[:10] <= 16) and 16 < ratio[11] < 64
    for case in P.SVD_CASES:
        for q in ("S", "U", "Vh", "resid"):
            if (q, case) not in P.FINDINGS:
                assert np.all(P.build_term(q, case) == 0)


@pytest.mark.parametrize("kind", ["graded", "cluster", "indefinite", "diagonal_tiny_live", "zero"])
def test_eig_noise_above_floor(kind):
    for r in (2, 25):
        ev, orth, res = P.eig_noise(kind, r)
        nrm = float(np.max(np.abs(P.eig_truth(kind, r).hi)))
        assert ev >= 4 * EPS * nrm and orth >= 4 * EPS * r and res >= 4 * EPS * r * nrm
        assert np.isfinite(ev) and ev <= 64 * EPS * max(nrm, 1.0) * r


def test_weights_truth_and_noise():
    """weights on an orthonormal-row K is y_std K^T; noise above its floor."""
    rng = np.random.default_rng(3)
    K = np.linalg.qr(rng.standard_normal((30, 4)))[0].T
    y = rng.standard_normal((6, 30))
    truth = P.weights(y, K)
    assert truth[0].err(y @ K.T) <= 64 * EPS and truth[1].err(np.ones(4)) <= 8 * EPS
    e_w, e_l = P.weights_noise(y, K, truth)
    assert np.all(e_w >= 4 * EPS * np.max(np.abs(truth[0].hi), axis=0)) and np.all(e_l >= 4 * EPS * truth[1].hi)
    Kt = P.basis(np.array([2.0, 1.0]), K[:2], 2, 4)
    assert Kt.err(np.diag([2.0, 1.0]) @ K[:2] / 2.0) <= 2 * EPS


@pytest.mark.parametrize("k", [-600, 600])
def test_stop_rule_needs_the_normaliser(k):
    """eig.hip's stop rule on a dense 4 x 4 matrix scaled by 2^+-600: on the bare squares it
    reads 0 <= 0 (or inf <= inf) and declares convergence at sweep 0; on entries normalised by a
    power of two from max|a| it does not, and it decides the unscaled matrix the same either way."""
    rng = np.random.default_rng(4)
    A = rng.standard_normal((4, 4))
    A = A + A.T
    c = 2.0 ** k
    assert not P.stop_rule_converged(A, normalise=False)
    assert not P.stop_rule_converged(A, normalise=True)
    if k < 0:
        assert P.stop_rule_converged(A * c, normalise=False)        # 0 <= 0
    else:
        with np.errstate(all="ignore"):
            B = (A * c) ** 2
            assert np.all(np.isinf(B)) and np.inf <= 1e-30 * np.inf  # what the kernel compared
    assert not P.stop_rule_converged(A * c, normalise=True)
    D = np.diag([3.0, -1.0, 0.5, 2.0]) * c
    assert P.stop_rule_converged(D, normalise=True)
