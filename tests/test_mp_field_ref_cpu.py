"""CPU: the 50-digit field reference (tests/_mp_field_ref.py) checked against itself -- exact
rational arithmetic on a 3 x 4 x 5 case, the double-double round trip, the float32 rounding, the
fp64 position rule against numpy's own selection, the zero-cap condition on the score's Y, the
cancel regime's condition number, the noise floors and the +-300 scalings.  No GPU.
"""
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

import _mp_field_ref as F
from _mp_ref import DD, EPS, MARGIN


def _fr(a):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _close(dd: DD, exact, rel=1e-30):
    """hi is the exact value rounded to fp64 and hi + lo the exact value to ~2^-105."""
    exact = np.array(exact, dtype=object).reshape(dd.hi.shape)
    for h, l, x in zip(dd.hi.reshape(-1), dd.lo.reshape(-1), exact.reshape(-1)):
        assert h == float(x), (h, float(x))
        assert abs(Fraction(float(h)) + Fraction(float(l)) - x) <= rel * abs(x) + Fraction(1, 2 ** 1070)


def test_truth_against_fractions():
    """field, summary, score and gp_pca_trunc truths on S = 3 samples x P = 4 PCs x 5 columns
    against fractions.Fraction (exact)."""
    rng = np.random.default_rng(3)
    S, P, n = 3, 4, 5
    W, K = rng.standard_normal((S, P)), rng.standard_normal((P, n)) * 10.0 ** -np.arange(P)[:, None]
    sd, mu, err = rng.uniform(0.5, 2, n), rng.standard_normal(n) * 1e3, rng.standard_normal(S)
    Wf, Kf = _fr(W), _fr(K)
    sdf, muf, ef = _fr([sd])[0], _fr([mu])[0], _fr([err])[0]
    a = [[sum(Wf[r][k] * Kf[k][c] for k in range(P)) for c in range(n)] for r in range(S)]
    y = [[a[r][c] * sdf[c] + muf[c] for c in range(n)] for r in range(S)]
    z = [[(a[r][c] + ef[r]) * sdf[c] + muf[c] for c in range(n)] for r in range(S)]
    ft = F.field_truth(W, K, sd, mu, err)
    _close(ft.y, y)
    _close(ft.z, z)
    _close(F.field_truth(W, K).y, a)
    q = (1 / 3, 0.999)
    st = F.summary_truth(ft, S, 1, q)
    _close(st.mean, [[sum(y[r][c] for r in range(S)) / S for c in range(n)]])
    for qq, got in zip(q, (st.lo, st.hi)):
        j, t = F.position(qq, S)
        want = []
        for c in range(n):
            col = sorted(z[r][c] for r in range(S))
            want.append(col[j] + (col[j + 1] - col[j]) * Fraction(t) if j < S - 1 else col[S - 1])
        _close(got, [want])
    # the score's sums on the fp64-stored maps
    Y = np.array([[y[1][c] for c in range(n)]], dtype=np.float64) + 0.25
    Y[0, 1] = np.nan
    rows, cols, _, _ = F.score_truth(st, False, Y, 0.5)
    mean64 = [Fraction(float(v)) for v in st.mean.hi[0]]
    ok = [c for c in range(n) if c != 1]
    _close(rows.take((slice(None), 0)), [[sum((mean64[c] - Fraction(float(Y[0, c]))) ** 2 for c in ok)]][0])
    assert rows.hi[0, 1] == 4 and list(cols.hi[:, 1]) == [1, 0, 1, 1, 1]
    assert rows.hi[0, 3] == sum(1 for c in ok if not Y[0, c] < 0.5)
    _close(cols.take((slice(None), 3)),
           [Fraction(float(st.hi.hi[0, c])) - Fraction(float(st.lo.hi[0, c])) for c in range(n)])
    # gp_pca_trunc: Y (3 x 5), C = W (3 x 4), V = K, ranks 0, 1, 3, 4
    Yt = rng.standard_normal((S, n))
    ranks = [0, 1, 3, 4]
    tt = F.trunc_truth(Yt, W, K, ranks, mu, sd)
    Yf = _fr(Yt)
    tot, node, var = [], [], []
    for p in ranks:
        e = [[(Yf[i][j] - muf[j]) - sdf[j] * sum(Wf[i][k] * Kf[k][j] for k in range(p))
              for j in range(n)] for i in range(S)]
        s2, s1 = sum(v * v for r in e for v in r), sum(v for r in e for v in r)
        tot.append([s2, s1])
        node.append([sum(e[i][j] ** 2 for i in range(S)) for j in range(n)])
        var.append(s2 / 15 - (s1 / 15) ** 2)
    _close(tt.tot, tot)
    _close(tt.node, node)
    _close(tt.var, var)
    with mp.workdps(60):
        for r in range(len(ranks)):
            rm = mp.sqrt(mpf(tot[r][0].numerator) / tot[r][0].denominator / 15)
            assert abs(mpf(float(tt.rmse.hi[r])) + mpf(float(tt.rmse.lo[r])) - rm) <= rm * mpf(10) ** -30


def test_dd_round_trip():
    with mp.workdps(F.DPS):
        vals = [mp.pi * mpf(10) ** k for k in (-280, -40, 0, 40, 300)] + [mpf(0), -mp.e, mpf(1) / 3]
        dd = DD(vals)
        for v, h, l in zip(vals, dd.hi, dd.lo):
            assert h == float(v)
            assert abs(mpf(float(h)) + mpf(float(l)) - v) <= abs(v) * mpf(2) ** -104
        assert dd.err(dd.hi) <= 2.0 ** -53 * dd.scale()
        assert dd.take(slice(1, 3)).hi.shape == (2,)


def test_round_f32():
    """One rounding to float32: numpy's cast of every fp64 probe (exact inputs), the ties, the
    overflow threshold FLT_MAX + half an ulp, the subnormal grid; and a value whose fp64 rounding
    would round differently (double rounding is not what the truth does)."""
    rng = np.random.default_rng(0)
    probes = np.concatenate([
        rng.standard_normal(200) * 10.0 ** rng.uniform(-46, 39, 200),
        [0.0, F.FLT_MAX, -F.FLT_MAX, 2.0 ** 128, 2.0 ** 128 - 2.0 ** 103, 2.0 ** 128 - 2.0 ** 102,
         np.nextafter(2.0 ** 128 - 2.0 ** 103, 0.0), 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150,
         np.nextafter(2.0 ** -150, 1.0), 2.0 ** -126, 2.0 ** -126 - 2.0 ** -150, 1 + 2.0 ** -24,
         1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52, -1e-46, 1e39]])
    with np.errstate(over="ignore", under="ignore"):
        want = probes.astype(np.float32).astype(np.float64)
    with mp.workdps(F.DPS):
        got = np.array([F.round_f32(mpf(float(v))) for v in probes])
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got[got != 0]),
                                                            np.signbit(want[want != 0]))
        # 1 + 2^-24 + 2^-60 is above the tie: float32 1 + 2^-23, though fp64 rounds it to the tie
        v = mpf(1) + mpf(2) ** -24 + mpf(2) ** -60
        assert float(v) == 1 + 2.0 ** -24 and F.round_f32(v) == 1 + 2.0 ** -23
        assert F.round_f32(mpf(2) ** 128 - mpf(2) ** 103 - mpf(2) ** -10) == F.FLT_MAX
        assert F.round_f32(-(mpf(2) ** 128 - mpf(2) ** 103)) == -np.inf
    assert np.array_equal(F.ulp_f32(np.array([1.0, 1.5, 2.0, 2.0 ** -126, 2.0 ** -140, 3e38])),
                          [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149, 2.0 ** 104])


QS = (0.0, 0.025, 0.1, 0.12, 0.88, 0.9, 0.975, 1.0, 1.0 - 0.025, 1.0 - 0.1, 1 / 3, 0.999, 0.5, 0.25,
      0.05, 0.95, 2 / 3, 1e-3)


def test_position_rule_is_numpys():
    """(j, t) of ``position`` against numpy's own selection for S = 1 ... 400 and every q in
    use: on the data k - j (k = 0 ... S - 1) np.quantile returns (j' - j) + t' with both
    interpolation forms exact, so it equals t bit for bit exactly when numpy's (j', t') is
    (j, t).  Exact agreement on every case."""
    cases = 0
    for S in range(1, 401):
        base = np.arange(S, dtype=np.float64)
        for q in QS:
            j, t = F.position(q, S)
            assert 0 <= j <= S - 1 and 0.0 <= t < 1.0
            if j == S - 1:
                assert t == 0.0
            got = float(np.quantile(base - j, q))
            assert got == t and not np.signbit(got), (S, q, j, t, got)
            cases += 1
    assert cases == 400 * len(QS)
    # the depths the summary cases rely on, and the two refusals
    assert {F.list_depth(c[1], c[5]) for c in F.SUMMARY_CASES} == {2, 4, 8}
    assert max(F.tail_depths(64, 0.1)) == 8
    assert F.tail_depths(64, (0.12, 1.0))[0] == 9 and F.tail_depths(64, (0.0, 0.88))[1] == 9


def test_cases_cover_the_edges():
    assert {c[0] for c in F.FIELD_CASES} == set(F.FIELD_REGIMES)
    assert {c[2] for c in F.FIELD_CASES} == {1, 5, 12, 25, 40, 64}
    assert {c[1] for c in F.FIELD_CASES} == {1, 37} and {c[3] for c in F.FIELD_CASES} == {1, 130}
    s = F.SUMMARY_CASES
    assert {c[0] for c in s} == set(F.FIELD_REGIMES)
    assert {c[1] for c in s} == {1, 2, 17, 33, 64} and {c[2] for c in s} == {8, 40}
    assert {c[3] for c in s} == {1, 3} and {c[4] for c in s} == {31, 130}
    assert {c[5] for c in s} == {0, 0.025, 0.1, (0, 1)}
    t = F.TRUNC_CASES
    assert {c[0] for c in t} == set(F.TRUNC_REGIMES)
    assert {c[1] for c in t} == {1, 16, 17, 33} and {c[2] for c in t} == {1, 65, 130}
    assert {c[5] for c in t} == {True, False} and {c[6] for c in t} == {True, False}
    assert any(len(c[4]) == 32 and c[4][-1] == 128 and c[1] == 33 for c in t)
    assert {F.SUMMARY_CASES[c[0]][0] for c in F.SCORE_CASES} == set(F.FIELD_REGIMES)


def test_ties_hold_exact_duplicates():
    """The ties regime: equal samples give equal truths, duplicates sit at selected positions in
    many columns, and the zero rows carry both signs."""
    for case in F.SUMMARY_CASES:
        if case[0] != "ties":
            continue
        regime, S, P, m, ncols, q, sdmu, err = case
        W3, K, sd, mu, e = F.summary_operands(regime, S, m, P, ncols, q)
        sizes = [g for _, g in F.tie_groups(S, F.list_depth(S, q))]
        assert sizes[:4] == [1, 2, 3, F.list_depth(S, q) + 1][: len(sizes[:4])] or S < 4
        _, st = F.summary_case_truth(case)
        if S >= 17:
            assert np.count_nonzero(st.tied_lo) >= 5 and np.count_nonzero(st.tied_hi) >= 5
            assert np.any(np.signbit(W3[W3 == 0])) and not np.all(np.signbit(W3[W3 == 0]))


def test_cancel_reaches_its_condition():
    """sum_k |w_k K_k| / |a| per (row, column): the median within a factor 10 of 1e10, no
    element below 1e8."""
    for case in F.FIELD_CASES:
        if case[0] != "cancel":
            continue
        W, K, _, _, _ = F.field_operands(*case)
        a = np.abs(F.field_case_truth(*case, False, False).y.hi)
        cond = (np.abs(W) @ np.abs(K)) / a
        assert 0.1 * F.CANCEL <= np.median(cond) <= 10 * F.CANCEL, (case, np.median(cond))
        assert cond.min() >= 1e-2 * F.CANCEL, (case, cond.min())


def test_noise_floors_hold():
    for case in (("mid", 37, 5, 130), ("cancel", 37, 40, 130), ("f32edge", 37, 12, 130)):
        for sdmu, err in F.COMBOS:
            t = F.field_case_truth(*case, sdmu, err)
            ny, nz = F.field_noise(*case, sdmu, err)
            assert np.all(ny >= 4 * EPS * np.max(np.abs(t.y.hi), axis=0))
            assert np.all(nz >= 4 * EPS * np.max(np.abs(t.z.hi), axis=0))
            # the ensemble is within a few hundred eps of the columns' sum |w K| sd + |mu|
            assert np.all(np.isfinite(nz))
    case = F.SUMMARY_CASES[8]
    ft, st = F.summary_case_truth(case)
    nz = F.summary_noise(case)
    zmax = np.max(np.abs(ft.z.hi), axis=0)
    assert np.all(nz["lo"] >= 6.99 * EPS * zmax) and np.all(nz["mean"] >= 4 * EPS * np.abs(st.mean.hi))
    for case in (F.TRUNC_CASES[4], F.TRUNC_CASES[13]):
        _, t, nz = F.trunc_case(case)
        assert np.all(nz["sse"] >= 4 * EPS * t.tot.hi[:, 0]) and np.all(nz["sum"] >= 4 * EPS * t.abs1)
        assert np.all(nz["var"] >= 4 * EPS * np.abs(t.var.hi))
        assert np.all(nz["node"] >= 4 * EPS * t.node.hi) and np.all(nz["rmse"] >= 4 * EPS * t.rmse.hi)


def test_biased_var_cancels():
    """biased: (mean e)^2 / var is about BIAS^2 at the deep ranks, and the derived one-pass term is
    that many units in the last place of var; it is 0 outside FINDINGS."""
    case = F.TRUNC_CASES[11]
    _, t, nz = F.trunc_case(case)
    ratio = t.B[-1] ** 2 / t.var.hi[-1]
    assert 0.1 * F.BIAS ** 2 <= ratio <= 10 * F.BIAS ** 2, ratio
    term = F.one_pass_var_term(t, nz)
    assert np.all(term >= F.U * (t.A + 3 * t.B ** 2))
    assert np.all(F.trunc_limit("var", case) == MARGIN * (nz["var"] + term))
    mid = F.TRUNC_CASES[1]
    assert np.all(F.trunc_limit("var", mid) == MARGIN * F.trunc_case(mid)[2]["var"])


@pytest.mark.parametrize("scase", F.SCORE_CASES, ids=lambda s: f"{F.SUMMARY_CASES[s[0]][0]}-{s[0]}")
def test_score_Y_is_decided(scase):
    """Zero cap: no element of the score's Y within MARGIN x noise of a band edge or of the
    floor, so every count of the truth is the count of any correct evaluation."""
    Y, rows, cols, e_r, e_c, undecided = F.score_case(scase)
    assert undecided == 0
    y = np.asarray(Y)
    assert np.isnan(y).any() and not np.isinf(y).any() and not np.any(y == 0)
    R = F._score_ref.ROW
    assert 0 < rows.hi[:, R["covered"]].sum() < rows.hi[:, R["valid"]].sum() or scase[1]
    if scase[4]:
        assert np.any(np.abs(y) == 1e-300)
    assert np.all(np.isfinite(rows.hi)) and np.all(np.isfinite(cols.hi))


def test_scalings_stay_normal():
    """a = +-300: W 2^a, K 2^-a, (sd, mu) 2^a and the outputs 2^a for the field; Y, mu, sd 2^a,
    C 2^a, V 2^-a, tot 2^a / 2^2a and node 2^2a for gp_pca_trunc -- every non-zero value stays
    in the normal range."""
    for a in (-300, 300):
        for case in F.SCALED_FIELD_CASES:
            W, K, sd, mu, err = F.field_operands(*case)
            t = F.field_case_truth(*case, True, True)
            assert F.all_normal(np.ldexp(W, a), np.ldexp(K, -a), np.ldexp(sd, a), np.ldexp(mu, a),
                                np.ldexp(t.z.hi, a), np.ldexp(t.y.hi, a))
            assert F.all_normal(np.ldexp(F.field_case_truth(*case, False, False).y.hi, a))
        for idx in F.SCALED_SCORE_CASES:
            regime, S, P, m, ncols, q, sdmu, err = F.SUMMARY_CASES[idx]
            _, _, sd, mu, _ = F.summary_operands(regime, S, m, P, ncols, q)
            Y = np.asarray(F.score_Y(idx, False, False, False))
            _, rows, cols, _, _, undecided = F.score_case((idx, False, False, 0.5, False))
            assert sdmu and undecided == 0
            assert F.all_normal(np.ldexp(sd, a), np.ldexp(mu, a), np.ldexp(Y[~np.isnan(Y)], a),
                                np.ldexp(rows.hi, 2 * a), np.ldexp(cols.hi, 2 * a),
                                np.ldexp(rows.hi, a), np.ldexp(cols.hi, a))
        for case in F.SCALED_TRUNC_CASES:
            (Y, C, V, mu, sd), t, _ = F.trunc_case(case)
            assert Y.dtype == np.float64
            ops = [np.ldexp(Y, a), np.ldexp(C, a), np.ldexp(V, -a)]
            ops += [np.ldexp(mu, a), np.ldexp(sd, a)] if mu is not None else []
            assert F.all_normal(*ops, np.ldexp(t.tot.hi[:, 0], 2 * a), np.ldexp(t.tot.hi[:, 1], a),
                                np.ldexp(t.node.hi, 2 * a))
    assert not F.all_normal(np.array([1e-310])) and not F.all_normal(np.array([np.inf]))
    assert F.all_normal(np.array([0.0, -0.0, 2.0 ** -1022, -1.7e308]))
