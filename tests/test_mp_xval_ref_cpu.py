"""The 50-digit reference of gp_xval itself (tests/_mp_xval_ref.py): the chain truth against a
brute-force refit carried at the same precision and against ``_mp_ref.truth`` on the reduced
design, the whole-design folds against the prior, the truth against the numpy closed form, the
kernel truth against the chain truth, the three conditions the device tests rely on (nothing
skipped, every Q_FF factors in every fp64 restatement, the scalings keep every intermediate
normal), the noise finite and above its floor, the findings' term under its closed form, and the
reason xq is held on its own scale.  No GPU.

CPU time: 113 s wall alone (154 tests, measured 2026-10-21), most of it the 65-digit
factorisations, the per-plan truths and the brute-force refits; the per-(regime, n, plan) truths
and noise levels are the ones tests/test_gpu_xval_extremes.py needs.
"""
import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import gp_ref

import _mp_ref as M
import _mp_xval_ref as X
import _xval_ref

BRUTE = [(r, 5) for r in M.REGIMES] + [(r, n) for r in ("mid", "grid") for n in (64, 65)]


def test_plans_are_what_the_design_says():
    """Sizes, coverage and the edges each plan is there for."""
    assert X.SIZES == (1, 5, 64, 65, 130)
    sizes = {n: {k: (None if f is None else sorted(len(F) for F in f))
                 for k, f in X.plans(n).items()} for n in X.SIZES}
    assert sizes[1] == {"loo": None, "one": [1]}
    assert sizes[5] == {"loo": None, "pair_triple": [2, 3], "whole": [5]}
    assert X.plans(5)["whole"] == [[4, 0, 2, 1, 3]]
    assert sizes[64] == {"loo": None, "whole": [64], "tiles": [1] * 14 + [2, 15, 16, 17]}
    assert sizes[65] == {"loo": None, "tail64": [64], "head64": [64], "split": [32, 33]}
    assert sizes[130] == {"loo": None, "big": [1, 2, 63, 64], "mid": [33, 48, 49],
                          "thirds": [43, 43, 44], "late": [1, 2, 15, 16, 17],
                          "late_pair": [2, 15, 16, 17]}
    for n in X.SIZES:
        for name, f in X.plans(n).items():
            if f is None:
                continue
            flat = [i for F in f for i in F]
            assert len(set(flat)) == len(flat) and min(flat) >= 0 and max(flat) < n, (n, name)
            assert all(len(F) <= 64 for F in f)
            if name in ("whole", "tiles", "split", "big", "mid", "thirds"):
                assert sorted(flat) == list(range(n)), (n, name)     # every index covered
    p = X.plans(130)
    assert sorted(min(F) for F in p["late"] if len(F) > 2) == [64, 80, 112]
    assert sorted(min(F) for F in p["late_pair"] if len(F) > 2)[:2] == [64, 79]
    assert min(min(F) for F in p["late_pair"] if len(F) == 15) >= 112
    assert [127, 129] in p["late"] and [128, 129] in p["late_pair"]
    assert any(F != sorted(F) for F in p["big"]) and any(F == sorted(F) for F in p["big"])
    assert any(64 in F for F in X.plans(65)["split"])
    assert X.plans(130) is X.plans(130)                               # deterministic, shared


def test_factor_rounds_to_the_chain_truth_of_mp_ref():
    """The L^-1 the xval truth starts from is ``truth_of``'s: equal after rounding to fp64."""
    for regime, n in (("mid", 5), ("grid", 65), ("sharp", 64)):
        C, z, _ = X.factor_mp(regime, n)
        t = M.truth_of(regime, n)
        got = np.array([[float(C[j][i]) for j in range(n)] for i in range(n)])
        np.testing.assert_array_equal(got, t.Linv.hi)
        np.testing.assert_array_equal(np.array([float(v) for v in z]), t.z.hi)


def _loo_sample(n):
    return sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1} & set(range(n)))


@pytest.mark.parametrize("regime,n", BRUTE)
def test_chain_truth_equals_a_brute_force_refit(regime, n):
    """Every fold of every plan refitted at the truth's own precision: |difference| <= 1e-45 on
    the mpf values (of O(1) quantities: absolute).  Then ``_mp_ref.truth`` on the design without
    F, whose results are double-double pairs: the two pairs agree to 2^-100 of the quantity's
    scale.  At n = 64 and 65 leave-one-out refits a sample of six singletons (both ends and both
    sides of the middle; all 64 cost 14 s per regime), every other plan all its folds."""
    p = M.problem(regime, n)
    for plan, folds in X.plans(n).items():
        t = X.chain_truth(regime, n, plan)
        sample = folds is None and n > 5
        bm, bv = X.refit_mp(regime, n, [[i] for i in _loo_sample(n)] if sample else folds)
        with mp.workdps(M.DPS + X.GUARD_DIGITS):
            at = {int(i): k for k, i in enumerate(t.idx)}
            for i in bm:
                assert abs(t.mp["xmean"][at[i]] - bm[i]) <= mpf(10) ** -45, (plan, i)
                assert abs(t.mp["xvar"][at[i]] - bv[i]) <= mpf(10) ** -45, (plan, i)
        ld = np.longdouble
        for F in X.listed(folds, n):
            if len(F) == n or (len(F) == 1 and n > 5 and F[0] not in _loo_sample(n)):
                continue
            dm, dv = X.refit_dd(regime, n, F)
            k = [at[i] for i in F]
            for mine, theirs, scale in ((t.xmean, dm, float(np.max(np.abs(p.w)))),
                                        (t.xvar, dv, p.s_pred)):
                gap = (mine.hi[k].astype(ld) - theirs.hi.astype(ld)) + \
                      (mine.lo[k].astype(ld) - theirs.lo.astype(ld))
                assert np.max(np.abs(gap)) <= 2.0 ** -100 * scale, (plan, F[:3])


@pytest.mark.parametrize("regime", M.REGIMES)
def test_whole_design_folds_give_the_prior(regime):
    """The fold that is the whole design (n = 1, 5 and 64): mean 0 and xvar = s_pred at 50
    digits, through the heaviest cancellation the closed form has."""
    for n, plan in ((1, "loo"), (1, "one"), (5, "whole"), (64, "whole")):
        p, t = M.problem(regime, n), X.chain_truth(regime, n, plan)
        with mp.workdps(M.DPS + X.GUARD_DIGITS):
            wmax = mpf(float(np.max(np.abs(p.w))))
            assert max(abs(v) for v in t.mp["xmean"]) <= mpf(10) ** -50 * wmax, (n, plan)
            assert max(abs(v - mpf(p.s_pred)) for v in t.mp["xvar"]) <= \
                mpf(10) ** -50 * mpf(p.s_pred), (n, plan)


@pytest.mark.parametrize("n", M.SIZES)
def test_chain_truth_against_the_closed_form_mid(n):
    """tests/_xval_ref.closed_form on the oracle's Gram is one member of the ensemble, so it
    sits within the noise of the truth."""
    p = M.problem("mid", n)
    A = gp_ref.gram_ardse(p.X, p.beta, p.s, p.delta)
    for plan, folds in X.plans(n).items():
        t = X.chain_truth("mid", n, plan)
        mean, xq = _xval_ref.closed_form(A, p.w, folds, 0.0)
        assert np.array_equal(np.flatnonzero(~np.isnan(mean)), t.idx)
        for q, x in (("xmean", mean), ("xq", xq), ("xvar", xq - X.shift_of(p))):
            assert t.err(q, x) <= X.chain_noise(q, "mid", n, plan), (plan, q)


@pytest.mark.parametrize("regime,n,plan", X.REGIME_CASES)
def test_noise_conditions_and_layers(regime, n, plan):
    """Per case: every Q_FF factors in every fp64 restatement of both layers; every noise is
    finite and at or above its floor; the kernel truth on Linv.hi stays within the chain noise
    of the chain truth; the device test's scalings keep every intermediate normal with the
    guard of ``_mp_xval_ref.GUARD``; a finding's term stays under its closed form."""
    p = M.problem(regime, n)
    folds = X.folds_of(n, plan)
    nfolds = len(X.listed(folds, n))
    assert X.every_q_factors(regime, n, plan) == (2 * len(M.permutations(n)) + 3) * nfolds
    ct, kt = X.chain_truth(regime, n, plan), X.kernel_truth_hi(regime, n, plan)
    kn = X.kernel_noise_hi(regime, n, plan)
    for q in X.QUANTITIES:
        for nz, t in ((X.chain_noise(q, regime, n, plan), ct), (kn[q], kt)):
            assert np.isfinite(nz) and nz >= X.floor_of(q, t, p) > 0.0, (q, nz)
        gap = ct.err(q, kt.full(q))
        assert gap <= X.chain_noise(q, regime, n, plan), (q, gap)
        term = X.explicit_inverse_term(q, regime, n, plan)
        if (q, regime, n, plan) in X.FINDINGS:
            assert regime == "grid" and n >= 64
            assert 0.0 <= term <= (M.block_condition(regime, n) - 1.0) * \
                X.chain_noise(q, regime, n, plan)
        else:
            assert term == 0.0
    for shift in (X.shift_of(p), None):
        mags = X.magnitudes(M.truth_of(regime, n).Linv.hi, p.w, folds, shift)
        assert X.largest_k(mags, "w", X.K_W) == X.K_W, (regime, n, plan)
        assert X.largest_k(mags, "Linv", X.K_LINV) == X.K_LINV, (regime, n, plan)


def test_no_case_is_left_out():
    """The device file's parameter list is every (regime, n, plan); none carries a mark."""
    assert len(X.REGIME_CASES) == len(M.REGIMES) * sum(len(X.plans(n)) for n in M.SIZES) == 126
    assert {c[0] for c in X.REGIME_CASES} == set(M.REGIMES)
    assert all(M.group_of(r) in M.GROUPS for r in M.REGIMES)


def test_findings_are_confined():
    for q, regime, n, plan in X.FINDINGS:
        assert q in X.QUANTITIES and regime == "grid" and n >= 64 and plan in X.plans(n)


def test_xq_hides_under_the_shift_on_the_grid():
    """Why xq is a quantity of its own: on the 1-D grid at n = 65 the leave-one-out variance
    before the shift is below 1e-6 s_pred while the reported one is the shift's size, so a
    relative error of xq far above fp64's passes any bound scaled by s_pred."""
    p, t = M.problem("grid", 65), X.chain_truth("grid", 65, "loo")
    assert 0.0 < t.xq.scale() < 1e-6 * p.s_pred
    assert np.min(t.xvar.hi) > 0.5 * 0.01
    assert 1e-7 * t.xq.scale() < 1e-4 * 1e-9 * p.s      # seven lost digits of xq: 1e-4 of the
    #                                                     oracle-parity bound on the variance
    assert X.chain_noise("xq", "grid", 65, "loo") < 1e-7 * t.xq.scale()    # and xq sees them
