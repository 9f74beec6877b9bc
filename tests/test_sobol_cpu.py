"""CPU: the interval rules of gladsgp_amd.sensitivity pinned to scipy.stats.bootstrap itself, the
Saltelli design helpers, and the numpy restatement the GPU tests compare against
(tests/_sobol_ref.py) checked against the reference's own function (tests/golden/
sobol_ref_d3_m6.npz, written by tests/golden/make_sobol_golden.py).
"""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

import _sobol_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_ref_d3_m6.npz")


def _statistic(x, axis=-1):
    """Vector-valued: mean, standard deviation and a skew-sensitive ratio."""
    m = np.mean(x, axis=axis)
    s = np.std(x, axis=axis)
    return np.stack([m, s, np.mean(x ** 3, axis=axis) / (1.0 + s)])


def _data(kind, n):
    rng = np.random.default_rng(100 * n + kind)
    if kind == 0:
        return rng.standard_normal(n) + 2.0
    if kind == 1:
        return rng.gamma(2.0, 1.5, n)
    return rng.uniform(1.0, 3.0, n) ** 2


@pytest.mark.parametrize("n", [40, 64])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("as_torch", [False, True])
def test_bca_and_percentile_equal_scipy(n, kind, as_torch):
    from gladsgp_amd import sensitivity as sn
    x = _data(kind, n)
    theta = _statistic(x)
    jack = np.stack([_statistic(np.delete(x, i)) for i in range(n)])       # (n, 3)
    for level in (0.95, 0.8):
        res = stats.bootstrap([x], _statistic, n_resamples=999, method="BCa",
                              confidence_level=level, random_state=np.random.default_rng(5),
                              vectorized=True)
        boot = np.moveaxis(res.bootstrap_distribution, -1, 0)              # (R, 3)
        args = (theta, boot, jack)
        if as_torch:
            args = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in args)
        ci = sn.bca_interval(*args, confidence_level=level)
        np.testing.assert_allclose(np.asarray(ci.low), res.confidence_interval.low, rtol=1e-12)
        np.testing.assert_allclose(np.asarray(ci.high), res.confidence_interval.high, rtol=1e-12)
        resp = stats.bootstrap([x], _statistic, n_resamples=999, method="percentile",
                               confidence_level=level, random_state=np.random.default_rng(5),
                               vectorized=True)
        bootp = np.moveaxis(resp.bootstrap_distribution, -1, 0)
        cip = sn.percentile_interval(torch.from_numpy(np.ascontiguousarray(bootp)) if as_torch
                                     else bootp, confidence_level=level)
        np.testing.assert_allclose(np.asarray(cip.low), resp.confidence_interval.low, rtol=1e-12)
        np.testing.assert_allclose(np.asarray(cip.high), resp.confidence_interval.high,
                                   rtol=1e-12)


def test_bca_degenerate_distribution_is_nan():
    from gladsgp_amd import sensitivity as sn
    boot = np.ones((50, 2))
    boot[:, 1] = np.linspace(0.0, 1.0, 50)
    jack = np.ones((10, 2))
    jack[:, 1] = np.linspace(0.4, 0.6, 10)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for conv in (np.asarray, torch.from_numpy):
            ci = sn.bca_interval(conv(np.array([1.0, 0.5])), conv(boot), conv(jack), 0.95)
            lo, hi = np.asarray(ci.low), np.asarray(ci.high)
            assert np.isnan(lo[0]) and np.isnan(hi[0])            # no spread: a = 0 / 0
            assert np.isfinite(lo[1]) and np.isfinite(hi[1]) and lo[1] < hi[1]


def test_saltelli_design_and_points():
    from gladsgp_amd import sensitivity as sn
    d, m = 4, 5
    A, B = sn.saltelli_design(d, m, seed=3)
    assert A.shape == B.shape == (2 ** m, d)
    AB = stats.qmc.Sobol(d=2 * d, seed=3).random_base2(m)
    np.testing.assert_array_equal(A, AB[:, d:])                   # A: the last n_dim columns
    np.testing.assert_array_equal(B, AB[:, :d])
    A2, B2 = sn.saltelli_design(d, m, seed=3)
    np.testing.assert_array_equal(A, A2)
    np.testing.assert_array_equal(B, B2)
    assert not np.array_equal(A, sn.saltelli_design(d, m, seed=4)[0])
    pts = sn.saltelli_points(A, B)
    N = 2 ** m
    assert pts.shape == ((d + 2) * N, d)
    np.testing.assert_array_equal(pts[:N], A)
    np.testing.assert_array_equal(pts[N:2 * N], B)
    for i in range(d):
        ABi = pts[(2 + i) * N:(3 + i) * N]
        other = [c for c in range(d) if c != i]
        np.testing.assert_array_equal(ABi[:, other], B[:, other])
        np.testing.assert_array_equal(ABi[:, i], A[:, i])
        assert not np.array_equal(ABi[:, i], B[:, i])
    with pytest.raises(ValueError):
        sn.saltelli_points(A, B[:, :3])


def test_restatement_matches_reference_golden():
    g = np.load(GOLDEN)
    fA, fB, fAB = ref.to_output_major(g["fA"], g["fB"], g["fAB"])
    N = fA.shape[1]
    assert N == 64 and g["A"].shape == (64, 3) and fAB.shape == (3, 3, 64)
    # the recorded design is a Saltelli stack: AB_i is B with column i from A
    out = ref.replicates(fA, fB, fAB, np.arange(N)[None], pcvar=g["pcvar"], clamp=False)
    for mine, bound, theirs in (("first", "b_first", "first_order"),
                                ("total", "b_total", "total_index"),
                                ("gfirst", "b_gfirst", "gen_first_order"),
                                ("gtotal", "b_gtotal", "gen_total_index")):
        err = np.abs(out[mine][0] - g[theirs])
        assert (err <= out[bound][0]).all(), (mine, err.max(), out[bound][0].min())


def test_restatement_rows():
    """The row rules of the header: jackknife replicate r leaves row r out; Philox rows are in
    range, differ by replicate and offset, and depend on (seed, offset, r, k) alone."""
    jk = ref.jackknife_rows(7)
    assert jk.shape == (7, 6)
    for r in range(7):
        assert sorted(set(range(7)) - set(jk[r])) == [r]
    rows = ref.philox_rows(100, 37, 5, seed=9, offset=3)
    assert rows.shape == (5, 37) and rows.min() >= 0 and rows.max() < 100
    np.testing.assert_array_equal(rows[:3, :20], ref.philox_rows(100, 20, 3, seed=9, offset=3))
    assert not np.array_equal(rows, ref.philox_rows(100, 37, 5, seed=9, offset=4))
    assert not np.array_equal(rows[0], rows[1])


def test_restatement_clamp_and_general():
    rng = np.random.default_rng(0)
    p, N, d = 3, 20, 2
    fA, fB = rng.standard_normal((p, N)), rng.standard_normal((p, N))
    fAB = rng.standard_normal((d, p, N))                 # unrelated outputs: V of either sign
    rows = rng.integers(0, N, (6, N))
    w = np.array([0.5, 0.3, 0.2])
    raw = ref.replicates(fA, fB, fAB, rows, pcvar=w, clamp=False)
    cl = ref.replicates(fA, fB, fAB, rows, pcvar=w, clamp=True)
    assert (raw["first"] < 0).any()
    np.testing.assert_array_equal(cl["first"], np.maximum(raw["first"], 0.0))
    np.testing.assert_array_equal(cl["total"], raw["total"])
    np.testing.assert_allclose(cl["gfirst"], np.einsum("j,rji->ri", w, cl["first"]), rtol=1e-14)
    # one replicate by hand
    r = 2
    a, b, c = fA[1, rows[r]], fB[1, rows[r]], fAB[0, 1, rows[r]]
    var = np.var(np.concatenate([a, b]))
    np.testing.assert_allclose(raw["first"][r, 1, 0], np.mean(a * (c - b)) / var, rtol=1e-13)
    np.testing.assert_allclose(raw["total"][r, 1, 0], 0.5 * np.mean((b - c) ** 2) / var,
                               rtol=1e-13)
