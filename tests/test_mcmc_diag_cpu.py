"""CPU: mcmc.rhat / mcmc.ess against a plain-loop restatement of their docstring formulas
(direct O(N^2) autocovariance, no FFT, no array arithmetic across chains or elements), and three
inputs whose outcome is certain."""
import math

import numpy as np
import pytest

from gladsgp_amd import mcmc


def _ar1(rng, C, N, K, phi=0.6):
    """C chains of K AR(1) series: autocorrelated, so the Geyer cut falls inside the series."""
    x = np.empty((C, N, K))
    x[:, 0] = rng.standard_normal((C, K))
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + math.sqrt(1 - phi * phi) * rng.standard_normal((C, K))
    return x


def _mean(v):
    s = 0.0
    for a in v:
        s += a
    return s / len(v)


def _var1(v):
    m = _mean(v)
    s = 0.0
    for a in v:
        s += (a - m) ** 2
    return s / (len(v) - 1)


def rhat_loops(x):
    """The docstring of mcmc.rhat for one element: x is a list of C lists of N' draws."""
    h = len(x[0]) // 2
    seq = [c[:h] for c in x] + [c[len(c) - h:] for c in x]
    m = len(seq)
    means = [_mean(s) for s in seq]
    grand = _mean(means)
    B = h / (m - 1) * sum((a - grand) ** 2 for a in means)
    W = _mean([_var1(s) for s in seq])
    return math.sqrt(((h - 1) / h * W + B / h) / W)


def ess_loops(x):
    """The docstring of mcmc.ess for one element, the autocovariance as the direct double sum."""
    C, N = len(x), len(x[0])
    means = [_mean(c) for c in x]

    def acov(c, t):
        s = 0.0
        for i in range(N - t):
            s += (x[c][i] - means[c]) * (x[c][i + t] - means[c])
        return s / N

    W = N / (N - 1) * _mean([acov(c, 0) for c in range(C)])
    varp = (N - 1) / N * W + (_var1(means) if C > 1 else 0.0)
    rho = [1.0] + [1.0 - (W - _mean([acov(c, t) for c in range(C)])) / varp
                   for t in range(1, N)]
    tau = -1.0
    for k in range(N // 2):
        pk = rho[2 * k] + rho[2 * k + 1]
        if k >= 1 and pk <= 0:
            break
        tau += 2.0 * pk
    return C * N / tau


@pytest.mark.parametrize("N", [16, 101])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_rhat_and_ess_match_the_plain_loops(C, N):
    K, nburn = 3, 2
    x = _ar1(np.random.default_rng([C, N]), C, N + nburn, K)
    got_r, got_e = mcmc.rhat(x, nburn), mcmc.ess(x, nburn)
    assert got_r.shape == got_e.shape == (K,)
    for e in range(K):
        cols = [[float(v) for v in x[c, nburn:, e]] for c in range(C)]
        want_r, want_e = rhat_loops(cols), ess_loops(cols)
        assert abs(got_r[e] - want_r) <= 1e-10 * abs(want_r), (e, got_r[e], want_r)
        assert abs(got_e[e] - want_e) <= 1e-10 * abs(want_e), (e, got_e[e], want_e)
    # autocorrelated draws are worth fewer than C N independent ones, and the cut was used
    assert np.all(got_e > 0) and (N < 100 or np.all(got_e < C * N))
    # a (C, N) input is the K = 1 case
    assert abs(mcmc.rhat(x[:, :, 0], nburn) - got_r[0]) <= 1e-12 * got_r[0]
    assert abs(mcmc.ess(x[:, :, 0], nburn) - got_e[0]) <= 1e-12 * got_e[0]
    assert mcmc.rhat(x[:, :, 0], nburn).shape == ()


@pytest.mark.parametrize("C", [1, 2, 4])
def test_identical_chains(C):
    """C copies of one chain of independent draws: the only between-sequence variance is that of
    the two halves' means, (C / (2 C - 1)) chi2_1 / h against the 1 / h that var+ gives up, so
    R-hat <= 1 for a draw whose halves agree as well as they typically do (this seed)."""
    one = np.random.default_rng(7).standard_normal((1, 200, 2))
    r = mcmc.rhat(np.repeat(one, C, axis=0))
    assert np.all(np.isfinite(r)) and np.all(r <= 1.0), r
    assert np.all(r > 0.98)


def test_chains_shifted_apart():
    """Four chains whose means lie 10 standard deviations apart."""
    x = np.random.default_rng(3).standard_normal((4, 100, 2))
    x += 10.0 * np.arange(4)[:, None, None]
    r = mcmc.rhat(x)
    assert np.all(r > 3.0), r
    assert np.all(mcmc.ess(x) < 4 * 100 / 10)          # and hardly any independent draws


def test_constant_chain_is_nan():
    x = np.full((2, 40, 3), 2.5)
    x[:, :, 1] = np.random.default_rng(0).standard_normal((2, 40))
    with np.errstate(all="raise"):                     # no floating-point warning escapes either
        r, e = mcmc.rhat(x), mcmc.ess(x)
    assert np.isnan(r[0]) and np.isnan(r[2]) and np.isfinite(r[1])
    assert np.isnan(e[0]) and np.isnan(e[2]) and np.isfinite(e[1])
    # too few draws for two halves of two: NaN, not an exception
    assert np.isnan(mcmc.rhat(np.zeros((2, 3)))) and np.isnan(mcmc.ess(np.zeros((2, 3))))
