"""CPU: the numpy restatement of gp_pca_trunc (tests/_pca_ref.py), which the GPU tests compare
against, agrees with the closed forms of an exact SVD; the curve's derived quantities (rmse, var,
cvar) follow from the two sums.  No device work."""
import numpy as np
import pytest

from _pca_ref import REFERENCE_RANKS, ensemble, pca_trunc_ref, rmse_var


def test_reference_rank_list():
    """plot_PC_RMSE.py:63-64: 26 ranks from 1 to 100, every residue mod 4 among the boundaries."""
    assert len(REFERENCE_RANKS) == 26
    assert REFERENCE_RANKS[0] == 1 and REFERENCE_RANKS[-1] == 100
    assert list(REFERENCE_RANKS[:11]) == list(range(1, 12))
    assert np.all(np.diff(REFERENCE_RANKS) > 0)
    assert set(REFERENCE_RANKS % 4) == {0, 1, 2, 3}


@pytest.mark.parametrize("n,ncols", [(12, 40), (30, 17), (1, 9)])
def test_exact_svd_closed_forms(n, ncols):
    """With the exact SVD of Y and sd = 1, mu = 0: tot[r, 0] = sum_{k >= p_r} S_k^2, the rank-0
    level is sum Y^2, and the residual is orthogonal to nothing it should not be."""
    g = np.random.default_rng(n * 100 + ncols)
    Y = g.standard_normal((n, ncols))
    U, S, Vh = np.linalg.svd(Y, full_matrices=False)
    ranks = list(range(0, len(S) + 1))
    tot, node, ab = pca_trunc_ref(Y, U * S[None, :], Vh, ranks)
    tail = np.array([np.sum(S[p:] ** 2) for p in ranks])
    np.testing.assert_allclose(tot[:-1, 0], tail[:-1], rtol=1e-12)
    assert tot[-1, 0] <= 1e-24 * tot[0, 0]                    # full rank: rounding only
    np.testing.assert_allclose(tot[0, 0], np.sum(Y * Y), rtol=1e-14)
    np.testing.assert_allclose(tot[0, 1], np.sum(Y), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(node.sum(axis=1), tot[:, 0], rtol=1e-13, atol=1e-28)
    assert np.all(np.diff(tot[:, 0]) <= 0)                    # the curve never rises


def test_rank_zero_level_and_statistics():
    """mu and sd enter as (Y - mu) - sd * product: rank 0 is sum (Y - mu)^2 whatever sd is, and
    a residual in physical units is sd times the standardised one."""
    Y, C, V, mu, sd = ensemble(9, 31, 6, seed=3)
    tot, node, ab = pca_trunc_ref(Y, C, V, [0, 2, 6], mu, sd)
    np.testing.assert_allclose(tot[0, 0], np.sum((Y - mu) ** 2), rtol=1e-14)
    np.testing.assert_allclose(tot[0, 1], np.sum(Y - mu), rtol=1e-12)
    Ystd = (Y - mu) / sd
    tstd, nstd, _ = pca_trunc_ref(Ystd, C, V, [0, 2, 6])
    np.testing.assert_allclose(node, nstd * sd[None, :] ** 2, rtol=1e-9)
    np.testing.assert_allclose(node.sum(axis=1), tot[:, 0], rtol=1e-13)
    # at full rank only the noise is left: 1e-3 of the signal's scale, far above rounding
    assert 1e-8 * tot[0, 0] < tot[2, 0] < 1e-4 * tot[0, 0]
    assert np.all(ab > 0)


def test_rmse_var_and_cvar_follow_from_the_sums():
    """rmse = ||e||_F / sqrt(size) and var = np.var(e) from (sum e^2, sum e); cvar of an exact SVD
    is 1 - tot[r, 0] / tot[rank 0, 0]."""
    g = np.random.default_rng(5)
    Y = g.standard_normal((8, 50)) + 0.3
    U, S, Vh = np.linalg.svd(Y, full_matrices=False)
    ranks = [0, 1, 3, 5, 8]
    tot, _, _ = pca_trunc_ref(Y, U * S[None, :], Vh, ranks)
    rmse, var = rmse_var(tot, *Y.shape)
    for r, p in enumerate(ranks):
        e = Y - (U[:, :p] * S[None, :p]) @ Vh[:p]
        np.testing.assert_allclose(rmse[r], np.linalg.norm(e, ord="fro") / np.sqrt(e.size),
                                   rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(var[r], np.var(e), rtol=1e-9, atol=1e-28)
    cvar = np.cumsum(S ** 2) / np.sum(S ** 2)
    np.testing.assert_allclose(cvar[[0, 2, 4]], 1.0 - tot[[1, 2, 3], 0] / tot[0, 0], rtol=1e-10)
    assert cvar[-1] == pytest.approx(1.0, abs=1e-15)


def test_clamped_ranks_equal_full_rank():
    """numpy's slices clamp: a rank above the number of columns is the full rank
    (plot_PC_RMSE.py:98-100 with 16 simulations and ranks up to 100)."""
    Y, C, V, mu, sd = ensemble(5, 20, 4, seed=9)
    tot, _, _ = pca_trunc_ref(Y, C, V, [4, 7, 100], mu, sd)
    assert np.array_equal(tot[0], tot[1]) and np.array_equal(tot[0], tot[2])
