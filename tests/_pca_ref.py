"""numpy fp64 restatement of gp_pca_trunc's definition (include/gpfit.h), level by level with the
explicit residual -- the thing the kernel never forms:

    e_r = (Y - mu) - sd * (C[:, :p_r] @ V[:p_r]),   tot[r] = (sum e_r^2, sum e_r),
    node[r, j] = sum_i e_r[i, j]^2.
"""
import numpy as np

# the 26 truncation ranks of the reference's architecture study (plot_PC_RMSE.py): every rank up to
# 11, then wider and wider steps up to 100
REFERENCE_RANKS = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 17, 21, 25, 30, 35, 40, 46, 53,
                            60, 67, 74, 82, 91, 100])


def pca_trunc_ref(Y, C, V, ranks, mu=None, sd=None):
    """-> (tot (R, 2), node (R, ncols), abs (R,) = sum |e_r|), all float64."""
    Y = np.asarray(Y, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    n, ncols = Y.shape
    mu = np.zeros(ncols) if mu is None else np.asarray(mu, dtype=np.float64)
    sd = np.ones(ncols) if sd is None else np.asarray(sd, dtype=np.float64)
    e0 = Y - mu[None, :]
    tot = np.zeros((len(ranks), 2))
    node = np.zeros((len(ranks), ncols))
    ab = np.zeros(len(ranks))
    for r, p in enumerate(ranks):
        e = e0 - sd[None, :] * (C[:, :p] @ V[:p, :])
        tot[r] = np.sum(e * e), np.sum(e)
        node[r] = np.sum(e * e, axis=0)
        ab[r] = np.sum(np.abs(e))
    return tot, node, ab


def rmse_var(tot, n, ncols):
    """(Frobenius RMSE, np.var of the residual) from the two sums."""
    N = float(n) * float(ncols)
    return np.sqrt(tot[:, 0] / N), tot[:, 0] / N - (tot[:, 1] / N) ** 2


def ensemble(n, ncols, p, seed, noise=1e-3, dtype=np.float64, stats=True):
    """signal + noise test data: Y = mu + sd * (C V) + noise * scale, with C = U diag(S) of
    decaying S; returns (Y, C, V, mu, sd) (mu = sd = None when not ``stats``).  The noise keeps
    every level's residual well above rounding (1e-3 of the signal's scale)."""
    g = np.random.default_rng(seed)
    S = 2.0 ** (-np.arange(p) / 4.0)
    C = g.standard_normal((n, p)) * S[None, :]
    V = g.standard_normal((p, ncols)) / np.sqrt(max(p, 1))
    mu = g.standard_normal(ncols) * 3.0 if stats else None
    sd = g.uniform(0.5, 2.0, ncols) if stats else None
    Y = C @ V
    if stats:
        Y = mu[None, :] + sd[None, :] * Y
    Y = (Y + noise * g.standard_normal((n, ncols))).astype(dtype)
    return Y, C, V, mu, sd
