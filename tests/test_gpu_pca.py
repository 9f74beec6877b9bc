"""GPU: the PCA truncation-error curve (gp_pca_trunc, blas.pca_trunc, gladsgp_amd.pca).

Oracle: tests/_pca_ref.py, the explicit fp64 residual per level in numpy.  The inputs are
signal + noise with the noise at 1e-3 of the signal's scale, and the parity ranks stay below
min(n, ncols), so no level's residual is pure rounding: a residual element carries a relative
error of about u |e0| / |e| <~ 1e-13 (u = 2^-53, |e0| / |e| <= ~1e3), whatever the order of the
k-chain and of the sums.  Hence rtol = 1e-10 on tot[:, 0] and node; tot[:, 1] is a cancelling sum
and is compared with atol = 1e-10 sum|e|.
"""
import numpy as np
import pytest
import torch

import _layouts as L
from _pca_ref import REFERENCE_RANKS, ensemble, pca_trunc_ref, rmse_var

pytestmark = pytest.mark.gpu

RTOL = 1e-10
RANK_LISTS = ([0, 1, 2, 3, 4, 5], [3, 7, 8, 13], [1], [37], list(REFERENCE_RANKS))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _check(tot, node, ref, what):
    rt, rn, rabs = ref
    tot = tot.cpu().numpy()
    np.testing.assert_allclose(tot[:, 0], rt[:, 0], rtol=RTOL, atol=0, err_msg=f"{what}: sse")
    assert np.all(np.abs(tot[:, 1] - rt[:, 1]) <= RTOL * rabs), (what, tot[:, 1], rt[:, 1], rabs)
    if node is not None:
        np.testing.assert_allclose(node.cpu().numpy(), rn, rtol=RTOL, atol=0,
                                   err_msg=f"{what}: node")


def _clip(ranks, n, ncols):
    """The parity rows keep their ranks below min(n, ncols) (module docstring)."""
    return [r for r in ranks if r < min(n, ncols)]


@pytest.mark.parametrize("ncols", [1, 15, 16, 17, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_parity(dev, n, ncols):
    """Every rank list (clipped to the shape), float32 and fp64 Y, with and without mu / sd, with
    and without node: the reference's sums; node on or off gives the same tot bits."""
    from gladsgp_amd import blas
    p = max(min(n, ncols) - 1, 1)
    for stats in (True, False):
        Y64, C, V, mu, sd = ensemble(n, ncols, p, seed=1000 * n + ncols + stats, stats=stats)
        Ct, Vt, mut, sdt = _t(C, dev), _t(V, dev), _t(mu, dev), _t(sd, dev)
        for ydt in (np.float64, np.float32):
            Y = Y64.astype(ydt)
            Yt = _t(Y, dev)
            for ranks in RANK_LISTS:
                rk = _clip(ranks, n, ncols)
                if not rk:
                    continue
                ref = pca_trunc_ref(Y, C, V, rk, mu, sd)
                tot, node = blas.pca_trunc(Yt, Ct, Vt, rk, mu=mut, sd=sdt, node=True)
                _check(tot, node, ref, f"{n}x{ncols} {ydt.__name__} stats={stats} {rk}")
                tot2, none = blas.pca_trunc(Yt, Ct, Vt, rk, mu=mut, sd=sdt)
                assert none is None and torch.equal(tot, tot2)


def test_parity_multi_panel(dev):
    """n = 40, ncols = 5000: 79 column panels, three row tiles (the last one partial), the rank
    lists that need more than 33 simulations ([37], the reference's list up to 37)."""
    from gladsgp_amd import blas
    n, ncols = 40, 5000
    Y64, C, V, mu, sd = ensemble(n, ncols, 39, seed=5)
    Ct, Vt, mut, sdt = _t(C, dev), _t(V, dev), _t(mu, dev), _t(sd, dev)
    for ydt in (np.float32, np.float64):
        Y = Y64.astype(ydt)
        Yt = _t(Y, dev)
        for ranks in RANK_LISTS:
            rk = _clip(ranks, n, ncols)
            ref = pca_trunc_ref(Y, C, V, rk, mu, sd)
            tot, node = blas.pca_trunc(Yt, Ct, Vt, rk, mu=mut, sd=sdt, node=True)
            _check(tot, node, ref, f"multi-panel {ydt.__name__} {rk}")
    ref = pca_trunc_ref(Y64, C, V, [37], None, None)
    tot, node = blas.pca_trunc(_t(Y64, dev), Ct, Vt, [37], node=True)
    _check(tot, node, ref, "multi-panel no stats")


def test_limits(dev):
    """nlev = max_levels with rank = max_rank: every level but the last one PC wide (the longest
    padded chain, which takes the one-row-tile kernel), the even spread (no padding at all), and
    a list longer than max_levels, which Python splits, against one call per rank."""
    from gladsgp_amd import blas
    mr, ml = blas.pca_trunc_limits()
    n, ncols = mr + 2, mr + 70
    Y64, C, V, mu, sd = ensemble(n, ncols, mr, seed=11)
    Y = Y64.astype(np.float32)
    Yt, Ct, Vt, mut, sdt = (_t(a, dev) for a in (Y, C, V, mu, sd))
    narrow = list(range(ml - 1)) + [mr]
    even = [mr // ml * (i + 1) for i in range(ml)]
    long_list = list(range(0, 2 * ml + 3)) + [mr]
    for rk in (narrow, even, long_list):
        assert rk[-1] == mr and (len(rk) == ml or rk is long_list)
        ref = pca_trunc_ref(Y, C, V, rk, mu, sd)
        tot, node = blas.pca_trunc(Yt, Ct, Vt, rk, mu=mut, sd=sdt, node=True)
        _check(tot, node, ref, f"limits {rk[:3]}..{rk[-1]} ({len(rk)})")
    # a level's sums do not depend on the other levels of the call: the bits of single-rank calls
    tot, node = blas.pca_trunc(Yt, Ct, Vt, long_list, mu=mut, sd=sdt, node=True)
    for i in (0, 1, 5, ml, ml + 1, len(long_list) - 1):
        t1, n1 = blas.pca_trunc(Yt, Ct, Vt, [long_list[i]], mu=mut, sd=sdt, node=True)
        assert torch.equal(t1[0], tot[i]) and torch.equal(n1[0], node[i]), long_list[i]
    with pytest.raises(ValueError, match="limit"):
        blas.pca_trunc(_t(np.zeros((2, 4)), dev), _t(np.zeros((2, mr + 1)), dev),
                       _t(np.zeros((mr + 1, 4)), dev), [mr + 1])


def test_empty_problems(dev):
    from gladsgp_amd import blas
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)   # noqa: E731
    tot, node = blas.pca_trunc(z(0, 7), z(0, 3), z(3, 7), [1, 3], node=True)
    assert tot.shape == (2, 2) and node.shape == (2, 7)
    assert not tot.any() and not node.any()
    tot, node = blas.pca_trunc(z(5, 0), z(5, 3), z(3, 0), [0, 2])
    assert tot.shape == (2, 2) and node is None and not tot.any()


def _view(emb, rows, cols):
    """The (rows, cols) torch view of an Embedded (1, rows, cols) operand."""
    return torch.as_strided(emb.buf, (rows, cols), (emb.ld, 1), storage_offset=emb.offset)


@pytest.mark.parametrize("ydt", [np.float32, np.float64])
def test_layouts_and_reproducibility(dev, ydt):
    """Y, C, V and node with padded row strides and offset bases inside guarded allocations
    (tests/_layouts.py: the padding is NaN, so a stray read poisons a sum; a stray write shows in
    check), and C as a column sub-view of a wider factor: the tight call's bits, untouched
    padding, and a second call repeats them."""
    from gladsgp_amd import blas
    n, ncols, p = 37, 331, 21
    rk = [0, 2, 7, 9, 20]
    Y64, C, V, mu, sd = ensemble(n, ncols, p, seed=21)
    Y = Y64.astype(ydt)
    mut, sdt = _t(mu, dev), _t(sd, dev)
    tight = blas.pca_trunc(_t(Y, dev), _t(C, dev), _t(V, dev), rk, mu=mut, sd=sdt, node=True)
    _check(tight[0], tight[1], pca_trunc_ref(Y, C, V, rk, mu, sd), "tight")
    again = blas.pca_trunc(_t(Y, dev), _t(C, dev), _t(V, dev), rk, mu=mut, sd=sdt, node=True)
    assert torch.equal(again[0], tight[0]) and torch.equal(again[1], tight[1])
    for case in ("odd_ld", "off8", "off16", "gap16"):
        ye = L.place(Y[None], case, device=dev, dtype=ydt)
        ce = L.place(C[None], case, device=dev)
        ve = L.place(V[None], case, device=dev)
        ne = L.blank_case((1, len(rk), ncols), case, device=dev)
        te = L.blank((1, 1, 2 * len(rk)), offset=3, device=dev)
        tot = torch.as_strided(te.buf, (len(rk), 2), (2, 1), storage_offset=te.offset)
        res = blas.pca_trunc(_view(ye, n, ncols), _view(ce, n, p), _view(ve, p, ncols), rk,
                             mu=mut, sd=sdt, node=True, out=(tot, _view(ne, len(rk), ncols)))
        assert torch.equal(res[0], tight[0]) and torch.equal(res[1], tight[1]), case
        for e in (ye, ce, ve):
            e.check(written=False)
        ne.check()
        te.check()
        assert np.array_equal(ne.extract()[0], tight[1].cpu().numpy())
    # C as the leading columns of a wider factor (ranks stop below its width), V its leading rows
    wide = np.concatenate([C, np.full((n, 5), np.nan)], axis=1)
    tall = np.concatenate([V, np.full((4, ncols), np.nan)], axis=0)
    res = blas.pca_trunc(_t(Y, dev), _t(wide, dev)[:, :p], _t(tall, dev)[:p], rk, mu=mut, sd=sdt,
                         node=True)
    assert torch.equal(res[0], tight[0]) and torch.equal(res[1], tight[1])
    # a list that stops early never reads the later PCs
    poisoned = C.copy()
    poisoned[:, 9:] = np.nan
    res = blas.pca_trunc(_t(Y, dev), _t(poisoned, dev), _t(V, dev), rk[:4], mu=mut, sd=sdt)
    assert torch.equal(res[0], tight[0][:4])


# ------------------------------------------------------------------ gladsgp_amd.pca
def _formula(U, S, Vh, y_mean, y_sd, y_sim):
    """plot_PC_RMSE.py's compute_truncation_error, in fp64."""
    e = y_sim.astype(np.float64) - y_mean - y_sd * (U.astype(np.float64) @ np.diag(S) @ Vh)
    return np.linalg.norm(e, ord="fro") / np.sqrt(e.size), e


def _svd_case(n, ny, seed):
    g = np.random.default_rng(seed)
    y_sim = (g.standard_normal((n, 6)) @ g.standard_normal((6, ny)) * 3.0 + 10.0 +
             0.05 * g.standard_normal((n, ny))).astype(np.float32)
    y_mean = np.mean(y_sim, axis=0)
    y_sd = np.std(y_sim, ddof=1, axis=0)
    y_sd[y_sd < 1e-6] = 1e-6
    y_std = (y_sim - y_mean) / y_sd
    U, S, Vh = np.linalg.svd(y_std.astype(np.float64), full_matrices=False)
    return y_sim, y_mean, y_sd, U, S, Vh


def test_truncation_error_drop_in(dev):
    """The reference's one-liner on a float32 ensemble, to float32 rounding: as a float for one
    (already truncated) rank, S as the np.diag matrix or as a vector; the curve with ranks, ranks
    above U's width clamped to the full rank; numpy in, numpy out."""
    from gladsgp_amd import pca
    n, ny = 20, 700
    y_sim, y_mean, y_sd, U, S, Vh = _svd_case(n, ny, seed=2)
    k = 5
    want, _ = _formula(U[:, :k], S[:k], Vh[:k], y_mean, y_sd, y_sim)
    # float32 statistics and factors, as the reference holds them: agreement to float32 rounding
    got = pca.truncation_error((U[:, :k].astype(np.float32), np.diag(S[:k]).astype(np.float32),
                                Vh[:k].astype(np.float32)), y_mean, y_sd, y_sim, device=dev)
    assert isinstance(got, float) and got == pytest.approx(want, rel=2e-5)
    # fp64 factors: the formula to fp64 rounding; S as a matrix and as a vector agree
    mean64, sd64 = y_mean.astype(np.float64), y_sd.astype(np.float64)
    want64, _ = _formula(U[:, :k], S[:k], Vh[:k], mean64, sd64, y_sim)
    g_mat = pca.truncation_error((U[:, :k], np.diag(S[:k]), Vh[:k]), mean64, sd64, y_sim,
                                 device=dev)
    g_vec = pca.truncation_error((U[:, :k], S[:k], Vh[:k]), mean64, sd64, y_sim, device=dev)
    assert g_mat == pytest.approx(want64, rel=1e-10) and g_vec == pytest.approx(want64, rel=1e-10)
    # the curve; 25 and 100 are above the 20 columns of U: the full-rank value
    ranks = [1, 2, 5, 11, 20, 25, 100, 5]
    cur = pca.truncation_error((U, S, Vh), mean64, sd64, y_sim, ranks=ranks, node=True, device=dev)
    assert isinstance(cur.rmse, np.ndarray) and cur.rmse.shape == (len(ranks),)
    assert cur.node_rmse.shape == (len(ranks), ny) and list(cur.ranks) == ranks
    for i, r in enumerate(ranks):
        if r >= n - 1:                # rank >= n - 1: the residual of a centred ensemble is rounding
            assert cur.rmse[i] <= 1e-5 * cur.rmse[0]
            continue
        w, e = _formula(U[:, :r], S[:r], Vh[:r], mean64, sd64, y_sim)
        assert cur.rmse[i] == pytest.approx(w, rel=1e-9), r
        assert cur.var[i] == pytest.approx(np.var(e), rel=1e-8), r
        np.testing.assert_allclose(cur.node_rmse[i], np.sqrt(np.mean(e * e, axis=0)), rtol=1e-8)
        np.testing.assert_allclose(cur.sse[i], np.sum(e * e), rtol=1e-9)
    assert cur.rmse[5] == cur.rmse[4] == cur.rmse[6] and cur.rmse[7] == cur.rmse[2]
    # device tensors in, device tensors out
    cur_t = pca.truncation_error((_t(U, dev), _t(S, dev), _t(Vh, dev)), _t(mean64, dev),
                                 _t(sd64, dev), _t(y_sim, dev), ranks=[1, 5])
    assert torch.is_tensor(cur_t.rmse) and cur_t.rmse.device.type == "cuda"
    np.testing.assert_array_equal(cur_t.rmse.cpu().numpy(), cur.rmse[[0, 2]])


def test_truncation_curve(dev):
    """plot_PC_RMSE.py:84-108 on a 24 x 700 float32 ensemble with a seeded omega: rmse at every
    rank equals the formula applied to the U, S, Vh the call returns (with the float32
    ensemble's fp64 mean and floored ddof=1 sd), cvar = cumsum(S^2) / sum(S^2)."""
    from gladsgp_amd import pca
    n, ny, pmax = 24, 700, 100
    y_sim = _svd_case(n, ny, seed=4)[0]
    y_sim[:, 13] = 7.0                                         # a constant node: sd floored
    omega = np.random.default_rng(8).standard_normal((ny, min(pmax, n))).astype(np.float32)
    ranks = [int(r) for r in REFERENCE_RANKS]
    cur = pca.truncation_curve(y_sim, ranks, pmax=pmax, k=0, q=1, omega=omega, device=dev)
    assert cur.U.shape == (n, n) and cur.S.shape == (n,) and cur.Vh.shape == (n, ny)
    y64 = y_sim.astype(np.float64)
    mean = y64.mean(axis=0)
    sd = np.maximum(y64.std(axis=0, ddof=1), 1e-6)
    assert sd[13] == 1e-6
    for i, r in enumerate(ranks):
        w, _ = _formula(cur.U[:, :r], cur.S[:r], cur.Vh[:r], mean, sd, y_sim)
        assert cur.rmse[i] == pytest.approx(w, rel=1e-7, abs=1e-9 * cur.rmse[0]), r
    np.testing.assert_allclose(cur.cvar, np.cumsum(cur.S ** 2) / np.sum(cur.S ** 2), rtol=1e-13)
    assert np.all(np.diff(cur.rmse) <= 1e-9 * cur.rmse[0]) and cur.rmse[0] > 10 * cur.rmse[10]
    # the randomized factors are the ensemble's SVD here (n test vectors span its range)
    S_np = np.linalg.svd((y64 - mean) / sd, compute_uv=False)
    np.testing.assert_allclose(cur.S[:6], S_np[:6], rtol=1e-8)


def test_truncation_variance(dev):
    """include_trunc_error.py:42-47 against numpy in fp64."""
    from gladsgp_amd import pca
    g = np.random.default_rng(6)
    n, ny, P = 18, 900, 5
    K = g.standard_normal((P, ny)) * g.uniform(0.5, 3.0, (P, 1))
    y_sim = (g.standard_normal((n, P)) @ K + 2.0 + 0.1 * g.standard_normal((n, ny))).astype(
        np.float32)
    Kn = K / np.vstack(np.linalg.norm(K, axis=1))
    y64 = y_sim.astype(np.float64)
    want = np.var(y64 - y64 @ Kn.T @ Kn)
    got = pca.truncation_variance(y_sim, K, device=dev)
    assert isinstance(got, float) and got == pytest.approx(want, rel=1e-9)
    got_t = pca.truncation_variance(_t(y_sim, dev), _t(K, dev))
    assert got_t == got
