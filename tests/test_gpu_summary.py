"""GPU: the fused predictive summary (gp_field_summary, blas.field_summary,
EmulatorPrediction.summary) against numpy on the field it never stores.

Expected values: np.mean(y, 0) and np.quantile(z, q, 0) of the fp64 output of the existing
blas.field at the same inputs (y without, z with the error term), whose elements the summary
kernel forms bit for bit.  Tolerances are derived, not tuned:
  * quantiles  4 * 2^-52 * max|z|: the order statistics are selections (exact), the interpolation
    rounds three times;
  * mean       S * 2^-52 * max|y|: two fixed-order fp64 sums of S terms, differently ordered;
  * float32 outputs equal the fp64 outputs cast to float32, bit for bit;
  * q = 0 / (0, 1) give the minimum and maximum exactly (t = 0).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(dev, S, m, P, ncols, err, sdmu, seed=0):
    """W3: a strided (S, m, P) view (ldw = P + 3, lds > m ldw); K: a column block of a wider
    matrix; sd > 0, mu, err as asked."""
    rng = np.random.default_rng(seed)
    wbuf = torch.as_tensor(rng.standard_normal((S, m + 2, P + 3)), device=dev)
    W3 = wbuf[:, :m, :P]
    kbuf = torch.as_tensor(rng.standard_normal((P, ncols + 11)), device=dev)
    K = kbuf[:, 5:5 + ncols]
    sd = mu = e = None
    if sdmu:
        sd = torch.as_tensor(rng.uniform(0.5, 2.0, ncols), device=dev)
        mu = torch.as_tensor(rng.standard_normal(ncols) * 3.0, device=dev)
    if err:
        e = torch.as_tensor(rng.standard_normal(S * m) * 0.3, device=dev)
    return W3, K, sd, mu, e


def _reference(W3, K, sd, mu, e, q):
    """numpy on the stored fp64 field (blas.field): mean of y, quantiles of z, and their scales."""
    from gladsgp_amd import blas
    S, m, P = W3.shape
    W2 = W3.contiguous().reshape(S * m, P)
    y = blas.field(W2, K, sd, mu, None).cpu().numpy().reshape(S, m, -1)
    z = y if e is None else blas.field(W2, K, sd, mu, e).cpu().numpy().reshape(S, m, -1)
    q_lo, q_hi = (q, 1 - q) if np.ndim(q) == 0 else q
    return (np.mean(y, 0), np.quantile(z, q_lo, 0), np.quantile(z, q_hi, 0),
            np.abs(y).max(), np.abs(z).max(), z)


def _check(got, ref, S, exact_extremes=False):
    mean, lo, hi = (t.cpu().numpy() for t in got)
    r_mean, r_lo, r_hi, ymax, zmax, z = ref
    print(f"S={S} mean err {np.abs(mean - r_mean).max():.3e} (tol {S * EPS * ymax:.3e}), "
          f"lo err {np.abs(lo - r_lo).max():.3e}, hi err {np.abs(hi - r_hi).max():.3e} "
          f"(tol {4 * EPS * zmax:.3e})")
    assert mean.shape == r_mean.shape and lo.shape == r_lo.shape and hi.shape == r_hi.shape
    assert np.abs(mean - r_mean).max() <= S * EPS * ymax
    assert np.abs(lo - r_lo).max() <= 4 * EPS * zmax
    assert np.abs(hi - r_hi).max() <= 4 * EPS * zmax
    if exact_extremes:
        assert np.array_equal(lo, z.min(0)) and np.array_equal(hi, z.max(0))


# a cross-section of S x P x m x ncols x err x (sd, mu) x q in which every value appears: one
# sample, a partial first tile, exact tiles, one row past a 16- and a 32-sample tile; every
# k-step count; columns below, across and beyond a block's 128-column panel; every list depth
SWEEP = [
    (1, 1, 1, 1, False, False, 0.025),
    (2, 8, 3, 31, True, True, 0.025),
    (5, 9, 1, 257, True, False, 0),
    (16, 25, 3, 1000, False, True, (0, 1)),
    (17, 64, 1, 31, True, True, 0.025),
    (33, 8, 3, 257, True, True, 0.025),
    (64, 9, 3, 1000, True, True, 0.025),
    (64, 8, 3, 257, True, True, 0),
    (128, 25, 1, 257, True, True, 0.025),
    (128, 64, 3, 31, False, False, 0.025),
    (33, 64, 1, 1000, True, True, (0, 1)),
]


@pytest.mark.parametrize("S,P,m,ncols,err,sdmu,q", SWEEP)
def test_shape_sweep(dev, S, P, m, ncols, err, sdmu, q):
    from gladsgp_amd import blas
    W3, K, sd, mu, e = _inputs(dev, S, m, P, ncols, err, sdmu, seed=S + P)
    assert W3.stride(0) > m * W3.stride(1) and K.stride(0) > ncols
    ref = _reference(W3, K, sd, mu, e, q)
    got = blas.field_summary(W3, K, sd, mu, e, q=q)
    assert all(t.dtype == torch.float64 and t.shape == (m, ncols) for t in got)
    _check(got, ref, S, exact_extremes=(q == 0 or q == (0, 1)))
    got32 = blas.field_summary(W3, K, sd, mu, e, q=q, f32=True)
    for a, b in zip(got32, got):
        assert a.dtype == torch.float32
        assert torch.equal(a.view(torch.int32), b.to(torch.float32).view(torch.int32))


@pytest.mark.parametrize("S", [7, 64])
def test_identical_samples(dev, S):
    """All S samples equal: lo == hi bitwise, and both equal the mean to the tolerances."""
    from gladsgp_amd import blas
    W3, K, sd, mu, _ = _inputs(dev, S, 2, 8, 200, False, True, seed=3)
    W3 = W3[:1].expand(S, 2, 8).contiguous()
    e = torch.as_tensor(np.tile(np.array([0.25, -0.5]), S), device=dev)   # one value per point
    for err in (None, e):
        mean, lo, hi = blas.field_summary(W3, K, sd, mu, err, q=0.025)
        assert torch.equal(lo.view(torch.int64), hi.view(torch.int64))
        ref = _reference(W3, K, sd, mu, err, 0.025)
        _check((mean, lo, hi), ref, S)
        if err is None:
            assert (mean - lo).abs().max().item() <= (S + 4) * EPS * ref[3]


@pytest.mark.parametrize("P", [8, 40])                   # 32- and 16-sample tiles
@pytest.mark.parametrize("order", ["ascending", "descending", "extremes_last"])
def test_sample_order(dev, P, order):
    """Order-dependent inputs (a wrong insertion or cross-lane merge shows here): every column's
    z_s already sorted ascending in s, descending, and with the extreme values in the last,
    partial tile (S = 37: five rows past a 32-sample tile, the third 16-sample tile partial)."""
    from gladsgp_amd import blas
    S, m, ncols = 37, 2, 150
    W3, K, sd, mu, _ = _inputs(dev, S, m, P, ncols, False, True, seed=11)
    W3 = W3[:1].expand(S, m, P).contiguous()             # the K term is the same for every s
    lev = np.arange(S, dtype=np.float64) - S / 2         # distinct levels, z monotone in them
    if order == "descending":
        lev = lev[::-1].copy()
    elif order == "extremes_last":
        lev = np.random.default_rng(5).permutation(lev[2:-2])
        lev = np.concatenate([lev, [S, -S, S - 1.5, 1.5 - S]])     # samples 33..36
    e = torch.as_tensor(np.repeat(lev[:, None], m, 1).reshape(-1), device=dev)
    for q in (0.025, 0.1, (0, 1)):
        got = blas.field_summary(W3, K, sd, mu, e, q=q)
        _check(got, _reference(W3, K, sd, mu, e, q), S, exact_extremes=(q == (0, 1)))


@pytest.mark.parametrize("P", [5, 12, 25, 40, 64])       # k-steps 2, 4, 8, 12, 16
def test_one_sample_is_the_field(dev, P):
    """S = 1, q = (0, 1): the lists hold the one value, _lerp at t = 0 returns it and the mean is
    y + 0 over 1, so the summary's maps are gp_field's elements themselves: mean = field without
    the error term, lo = hi = field with it, bit for bit, fp64 and float32 (three panels, the
    last one ragged; strided W and K)."""
    from gladsgp_amd import blas
    m, ncols = 37, 300
    W3, K, sd, mu, e = _inputs(dev, 1, m, P, ncols, True, True, seed=P)
    assert W3.stride(1) > P and K.stride(0) > ncols
    for f32 in (False, True):
        mean, lo, hi = blas.field_summary(W3, K, sd, mu, e, q=(0, 1), f32=f32)
        y = blas.field(W3[0], K, sd, mu, None, f32=f32)
        z = blas.field(W3[0], K, sd, mu, e, f32=f32)
        assert mean.dtype == y.dtype and mean.shape == y.shape == (m, ncols)
        assert torch.equal(mean, y), f32
        assert torch.equal(lo, z), f32
        assert torch.equal(hi, z), f32


@pytest.mark.parametrize("f32", [True, False])
def test_output_views_any_alignment(dev, f32):
    """Outputs written into a column block of a wider buffer at element offsets 0-3: the block
    equals the contiguous result bit for bit, nothing outside it changes."""
    from gladsgp_amd import blas
    S, m, P, ncols = 20, 3, 8, 133
    W3, K, sd, mu, e = _inputs(dev, S, m, P, ncols, True, True, seed=7)
    dt = torch.float32 if f32 else torch.float64
    want = blas.field_summary(W3, K, sd, mu, e, q=0.025, f32=f32)
    for off in range(4):
        bufs = [torch.full((m, ncols + 9), -777.0, dtype=dt, device=dev) for _ in range(3)]
        out = [b[:, off:off + ncols] for b in bufs]
        got = blas.field_summary(W3, K, sd, mu, e, q=0.025, f32=f32, out=out)
        for b, g, w in zip(bufs, got, want):
            assert torch.equal(g, w)
            assert torch.equal(b[:, off:off + ncols], w)
            assert bool((b[:, :off] == -777.0).all()) and bool((b[:, off + ncols:] == -777.0).all())


# ------------------------------------------------------------------ EmulatorPrediction.summary
def _ensemble(n=64, ny=300, d=6, seed=2):
    rng = np.random.default_rng(seed)
    t = rng.random((n, d))
    modes = rng.standard_normal((5, ny)) * (0.5 ** np.arange(5))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + k) for k in range(5)], 1)
    y = (3.0 + coef @ modes + 1e-2 * rng.standard_normal((n, ny))).astype(np.float32)
    return t.astype(np.float32), y


def _samples(S, d, P, seed=1):
    rng = np.random.default_rng(seed)
    return {"betaU": rng.uniform(0.2, 3.0, (S, (d + 1) * P)),
            "lamUz": rng.uniform(0.5, 3.0, (S, P)),
            "lamWs": rng.uniform(200, 3000, (S, P)),
            "lamWOs": rng.uniform(50, 500, (S, 1))}


@pytest.fixture(scope="module")
def preds_by_S(dev, tmp_path_factory):
    """A small fitted-shape model (n = 64, P = 4, ny = 300) and its predictions at m = 5 test
    points for S = 6 and S = 64 posterior samples, with marginal draws so the band has width."""
    from gladsgp_amd import model as gm
    from gladsgp_amd.emulator import EmulatorPrediction
    t, y = _ensemble()
    data, model = gm.init_model(t, y, "summary", 4, data_dir=str(tmp_path_factory.mktemp("d")),
                                device=dev, verbose=False)
    t_pred = np.random.default_rng(5).random((5, t.shape[1]))
    return {S: EmulatorPrediction(model=model, samples=_samples(S, t.shape[1], 4, seed=4),
                                  t_pred=t_pred, realize=True, seed=99) for S in (6, 64)}


def _numpy_summary(preds, q, w=None):
    y = preds.get_y(w=w)
    z = preds.get_y(w=w, add_error=True, rng=np.random.default_rng(7))
    assert y.dtype == np.float64 and z.dtype == np.float64
    q_lo, q_hi = (q, 1 - q) if np.ndim(q) == 0 else q
    return (np.mean(y, 0), np.quantile(z, q_lo, 0), np.quantile(z, q_hi, 0),
            np.abs(y).max(), np.abs(z).max(), z)


def test_depth_limit_takes_the_fallback(preds_by_S):
    """S = 64 with q = 0.2 needs 14 order statistics per tail: summary() reduces the stored
    field instead (same tolerances), the kernel's own entry point refuses."""
    from gladsgp_amd import _capi, blas
    preds = preds_by_S[64]
    got = preds.summary(0.2, rng=np.random.default_rng(7), to_host=False)
    _check(got, _numpy_summary(preds, 0.2), 64)
    with pytest.raises(_capi.GPFitError) as ei:
        blas.field_summary(preds.w_dev, preds.model.data.sim_data.K, q=0.2)
    assert ei.value.rc == -13


@pytest.mark.parametrize("S", [6, 64])
def test_dropin_summary(preds_by_S, S):
    """preds.summary(q, rng) == mean of get_y() and quantiles of get_y(add_error=True, rng) with
    the same seed; two runs are bit-identical; after ``preds.w = preds.w.astype(np.float32)`` the
    outputs are float32: the fp64 result of the cast weights rounded once (half a float32 ulp on
    top of the fp64 tolerance)."""
    preds = preds_by_S[S]
    got = preds.summary(0.025, rng=np.random.default_rng(7))
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (5, 300)
               for a in got)
    _check([torch.as_tensor(a) for a in got], _numpy_summary(preds, 0.025), S)
    again = preds.summary(0.025, rng=np.random.default_rng(7))
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    assert np.all(got[2] >= got[1])
    # no error term: the band collapses onto the samples' own spread, the mean is unchanged
    plain = preds.summary(0.025, add_error=False)
    assert np.array_equal(plain[0], got[0])

    w64 = preds.w
    try:
        preds.w = w64.astype(np.float32)
        got32 = preds.summary(0.025, rng=np.random.default_rng(7))
        assert all(a.dtype == np.float32 and a.shape == (5, 300) for a in got32)
        r_mean, r_lo, r_hi, ymax, zmax, _ = _numpy_summary(preds, 0.025, w=preds.w)
        for g, r, tol in ((got32[0], r_mean, S * EPS * ymax), (got32[1], r_lo, 4 * EPS * zmax),
                          (got32[2], r_hi, 4 * EPS * zmax)):
            assert np.all(np.abs(g.astype(np.float64) - r) <= 2.0 ** -24 * np.abs(r) + tol)
        again32 = preds.summary(0.025, rng=np.random.default_rng(7))
        assert all(np.array_equal(a, b) for a, b in zip(got32, again32))
    finally:
        preds.w = w64
