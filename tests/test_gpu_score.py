"""GPU: the fused test-error scores (gp_field_score, blas.field_score, EmulatorPrediction.score,
EmulatorXvalPrediction.score).

Oracle: the numpy reference tests/_score_ref.py applied to the maps the existing
blas.field_summary stores for the same inputs (tested against numpy on its own in
test_gpu_summary.py).  The kernel forms the same fp64 terms from the same stored values, so
  * every count is equal exactly;
  * every sum differs by at most N * 2^-52 * sum|terms| (two orderings of N fp64 terms);
  * the optional mean / lo / hi outputs equal field_summary's bit for bit;
  * two calls give the same bits.
"""
import numpy as np
import pytest
import torch

import _layouts as L
from _score_ref import COL, ROW, assert_sums_match, score_sums

pytestmark = pytest.mark.gpu

ROW_SUMS = [ROW[k] for k in ("sqerr", "ape", "lo", "hi", "mean")]
ROW_CNTS = [ROW[k] for k in ("valid", "ape_n", "covered")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(dev, S, m, P, ncols, err, sdmu, seed=0):
    """W3: a strided (S, m, P) view (ldw = P + 3, lds > m ldw); K: a column block of a wider
    matrix; sd > 0, mu, err as asked (the operands of test_gpu_summary.py)."""
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


def _truth(maps, y_dtype, seed):
    """A truth that takes every branch: mean + noise of the band's size, ~5 % NaN, entries set
    exactly to the stored lo / hi of their element (inclusive bounds), one row all NaN when there
    is more than one; the floor leaves about a third of the entries below it."""
    mean, lo, hi = (np.asarray(a).astype(np.float64) for a in maps)
    m, n = mean.shape
    rng = np.random.default_rng(seed)
    y = mean + rng.standard_normal((m, n)) * (0.6 * (hi - lo) + 0.1)
    on_lo, on_hi = rng.random((m, n)) < 0.1, rng.random((m, n)) < 0.1
    y[on_lo] = lo[on_lo]
    y[on_hi] = hi[on_hi]
    y[rng.random((m, n)) < 0.05] = np.nan
    if m > 1:
        y[1] = np.nan
    y = y.astype(y_dtype)
    floor = float(np.nanquantile(y.astype(np.float64), 0.3)) if np.isfinite(y).any() else 0.0
    return y, floor


# a cross-section in which every value of S, P, m, ncols appears, every list depth (2: q = 0.025
# up to S = 33 and the extremes; 4: q = 0.025 at S = 64; 8: q = 0.1 at S = 64), with and without
# sd / mu and err, float32 and fp64 outputs, a float32 and an fp64 truth
SWEEP = [
    # S   P   m  ncols  err    sdmu   q       f32    y32
    (1, 1, 1, 1, False, False, 0.025, False, False),
    (5, 8, 3, 31, True, True, 0.025, True, True),
    (17, 9, 1, 257, True, False, 0, False, True),
    (33, 25, 3, 1000, False, True, 0.025, True, False),
    (33, 40, 3, 257, True, True, (0, 1), False, False),
    (64, 64, 3, 31, True, True, 0.025, False, False),
    (64, 8, 3, 257, True, True, 0.1, True, True),
    (64, 64, 1, 1000, True, True, 0.1, False, False),
]


@pytest.mark.parametrize("S,P,m,ncols,err,sdmu,q,f32,y32", SWEEP)
def test_shape_sweep(dev, S, P, m, ncols, err, sdmu, q, f32, y32):
    from gladsgp_amd import blas
    W3, K, sd, mu, e = _inputs(dev, S, m, P, ncols, err, sdmu, seed=S + P)
    want = blas.field_summary(W3, K, sd, mu, e, q=q, f32=f32)
    maps = [t.cpu().numpy() for t in want]
    y, floor = _truth(maps, np.float32 if y32 else np.float64, seed=S)
    Y = torch.as_tensor(y, device=dev)
    if y32 == f32:                                    # the planted bounds are hit exactly
        assert (y == maps[1]).sum() + (y == maps[2]).sum() > 0 or ncols == 1
    # with the maps: the same bits as field_summary, and the sums
    out = [torch.full_like(t, -5.0) for t in want]
    res = blas.field_score(W3, K, sd, mu, e, Y, q=q, mape_floor=floor, f32=f32, out=out)
    assert len(res) == 5 and res[0].shape == (m, 8) and res[1].shape == (ncols, 4)
    for a, b in zip(res[2:], want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    rows, cols = res[0].cpu().numpy(), res[1].cpu().numpy()
    assert_sums_match(rows, cols, score_sums(*maps, y, floor), "maps + floor")
    # without the maps: the same bits again; every floor; no per-node sums; no truth
    r2, c2 = blas.field_score(W3, K, sd, mu, e, Y, q=q, mape_floor=floor, f32=f32)
    assert np.array_equal(r2.cpu().numpy(), rows) and np.array_equal(c2.cpu().numpy(), cols)
    for fl in (-np.inf, np.nan, np.inf):
        r, c = blas.field_score(W3, K, sd, mu, e, Y, q=q, mape_floor=fl, f32=f32)
        assert_sums_match(r.cpu().numpy(), c.cpu().numpy(), score_sums(*maps, y, fl), f"floor {fl}")
    r, c = blas.field_score(W3, K, sd, mu, e, Y, q=q, mape_floor=floor, f32=f32, cols=False)
    assert c is None and np.array_equal(r.cpu().numpy(), rows)
    r, c = blas.field_score(W3, K, sd, mu, e, None, q=q, f32=f32)
    r, c = r.cpu().numpy(), c.cpu().numpy()
    assert_sums_match(r, c, score_sums(*maps, None), "no truth")
    assert np.all(r[:, ROW_CNTS] == 0) and np.all(r[:, [ROW["sqerr"], ROW["ape"]]] == 0)
    assert np.array_equal(r[:, [ROW["lo"], ROW["hi"], ROW["mean"]]],
                          rows[:, [ROW["lo"], ROW["hi"], ROW["mean"]]])
    assert np.array_equal(c[:, COL["width"]], cols[:, COL["width"]])
    if m > 1:                                         # the row without truth: zero counts
        assert np.all(rows[1, ROW_CNTS] == 0) and rows[1, ROW["sqerr"]] == 0


def test_more_units_than_blocks(dev):
    """More (panel, point) units than resident blocks: a block's range starts and ends inside a
    panel, so panels are split between blocks and blocks span several panels."""
    from gladsgp_amd import blas
    S, P, m, ncols = 8, 8, 5, 128 * 300 + 7
    units = -(-ncols // 128) * m
    # the launcher takes at most one residency round: CUs x blocks per CU, and the 34.5 KB of
    # LDS per block bound the latter by 4 (160 KB per CU)
    grid_max = torch.cuda.get_device_properties(dev).multi_processor_count * 4
    if units <= grid_max:
        pytest.skip(f"{units} units do not exceed the largest grid ({grid_max} blocks) here")
    W3, K, sd, mu, e = _inputs(dev, S, m, P, ncols, True, True, seed=1)
    want = blas.field_summary(W3, K, sd, mu, e, q=0.025)
    maps = [t.cpu().numpy() for t in want]
    y, floor = _truth(maps, np.float64, seed=2)
    Y = torch.as_tensor(y, device=dev)
    out = [torch.empty_like(t) for t in want]
    res = blas.field_score(W3, K, sd, mu, e, Y, q=0.025, mape_floor=floor, out=out)
    for a, b in zip(res[2:], want):
        assert torch.equal(a, b)
    rows, cols = res[0].cpu().numpy(), res[1].cpu().numpy()
    assert_sums_match(rows, cols, score_sums(*maps, y, floor), "big")
    again = blas.field_score(W3, K, sd, mu, e, Y, q=0.025, mape_floor=floor)
    assert np.array_equal(again[0].cpu().numpy(), rows)
    assert np.array_equal(again[1].cpu().numpy(), cols)


def _view(emb, m, ncols):
    """The (m, ncols) torch view of an Embedded (1, m, ncols) operand."""
    return torch.as_strided(emb.buf, (m, ncols), (emb.ld, 1), storage_offset=emb.offset)


@pytest.mark.parametrize("f32", [False, True])
def test_layouts_and_reproducibility(dev, f32):
    """W3 a strided view, K a column block, Y and the optional maps with padded row strides and
    an offset base inside guarded allocations: the guards are untouched, Y is only read inside
    its elements (the padding is NaN: a stray read would change a count), the results are the
    tight layout's bits, and a second call repeats them."""
    from gladsgp_amd import blas
    S, m, P, ncols = 20, 3, 8, 261
    W3, K, sd, mu, e = _inputs(dev, S, m, P, ncols, True, True, seed=7)
    assert W3.stride(0) > m * W3.stride(1) and K.stride(0) > ncols
    odt = np.float32 if f32 else np.float64
    want = blas.field_summary(W3, K, sd, mu, e, q=0.025, f32=f32)
    maps = [t.cpu().numpy() for t in want]
    for ydt in (np.float64, np.float32):
        y, floor = _truth(maps, ydt, seed=9)
        tight = blas.field_score(W3, K, sd, mu, e, torch.as_tensor(y, device=dev), q=0.025,
                                 mape_floor=floor, f32=f32)
        assert_sums_match(tight[0].cpu().numpy(), tight[1].cpu().numpy(),
                          score_sums(*maps, y, floor), "tight")
        for off, pad in ((1, 3), (3, 8)):
            ye = L.embed(y[None], offset=off, ld=ncols + pad, device=dev, dtype=ydt)
            outs = [L.blank((1, m, ncols), offset=off + 1, ld=ncols + pad + 2, device=dev,
                            dtype=odt) for _ in range(3)]
            res = blas.field_score(W3, K, sd, mu, e, _view(ye, m, ncols), q=0.025,
                                   mape_floor=floor, f32=f32,
                                   out=[_view(o, m, ncols) for o in outs])
            assert torch.equal(res[0], tight[0]) and torch.equal(res[1], tight[1])
            ye.check(written=False)
            for o, w in zip(outs, maps):
                o.check()
                assert np.array_equal(o.extract()[0].view(L._UINT[np.dtype(odt)]),
                                      w.view(L._UINT[np.dtype(odt)]))
            rep = blas.field_score(W3, K, sd, mu, e, _view(ye, m, ncols), q=0.025,
                                   mape_floor=floor, f32=f32)
            assert torch.equal(rep[0], tight[0]) and torch.equal(rep[1], tight[1])


# ------------------------------------------------------------------ EmulatorPrediction.score
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
def fitted(dev, tmp_path_factory):
    """A small fitted-shape model (n = 64, P = 4, ny = 300), its predictions at m = 5 test points
    for S = 6 and S = 64 posterior samples (the fixture of test_gpu_summary.py), and its
    cross-validated predictions with seven folds of eight: simulations 56..63 are in no fold."""
    from gladsgp_amd import model as gm
    from gladsgp_amd.emulator import EmulatorPrediction, EmulatorXvalPrediction
    t, y = _ensemble()
    data, model = gm.init_model(t, y, "score", 4, data_dir=str(tmp_path_factory.mktemp("d")),
                                device=dev, verbose=False)
    t_pred = np.random.default_rng(5).random((5, t.shape[1]))
    preds = {S: EmulatorPrediction(model=model, samples=_samples(S, t.shape[1], 4, seed=4),
                                   t_pred=t_pred, realize=True, seed=99) for S in (6, 64)}
    folds = [list(range(8 * k, 8 * k + 8)) for k in range(7)]
    xval = EmulatorXvalPrediction(leave_out_inds=folds, model=model,
                                  samples=_samples(6, t.shape[1], 4, seed=4), realize=True,
                                  seed=99)
    return preds, xval, y


def _y_test(preds, seed=3):
    mean, lo, hi = preds.summary(0.025, rng=np.random.default_rng(7))
    return _truth((mean, lo, hi), np.float64, seed)


@pytest.mark.parametrize("S", [6, 64])
def test_dropin_score(fitted, dev, S):
    """preds.score(y_test, q, rng) == the reference sums of preds.summary(q, rng) with the same
    seed, for a numpy and a device truth in either dtype, with and without the maps, and after
    the float32 cast of .w; the derived statistics are the reference's expressions."""
    preds = fitted[0][S]
    y, floor = _y_test(preds)
    w64 = preds.w
    try:
        for cast in (False, True):
            if cast:
                preds.w = w64.astype(np.float32)
            maps = preds.summary(0.025, rng=np.random.default_rng(7))
            assert maps[0].dtype == (np.float32 if cast else np.float64)
            s = preds.score(y, 0.025, rng=np.random.default_rng(7))
            assert isinstance(s.rows, np.ndarray) and s.rows.shape == (5, 8)
            assert s.cols.shape == (300, 4) and s.maps is None
            assert_sums_match(s.rows, s.cols, score_sums(*maps, y), f"cast={cast}")
            # the same call again, a float32 host truth, a device truth, a floor, the maps
            s2 = preds.score(y, 0.025, rng=np.random.default_rng(7))
            assert np.array_equal(s2.rows, s.rows) and np.array_equal(s2.cols, s.cols)
            y32 = y.astype(np.float32)
            s3 = preds.score(y32, 0.025, mape_floor=floor, rng=np.random.default_rng(7),
                             maps=True)
            assert_sums_match(s3.rows, s3.cols, score_sums(*maps, y32, floor), "y32 + floor")
            assert all(np.array_equal(a, b) and a.dtype == b.dtype
                       for a, b in zip(s3.maps, maps))
            s4 = preds.score(torch.as_tensor(y, device=dev), 0.025,
                             rng=np.random.default_rng(7), to_host=False)
            assert torch.is_tensor(s4.rows) and s4.rows.is_cuda
            assert np.array_equal(s4.rows.cpu().numpy(), s.rows)
            assert np.array_equal(s4.rmse, s.rmse, equal_nan=True)
            # prediction only: the integration-point loop
            s5 = preds.score(None, 0.025, rng=np.random.default_rng(7))
            assert_sums_match(s5.rows, s5.cols, score_sums(*maps, None), "no truth")
            assert np.isnan(s5.rmse).all() and np.array_equal(s5.width, s.width)
            # derived statistics against the reference's expressions on the stored maps
            mean, lo, hi = (a.astype(np.float64) for a in maps)
            ok = ~np.isnan(y).all(1)
            with np.errstate(invalid="ignore"):
                rmse = np.sqrt(np.nanmean((mean[ok] - y[ok]) ** 2, axis=1))
            assert np.allclose(s.rmse[ok], rmse, rtol=1e-12, atol=0)
            assert np.isnan(s.rmse[~ok]).all() and np.isnan(s.frac_covered[~ok]).all()
            assert np.allclose(s.lower, lo.mean(1), rtol=1e-12, atol=0)
            assert np.allclose(s.upper, hi.mean(1), rtol=1e-12, atol=0)
            assert np.allclose(s.node_width, (hi - lo).mean(0), rtol=1e-12, atol=0)
            cov = (y >= lo) & (y <= hi)
            assert np.array_equal(s.n_covered, cov.sum(1))
            assert s.table(1.5).shape == (5, 6) and np.all(s.table(1.5)[:, 4] == 1.5)
    finally:
        preds.w = w64


def test_depth_limit_takes_the_block_route(fitted):
    """S = 64 with q = 0.2 needs 14 order statistics per tail: score() reduces summary()'s stored
    maps with torch (the same sums to the ordering tolerance, exact counts)."""
    preds = fitted[0][64]
    y, floor = _y_test(preds)
    maps = preds.summary(0.2, rng=np.random.default_rng(7))
    s = preds.score(y, 0.2, mape_floor=floor, rng=np.random.default_rng(7), maps=True)
    assert_sums_match(s.rows, s.cols, score_sums(*maps, y, floor), "block route")
    assert all(np.array_equal(a, b) for a, b in zip(s.maps, maps))


def test_xval_score(fitted):
    """EmulatorXvalPrediction.score() against the training simulations: the simulations in a fold
    score as summary()'s maps do; those in no fold (NaN predictions) come out as NaN sums with
    zero counts and enter no per-node sum."""
    _, xval, y_sim = fitted
    keep = np.arange(64) < 56
    maps = xval.summary(0.025, rng=np.random.default_rng(7))
    assert np.isnan(maps[0][~keep]).all() and np.isfinite(maps[0][keep]).all()
    s = xval.score(rng=np.random.default_rng(7), maps=True)
    ysim = np.asarray(y_sim, dtype=np.float64)
    ref = score_sums(*[a[keep] for a in maps], ysim[keep])
    assert_sums_match(s.rows[keep], s.cols, ref, "xval")
    assert np.all(s.rows[~keep][:, ROW_CNTS] == 0) and np.isnan(s.rows[~keep][:, ROW_SUMS]).all()
    assert np.isnan(s.rmse[~keep]).all() and np.isfinite(s.rmse[keep]).all()
    assert np.isfinite(s.node_rmse).all() and np.all(s.node_n_valid == 56)
    assert np.isfinite(s.total_rmse)
    # per-node means are over the 56 scored simulations, not over all 64 rows
    lo64, hi64 = (a[keep].astype(np.float64) for a in maps[1:])
    assert s.n_scored == 56
    assert np.allclose(s.node_width, (hi64 - lo64).mean(0), rtol=56 * 2.0 ** -51, atol=0)
    assert all(np.array_equal(a[keep], b[keep]) and np.isnan(a[~keep]).all()
               for a, b in zip(s.maps, maps))
    # an explicit truth and the standardised field
    s2 = xval.score(ysim, rng=np.random.default_rng(7))
    assert np.array_equal(s2.rows, s.rows, equal_nan=True) and np.array_equal(s2.cols, s.cols)
    ms = xval.summary(0.025, std=True, rng=np.random.default_rng(7))
    ss = xval.score(std=True, rng=np.random.default_rng(7))
    y_std = xval.model.data.sim_data.y_std.cpu().numpy()
    assert_sums_match(ss.rows[keep], ss.cols, score_sums(*[a[keep] for a in ms], y_std[keep]),
                      "xval std")
