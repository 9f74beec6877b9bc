"""CPU: the numpy reference of the score sums (tests/_score_ref.py) against a literal evaluation
of the reference's expressions (assess_all_models.py:524-537, plot_integrated_RMSE.py:113), and
the derivations of gladsgp_amd.score.FieldScore from hand-made sums.
"""
import numpy as np
import pytest

from _score_ref import COL, ROW, score_sums


def _maps(m=7, n=211, seed=0, nan=True):
    rng = np.random.default_rng(seed)
    mean = 3.0 + rng.standard_normal((m, n))
    lo = mean - rng.uniform(0.1, 1.0, (m, n))
    hi = mean + rng.uniform(0.1, 1.0, (m, n))
    y = mean + 0.6 * rng.standard_normal((m, n))
    y[0, :5] = lo[0, :5]                      # on the bounds: inclusive
    y[1, :5] = hi[1, :5]
    if nan:
        y[rng.random((m, n)) < 0.05] = np.nan
    return mean, lo, hi, y


def test_reference_matches_the_literal_expressions():
    """No NaN in the truth: the sums give exactly the reference's per-point statistics up to the
    rounding of the final division (the same fp64 terms, numpy's own row sums on both sides)."""
    mean, lo, hi, y = _maps(nan=False)
    m, n = y.shape
    lq = np.quantile(y, 0.1)
    rows, cols, _, _ = score_sums(mean, lo, hi, y, mape_floor=lq)
    # the statistics the issue names, each evaluated literally with numpy on the whole arrays:
    # sqrt(mean(resid^2, 1)), nanmean of |resid / y| masked below the floor, the fraction of
    # l <= y <= h, the row means of both bounds
    pred_resid = mean - y
    pred_rmse = np.sqrt(np.mean(pred_resid ** 2, axis=1))
    inner_mape = np.abs(pred_resid / y)
    inner_mape[y < lq] = np.nan
    pred_mape = np.nanmean(inner_mape, axis=1)
    is_covered = np.logical_and(y >= lo, y <= hi)
    frac_covered = is_covered.sum(axis=1) / is_covered.shape[1]
    pred_lq = np.mean(lo, axis=1)
    pred_uq = np.mean(hi, axis=1)
    rt = 4 * 2.0 ** -52
    assert np.all(rows[:, ROW["valid"]] == n)
    assert np.allclose(np.sqrt(rows[:, ROW["sqerr"]] / n), pred_rmse, rtol=rt, atol=0)
    assert np.allclose(rows[:, ROW["ape"]] / rows[:, ROW["ape_n"]], pred_mape, rtol=n * rt, atol=0)
    assert np.array_equal(rows[:, ROW["ape_n"]], (~(y < lq)).sum(1))
    assert np.array_equal(rows[:, ROW["covered"]] / n, frac_covered)
    assert np.allclose(rows[:, ROW["lo"]] / n, pred_lq, rtol=rt, atol=0)
    assert np.allclose(rows[:, ROW["hi"]] / n, pred_uq, rtol=rt, atol=0)
    assert np.allclose(rows[:, ROW["mean"]] / n, mean.mean(1), rtol=rt, atol=0)
    # the bounds are inclusive: the planted elements are covered
    assert is_covered[0, :5].all() and is_covered[1, :5].all()
    # per node: plot_integrated_RMSE.py:113 with one time step, and the mean band width
    assert np.allclose(np.sqrt(cols[:, COL["sqerr"]] / m),
                       np.sqrt(np.nanmean(pred_resid ** 2, axis=0)), rtol=rt, atol=0)
    assert np.array_equal(cols[:, COL["covered"]], is_covered.sum(0))
    assert np.allclose(cols[:, COL["width"]] / m, np.mean(hi - lo, axis=0), rtol=m * rt, atol=0)


def test_reference_with_missing_truth():
    """NaN in the truth: nanmean semantics; float32 maps are widened, not re-rounded; Y = None
    leaves the prediction-only sums; a NaN floor compares false (counts every valid element),
    +inf counts none."""
    mean, lo, hi, y = _maps(seed=3)
    y[4] = np.nan                                            # a row without truth
    rows, cols, rabs, cabs = score_sums(mean, lo, hi, y, mape_floor=2.5)
    resid = mean - y
    want = np.full(len(y), np.nan)
    want[np.arange(len(y)) != 4] = np.nanmean(np.delete(resid, 4, 0) ** 2, axis=1)
    ok = rows[:, ROW["valid"]] > 0
    assert not ok[4] and ok.sum() == len(ok) - 1
    assert np.allclose(rows[ok, ROW["sqerr"]] / rows[ok, ROW["valid"]], want[ok], rtol=1e-14)
    assert rows[4, ROW["sqerr"]] == 0 and rows[4, ROW["covered"]] == 0
    assert np.array_equal(cols[:, COL["valid"]], (~np.isnan(y)).sum(0))
    assert np.all(rows[:, ROW["ape_n"]] <= rows[:, ROW["valid"]])
    sums = [ROW[k] for k in ("sqerr", "ape", "lo", "hi", "mean")]
    assert np.all(rabs[:, sums] >= np.abs(rows[:, sums]) * (1 - 1e-13))
    assert np.all(rabs[:, [ROW["valid"], ROW["ape_n"], ROW["covered"]]] == 0)

    r32 = score_sums(mean.astype(np.float32), lo.astype(np.float32), hi.astype(np.float32), y)[0]
    r64 = score_sums(mean.astype(np.float32).astype(np.float64),
                     lo.astype(np.float32).astype(np.float64),
                     hi.astype(np.float32).astype(np.float64), y)[0]
    assert np.array_equal(r32, r64)

    r0, c0, _, _ = score_sums(mean, lo, hi, None)
    for k in ("sqerr", "valid", "ape", "ape_n", "covered"):
        assert np.all(r0[:, ROW[k]] == 0)
    assert np.array_equal(r0[:, ROW["lo"]], rows[:, ROW["lo"]])
    assert np.array_equal(c0[:, COL["width"]], cols[:, COL["width"]])

    r_all = score_sums(mean, lo, hi, y, mape_floor=-np.inf)[0]
    r_nan = score_sums(mean, lo, hi, y, mape_floor=np.nan)[0]
    r_none = score_sums(mean, lo, hi, y, mape_floor=np.inf)[0]
    assert np.array_equal(r_all[:, ROW["ape_n"]], r_all[:, ROW["valid"]])
    assert np.array_equal(r_nan, r_all)
    assert np.all(r_none[:, ROW["ape_n"]] == 0) and np.all(r_none[:, ROW["ape"]] == 0)


def _hand_made():
    rows = np.zeros((3, 8))
    #            sqerr valid ape  ape_n  lo    hi   covered mean
    rows[0] = [8.0, 2.0, 0.5, 1.0, 4.0, 12.0, 1.0, 8.0]
    rows[1] = [0.0, 0.0, 0.0, 0.0, 2.0, 6.0, 0.0, 4.0]       # no truth on this point
    rows[2] = [18.0, 4.0, 0.0, 0.0, 0.0, 8.0, 4.0, 4.0]      # nothing above the MAPE floor
    cols = np.array([[2.0, 2.0, 1.0, 3.0], [0.0, 0.0, 0.0, 6.0], [16.0, 1.0, 1.0, 9.0],
                     [8.0, 3.0, 3.0, 0.0]])
    return rows, cols


def test_field_score_derivations():
    from gladsgp_amd.score import TABLE_HEADER, FieldScore
    rows, cols = _hand_made()
    s = FieldScore(rows, cols, ny=4)
    assert np.array_equal(s.rmse, [2.0, np.nan, np.sqrt(4.5)], equal_nan=True)
    assert np.array_equal(s.mape, [0.5, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(s.lower, [1.0, 0.5, 0.0])
    assert np.array_equal(s.upper, [3.0, 1.5, 2.0])
    assert np.array_equal(s.mean, [2.0, 1.0, 1.0])
    assert np.array_equal(s.width, [2.0, 1.0, 2.0])
    assert np.array_equal(s.frac_covered, [0.5, np.nan, 1.0], equal_nan=True)
    assert np.array_equal(s.n_valid, [2, 0, 4]) and np.array_equal(s.n_mape, [1, 0, 0])
    assert np.array_equal(s.n_covered, [1, 0, 4])
    assert np.array_equal(s.node_rmse, [1.0, np.nan, 4.0, np.sqrt(8 / 3)], equal_nan=True)
    assert np.array_equal(s.node_coverage, [0.5, np.nan, 1.0, 1.0], equal_nan=True)
    assert np.array_equal(s.node_width, [1.0, 2.0, 3.0, 0.0])
    assert np.array_equal(s.node_n_valid, [2, 0, 1, 3])
    assert s.total_rmse == np.sqrt(26.0 / 6.0)
    t = s.table(integrated_ci=1.25)
    assert t.shape == (3, 6)
    assert TABLE_HEADER.split(",") == ["RMSE", "MAPE", "Lower quantile", "Upper quantile",
                                       "Integrated confidence interval", "Fraction covered"]
    for k, col in enumerate((s.rmse, s.mape, s.lower, s.upper, np.full(3, 1.25), s.frac_covered)):
        assert np.array_equal(t[:, k], col, equal_nan=True), k
    assert np.isnan(FieldScore(rows, None, ny=4).table()[:, 4]).all()
    with pytest.raises(ValueError, match="per-node"):
        FieldScore(rows, None, ny=4).node_rmse


def test_field_score_without_any_truth_and_nan_rows():
    """Zero counts everywhere give NaN error statistics and leave the band statistics; a point
    without a prediction (NaN sums, zero counts) does not poison total_rmse."""
    import torch
    from gladsgp_amd.score import FieldScore, rows_without_prediction
    rows, cols = _hand_made()
    rows[:, [0, 1, 2, 3, 6]] = 0.0
    cols[:, :3] = 0.0
    s = FieldScore(rows, cols, ny=4)
    assert np.isnan(s.rmse).all() and np.isnan(s.mape).all() and np.isnan(s.frac_covered).all()
    assert np.isnan(s.node_rmse).all() and np.isnan(s.total_rmse)
    assert np.array_equal(s.width, [2.0, 1.0, 2.0])

    rows, cols = _hand_made()
    keep = torch.tensor([True, False, True])
    full = rows_without_prediction(torch.as_tensor(rows[[0, 2]]), keep, 3).numpy()
    assert np.array_equal(full[[0, 2]], rows[[0, 2]])
    assert np.array_equal(full[1, [1, 3, 6]], [0, 0, 0]) and np.isnan(full[1, [0, 2, 4, 5, 7]]).all()
    s = FieldScore(full, cols, ny=4)
    assert np.isnan(s.rmse[1]) and np.isnan(s.lower[1]) and s.n_valid[1] == 0
    # the per-node mean width is over the two scored points, not over all three rows
    assert s.n_scored == 2 and np.array_equal(s.node_width, cols[:, 3] / 2)
    assert FieldScore(full, cols, ny=4, n_scored=2).n_scored == 2
    assert FieldScore(rows, cols, ny=4).n_scored == 3
    assert s.total_rmse == np.sqrt(26.0 / 6.0)


def test_sums_from_maps_is_the_reference():
    """The torch reduction of the generic route (CPU tensors here) gives the reference's counts
    exactly and its sums to the ordering tolerance."""
    import torch
    from _score_ref import assert_sums_match
    from gladsgp_amd.score import sums_from_maps
    mean, lo, hi, y = _maps(seed=5)
    y[2] = np.nan
    for dt in (np.float64, np.float32):
        maps = [a.astype(dt) for a in (mean, lo, hi)]
        for Y, floor in ((y, 2.5), (y.astype(np.float32), -np.inf), (None, 0.0), (y, np.nan)):
            rows, cols = sums_from_maps(*[torch.as_tensor(a) for a in maps],
                                        None if Y is None else torch.as_tensor(Y), floor)
            assert_sums_match(rows.numpy(), cols.numpy(), score_sums(*maps, Y, floor),
                              f"{dt.__name__} floor={floor}")
