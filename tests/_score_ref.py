"""numpy reference of gp_field_score's sums, written from the formulas in include/gpfit.h.

``score_sums(mean, lo, hi, Y, mape_floor)`` takes the *stored* (m, ncols) maps (float32 or
float64: they are widened to fp64 first, as the kernel widens what it would store) and the truth
``Y`` (float32 / float64, NaN = no truth, or None) and returns ``rows`` (m, 8), ``cols``
(ncols, 4) and, for the tolerance of a differently ordered fp64 sum, the sums of the terms'
absolute values in the same two shapes (zero in the count columns).
"""
import numpy as np

ROW = {"sqerr": 0, "valid": 1, "ape": 2, "ape_n": 3, "lo": 4, "hi": 5, "covered": 6, "mean": 7}
COL = {"sqerr": 0, "valid": 1, "covered": 2, "width": 3}
ROW_COUNTS = (ROW["valid"], ROW["ape_n"], ROW["covered"])
COL_COUNTS = (COL["valid"], COL["covered"])
EPS = 2.0 ** -52


def score_sums(mean, lo, hi, Y=None, mape_floor=-np.inf):
    mu = np.asarray(mean).astype(np.float64)
    l = np.asarray(lo).astype(np.float64)
    h = np.asarray(hi).astype(np.float64)
    m, n = mu.shape
    rows, rabs = np.zeros((m, 8)), np.zeros((m, 8))
    cols, cabs = np.zeros((n, 4)), np.zeros((n, 4))
    for k, a in ((ROW["lo"], l), (ROW["hi"], h), (ROW["mean"], mu)):
        rows[:, k] = a.sum(1)
        rabs[:, k] = np.abs(a).sum(1)
    w = h - l
    cols[:, COL["width"]] = w.sum(0)
    cabs[:, COL["width"]] = np.abs(w).sum(0)
    if Y is None:
        return rows, cols, rabs, cabs
    y = np.asarray(Y).astype(np.float64)
    valid = ~np.isnan(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = mu - y
        sq = np.where(valid, r * r, 0.0)
        counted = valid & ~(y < mape_floor)
        ape = np.where(counted, np.abs(r / y), 0.0)
        covered = valid & (l <= y) & (y <= h)
    rows[:, ROW["sqerr"]] = rabs[:, ROW["sqerr"]] = sq.sum(1)
    rows[:, ROW["valid"]] = valid.sum(1)
    rows[:, ROW["ape"]] = rabs[:, ROW["ape"]] = ape.sum(1)
    rows[:, ROW["ape_n"]] = counted.sum(1)
    rows[:, ROW["covered"]] = covered.sum(1)
    cols[:, COL["sqerr"]] = cabs[:, COL["sqerr"]] = sq.sum(0)
    cols[:, COL["valid"]] = valid.sum(0)
    cols[:, COL["covered"]] = covered.sum(0)
    return rows, cols, rabs, cabs


def assert_sums_match(got_rows, got_cols, ref, label=""):
    """Counts exactly; every sum within N * 2^-52 * sum|terms|: two orderings of the same N fp64
    terms, each off the exact sum by at most (N - 1) 2^-53 sum|terms| to first order."""
    rows, cols, rabs, cabs = ref
    m, n = rows.shape[0], cols.shape[0]
    got_rows, got_cols = np.asarray(got_rows), None if got_cols is None else np.asarray(got_cols)
    assert got_rows.shape == rows.shape, (label, got_rows.shape)
    for k in range(8):
        if k in ROW_COUNTS:
            assert np.array_equal(got_rows[:, k], rows[:, k]), (label, "row count", k)
        else:
            tol = n * EPS * rabs[:, k]
            err = np.abs(got_rows[:, k] - rows[:, k])
            assert np.all(err <= tol), (label, "row sum", k, err.max(), tol.max())
    if got_cols is None:
        return
    assert got_cols.shape == cols.shape, (label, got_cols.shape)
    for k in range(4):
        if k in COL_COUNTS:
            assert np.array_equal(got_cols[:, k], cols[:, k]), (label, "col count", k)
        else:
            tol = m * EPS * cabs[:, k]
            err = np.abs(got_cols[:, k] - cols[:, k])
            assert np.all(err <= tol), (label, "col sum", k, err.max(), tol.max())
