"""Test-error scores of an emulated field: the result object of ``EmulatorPrediction.score()``.

The sums come from one pass over w and K (gp_field_score, ``blas.field_score``); this module
turns them into the statistics the reference's assessment drivers write
(``assess_all_models.py:524-552``, ``plot_integrated_RMSE.py:108-116``) and holds the torch
reduction the generic route (more PCs or deeper tails than the kernel takes) applies to stored
maps.  The reference forms these statistics in float32 numpy; here they are fp64 sums of fp64
terms, so the two agree to float32 rounding, not bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from ._capi import SCORE_COL, SCORE_ROW

TABLE_HEADER = ("RMSE,MAPE,Lower quantile,Upper quantile,Integrated confidence interval,"
                "Fraction covered")


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _ratio(num, den):
    """num / den with 0 / 0 = NaN and no warning (np.nanmean of nothing)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(num, dtype=np.float64) / np.asarray(den, dtype=np.float64)


class FieldScore:
    """Scores of m predicted fields of ny nodes against a truth.

    ``rows`` (m, 8) and ``cols`` (ny, 4, or None) are the raw sums in the order of
    ``_capi.SCORE_ROW`` / ``SCORE_COL`` (numpy, or device tensors with ``to_host=False``);
    ``maps`` the (mean, lower, upper) arrays when they were asked for.  Everything else is derived
    on the host in fp64; a statistic over no valid element is NaN.
    """

    def __init__(self, rows, cols, ny: int, maps=None, n_scored=None):
        self.rows, self.cols, self.ny, self.maps = rows, cols, int(ny), maps
        self._n_scored = None if n_scored is None else int(n_scored)

    @property
    def n_scored(self) -> int:
        """Test points that entered the per-node sums: all m, less those without a prediction
        (NaN sums and zero counts: cross-validation's simulations in no fold)."""
        if self._n_scored is None:
            self._n_scored = int(np.count_nonzero(~np.isnan(self._r("lo"))))
        return self._n_scored

    def _r(self, name):
        return _host(self.rows)[:, SCORE_ROW[name]]

    def _c(self, name):
        if self.cols is None:
            raise ValueError("the per-node sums were not computed (score(..., cols=False))")
        return _host(self.cols)[:, SCORE_COL[name]]

    # ---- raw counts
    @property
    def n_valid(self):
        """(m,) elements with a truth (not NaN)."""
        return self._r("valid")

    @property
    def n_mape(self):
        """(m,) valid elements at or above the MAPE floor."""
        return self._r("ape_n")

    @property
    def n_covered(self):
        """(m,) valid elements inside [lower, upper]."""
        return self._r("covered")

    @property
    def node_n_valid(self):
        return self._c("valid")

    @property
    def node_n_covered(self):
        return self._c("covered")

    # ---- per test point (m,)
    @property
    def rmse(self):
        return np.sqrt(_ratio(self._r("sqerr"), self.n_valid))

    @property
    def mape(self):
        return _ratio(self._r("ape"), self.n_mape)

    @property
    def mean(self):
        """Mean of the predicted mean field over the nodes."""
        return _ratio(self._r("mean"), self.ny)

    @property
    def lower(self):
        return _ratio(self._r("lo"), self.ny)

    @property
    def upper(self):
        return _ratio(self._r("hi"), self.ny)

    @property
    def width(self):
        """Mean band width over the nodes: np.mean(upper - lower), the integrand of the
        reference's integrated confidence interval (assess_all_models.py:521)."""
        return _ratio(self._r("hi") - self._r("lo"), self.ny)

    @property
    def frac_covered(self):
        return _ratio(self.n_covered, self.n_valid)

    # ---- per node (ny,)
    @property
    def node_rmse(self):
        return np.sqrt(_ratio(self._c("sqerr"), self.node_n_valid))

    @property
    def node_coverage(self):
        return _ratio(self.node_n_covered, self.node_n_valid)

    @property
    def node_width(self):
        """Mean band width over the scored points (n_scored of them)."""
        return _ratio(self._c("width"), self.n_scored)

    @property
    def total_rmse(self) -> float:
        """RMSE over every valid element of every point."""
        return float(np.sqrt(_ratio(np.nansum(self._r("sqerr")), self.n_valid.sum())))

    def table(self, integrated_ci=np.nan) -> np.ndarray:
        """(m, 6) in the column order of the reference's performance CSV (TABLE_HEADER)."""
        m = _host(self.rows).shape[0]
        return np.array([self.rmse, self.mape, self.lower, self.upper,
                         float(integrated_ci) * np.ones(m), self.frac_covered]).T


def rows_without_prediction(rows: torch.Tensor, keep: torch.Tensor, m: int) -> torch.Tensor:
    """The (m, 8) sums of a prediction of which only the points ``keep`` (bool, m) were scored:
    the other rows get NaN sums and zero counts."""
    full = torch.full((m, 8), float("nan"), dtype=rows.dtype, device=rows.device)
    for nm in ("valid", "ape_n", "covered"):
        full[:, SCORE_ROW[nm]] = 0.0
    full[keep] = rows
    return full


def sums_from_maps(mean: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, Y, mape_floor: float,
                   cols: bool = True):
    """(rows, cols) of gp_field_score from stored (m, ny) maps with torch on their device: the
    same fp64 terms (every operation its own kernel, so nothing is contracted), summed in torch's
    order."""
    f64 = torch.float64
    mu, l, h = mean.to(f64), lo.to(f64), hi.to(f64)
    m, ny = mu.shape
    rows = torch.zeros((m, 8), dtype=f64, device=mu.device)
    colt = torch.zeros((ny, 4), dtype=f64, device=mu.device) if cols else None
    rows[:, SCORE_ROW["lo"]] = l.sum(1)
    rows[:, SCORE_ROW["hi"]] = h.sum(1)
    rows[:, SCORE_ROW["mean"]] = mu.sum(1)
    if colt is not None:
        colt[:, SCORE_COL["width"]] = (h - l).sum(0)
    if Y is None:
        return rows, colt
    y = Y.to(f64)
    valid = ~torch.isnan(y)
    r = mu - y
    zero = torch.zeros((), dtype=f64, device=mu.device)
    sq = torch.where(valid, r * r, zero)
    cnt = valid & ~(y < mape_floor)
    ape = torch.where(cnt, (r / y).abs(), zero)
    cov = valid & (l <= y) & (y <= h)
    rows[:, SCORE_ROW["sqerr"]] = sq.sum(1)
    rows[:, SCORE_ROW["valid"]] = valid.sum(1).to(f64)
    rows[:, SCORE_ROW["ape"]] = ape.sum(1)
    rows[:, SCORE_ROW["ape_n"]] = cnt.sum(1).to(f64)
    rows[:, SCORE_ROW["covered"]] = cov.sum(1).to(f64)
    if colt is not None:
        colt[:, SCORE_COL["sqerr"]] = sq.sum(0)
        colt[:, SCORE_COL["valid"]] = valid.sum(0).to(f64)
        colt[:, SCORE_COL["covered"]] = cov.sum(0).to(f64)
    return rows, colt
