"""PCA truncation error on the GPU: the architecture study's RMSE-per-rank curve in one pass.

Reference: ``experiments/synthetic/analysis/plot_PC_RMSE.py:25-46,84-108`` rebuilds the rank-k
field ``U_k S_k Vh_k`` for each of 26 truncation ranks and takes
``||y_sim - y_mean - y_sd (U S V)||_F / sqrt(size)`` of every one;
``include_trunc_error.py:41-49`` takes ``np.var`` of the same kind of residual.  Here the residual
sums of every rank come from one ``gp_pca_trunc`` call (one fp64 MFMA chain over the PCs, the
ensemble and the basis read once, no (n, ny) array stored):

  * :func:`truncation_error` -- drop-in for ``compute_truncation_error`` (a float), and with
    ``ranks`` the whole curve;
  * :func:`truncation_curve` -- the loop body of ``plot_PC_RMSE.py:84-108``: statistics,
    standardisation, ``randomized_svd``, the curve and ``cvar``;
  * :func:`truncation_variance` -- ``include_trunc_error.py:42-47``.

numpy inputs give numpy results, device tensors give device tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import blas
from .blas import CM, gemm
from .kernels import F64
from .svd import _device, _to_device, randomized_svd


@dataclass
class TruncationCurve:
    """Residual statistics of the PCA truncation at each of ``ranks`` (all of length R):
    ``sse`` = sum e^2, ``sum`` = sum e, ``rmse`` = sqrt(sse / (n ny)) (the reference's Frobenius
    RMSE), ``var`` = np.var(e) = sse / N - (sum / N)^2, ``node_rmse`` (R, ny) = sqrt(sum_i e^2 / n)
    when asked for.  :func:`truncation_curve` adds the factors it used (``U``, ``S``, ``Vh``) and
    ``cvar`` = cumsum(S^2) / sum(S^2).

    ``var`` is the one-pass form of the two sums gp_pca_trunc returns, so it cancels when the
    residual's mean is large against its spread: with A = sse / N, B = sum / N and u = 2^-53 its
    error is bounded by the two sums' own errors (|dsse| + 2 |B| |dsum|) / N plus
    u (A + 3 B^2 + |A - B^2|), about u (A + 3 B^2) / (A - B^2) relative -- (B / spread)^2 units in
    the last place, where a two-pass np.var of the stored residual keeps a few.  Measured on an
    MI355X with a mean of 1e4 spreads: 2.7e6 times the two-pass error, under 1 % of that bound
    (tests/_mp_field_ref.py ``one_pass_var_term``).  sse has lost the
    information by then, so no arithmetic on the two sums restores it; a residual whose mean
    matters should be centred first (the reference's residuals are: mu is the column mean)."""

    ranks: np.ndarray
    sse: object
    sum: object
    rmse: object
    var: object
    node_rmse: object = None
    U: object = None
    S: object = None
    Vh: object = None
    cvar: object = None


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    """As stored when row-major with a usable row stride, else a contiguous copy."""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and \
            (t.shape[0] <= 1 or t.stride(0) >= max(t.shape[1], 1)):
        return t
    return t.contiguous()


def _vector(v, ny, dev):
    """y_mean / y_sd as a contiguous fp64 device vector of ny values (scalars broadcast)."""
    t = v.to(device=dev, dtype=F64) if torch.is_tensor(v) else \
        torch.as_tensor(np.asarray(v, dtype=np.float64), device=dev)
    return t.reshape(-1).expand(ny).contiguous() if t.numel() == 1 else t.reshape(-1).contiguous()


def _curve(Y, C, V, mu, sd, ranks, node, as_numpy):
    """The kernel call behind the three entry points: ranks above C's columns count as full rank
    (numpy's clamping slices), repeated and unsorted ranks are computed once and handed out."""
    n, ny = Y.shape
    p = C.shape[1]
    want = np.asarray(ranks).reshape(-1)
    if want.size == 0 or not np.all(want == want.astype(np.int64)) or want.min() < 0:
        raise ValueError(f"truncation ranks must be integers >= 0, got {list(want)}")
    want = want.astype(np.int64)
    eff, inv = np.unique(np.minimum(want, p), return_inverse=True)
    tot, nod = blas.pca_trunc(Y, C, V, eff.tolist(), mu=mu, sd=sd, node=node)
    idx = torch.as_tensor(inv.reshape(-1), device=tot.device)
    tot = tot[idx]
    N = float(n) * float(ny)
    sse, sm = tot[:, 0], tot[:, 1]
    out = TruncationCurve(ranks=want, sse=sse, sum=sm, rmse=torch.sqrt(sse / N),
                          var=sse / N - (sm / N) ** 2,
                          node_rmse=torch.sqrt(nod[idx] / n) if node else None)
    if as_numpy:
        for nm in ("sse", "sum", "rmse", "var", "node_rmse"):
            t = getattr(out, nm)
            setattr(out, nm, t.cpu().numpy() if t is not None else None)
    return out


def truncation_error(usv, y_mean, y_sd, y_sim, ranks=None, node=False, device=None):
    """``compute_truncation_error(usv, y_mean, y_sd, y_sim)`` (plot_PC_RMSE.py:25-46): the RMSE of
    ``y_sim - y_mean - y_sd (U S V)`` in physical units, as a float.  ``S`` is a vector or the
    reference's ``np.diag`` matrix; ``y_sim`` (float32 or float64) is read as stored.

    With ``ranks`` the factors are truncated to each rank in turn (``U[:, :k]``, ``S[:k]``,
    ``V[:k]``; a rank above ``U.shape[1]`` is the full rank) and a :class:`TruncationCurve` is
    returned instead, with ``node_rmse`` when ``node``."""
    U, S, V = usv
    as_numpy = not torch.is_tensor(y_sim)
    dev = _device(device if as_numpy else (device or y_sim.device))
    Y = _rowmajor(_to_device(y_sim, dev))
    if Y.dim() != 2:
        raise ValueError("truncation_error: y_sim must be (simulations, nodes)")
    n, ny = Y.shape
    Ut = _to_device(U, dev).to(F64)
    St = _to_device(S, dev).to(F64)
    Vt = _rowmajor(_to_device(V, dev).to(F64))
    if St.dim() == 2:
        if St.shape[0] != St.shape[1]:
            raise ValueError(f"truncation_error: S {tuple(St.shape)} is neither a vector nor square")
        if Ut.dim() != 2 or Ut.shape[1] != St.shape[0]:
            raise ValueError(f"truncation_error: U {tuple(Ut.shape)} and S {tuple(St.shape)} "
                             "do not fit")
        # the reference's U @ S with S = np.diag(...) (or any square S): (U S)^T = S^T U^T
        Ut = gemm(False, False, CM.of_rowmajor(St), CM.of_rowmajor(Ut)).rowmajor_T()
    elif St.dim() == 1:
        Ut = Ut * St[None, :]
    else:
        raise ValueError("truncation_error: S must be a vector or a square matrix")
    if Ut.dim() != 2 or Vt.dim() != 2 or Ut.shape[0] != n or Vt.shape != (Ut.shape[1], ny):
        raise ValueError(f"truncation_error: U {tuple(Ut.shape)}, V {tuple(Vt.shape)} do not fit "
                         f"y_sim {tuple(Y.shape)}")
    C = Ut.contiguous()
    mu, sd = _vector(y_mean, ny, dev), _vector(y_sd, ny, dev)
    if mu.numel() != ny or sd.numel() != ny:
        raise ValueError(f"truncation_error: y_mean / y_sd need {ny} values")
    single = ranks is None
    out = _curve(Y, C, Vt, mu, sd, [C.shape[1]] if single else ranks, node and not single,
                 as_numpy)
    return float(out.rmse[0]) if single else out


def truncation_curve(y_sim, ranks, pmax=100, k=0, q=1, sd_floor=1e-6, omega=None, node=False,
                     device=None):
    """The body of plot_PC_RMSE.py:84-108 for one ensemble ``y_sim`` (n, ny): mean and ddof=1
    standard deviation floored at ``sd_floor`` (gp_sim_stats), ``y_std`` (gp_standardize),
    ``randomized_svd(y_std, min(pmax, n), k, q)`` (``omega`` overrides its test matrix) and the
    RMSE in physical units of the truncation at every rank of ``ranks`` from one gp_pca_trunc.
    Returns a :class:`TruncationCurve` with ``U``, ``S``, ``Vh`` as used and
    ``cvar = cumsum(S^2) / sum(S^2)``."""
    as_numpy = not torch.is_tensor(y_sim)
    dev = _device(device if as_numpy else (device or y_sim.device))
    Y = _rowmajor(_to_device(y_sim, dev))
    if Y.dim() != 2:
        raise ValueError("truncation_curve: y_sim must be (simulations, nodes)")
    n, ny = Y.shape
    Y64 = Y.to(F64).contiguous()         # the statistics kernels read fp64 (EmulatorData's y_dev)
    mu, sd = blas.sim_stats(Y64, sd_floor)
    ld = (ny + 15) // 16 * 16            # 16-B aligned rows, as EmulatorData.standardize_y pads
    y_std = blas.standardize(Y64, mu, sd,
                             out=torch.empty((n, ld), dtype=F64, device=dev)[:, :ny])
    del Y64
    U, S, Vh = randomized_svd(y_std, min(pmax, n), k=k, q=q, omega=omega)
    del y_std
    C = (U * S[None, :]).contiguous()
    out = _curve(Y, C, Vh, mu, sd, ranks, node, as_numpy)
    S2 = S * S
    cvar = torch.cumsum(S2, 0) / torch.sum(S2)
    conv = (lambda t: t.cpu().numpy()) if as_numpy else (lambda t: t)     # noqa: E731
    out.U, out.S, out.Vh, out.cvar = conv(U), conv(S), conv(Vh), conv(cvar)
    return out


def truncation_variance(y_sim, K, device=None):
    """``np.var(y_sim - y_sim Kn^T Kn)`` with ``Kn`` = the rows of ``K`` scaled to unit length
    (include_trunc_error.py:42-47), as a float: ``C = y_sim Kn^T`` by the tall-skinny GEMM, then
    one gp_pca_trunc at full rank with mu = 0, sd = 1."""
    as_numpy = not torch.is_tensor(y_sim)
    dev = _device(device if as_numpy else (device or y_sim.device))
    Y = _rowmajor(_to_device(y_sim, dev))
    Kt = _to_device(K, dev).to(F64)
    if Y.dim() != 2 or Kt.dim() != 2 or Kt.shape[1] != Y.shape[1]:
        raise ValueError(f"truncation_variance: y_sim {tuple(Y.shape)} and K {tuple(Kt.shape)} "
                         "need one column per node")
    Kn = (Kt / torch.linalg.norm(Kt, dim=1, keepdim=True)).contiguous()
    # (P x n) = Kn y_sim^T, column-major: its row-major view is C = y_sim Kn^T (n x P)
    Ct = gemm(True, False, CM.of_rowmajor(Kn), CM.of_rowmajor(Y))
    C = Ct.rowmajor_T()
    out = _curve(Y, C, Kn, None, None, [Kn.shape[0]], False, as_numpy)
    return float(out.var[0])
