"""Sobol' sensitivity indices with bootstrap confidence intervals on the device.

The reference's ``src/utils.py:27-256`` (``saltelli_sensitivity_indices`` /
``PCA_saltelli_sensitivity_indices``, called by ``sensitivity_indices.py:96,214``) computes the
Saltelli estimators once and then hands a Python statistic to four ``scipy.stats.bootstrap`` calls
(9,999 resamples each, BCa).  Here every replicate of the statistic -- the point estimate, the
resamples and the jackknife -- is one ``gp_sobol_replicates`` launch (``csrc/sobol.hip``), and the
interval arithmetic (scipy's BCa / percentile rules) runs on the device with torch.

One documented difference: the reference draws four independent sets of resamples, one per
statistic, and recomputes the same sums in each; here first-order, total and both general indices
come from ONE common set, so the intervals agree with the reference statistically, not number for
number.

Beside the estimators stands what they estimate: the function analysed is the emulator's posterior
mean, a sum of products over the input dimensions under the ARD kernel, so its Sobol' indices
under uniform inputs have a closed form (``gp_sobol_exact``, ``csrc/sobolx.hip``).
:func:`exact_indices` returns them with no design, no sampling error and no bootstrap, and, per
posterior sample, their posterior spread.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi
from .kernels import F64, _stream

IDENTITY, INDEX, PHILOX, JACKKNIFE = 0, 1, 2, 3      # GPFIT_SOBOL_*
_MODES = {"identity": IDENTITY, "index": INDEX, "philox": PHILOX, "jackknife": JACKKNIFE}
MAX_POINTS = 1 << 20
MAX_DIM = 32                                         # GPFIT_MAX_DIM

ConfidenceInterval = namedtuple("ConfidenceInterval", ["low", "high"])


# ------------------------------------------------------------------------------------------------
# design
# ------------------------------------------------------------------------------------------------

def saltelli_design(n_dim: int, m: int, seed=None):
    """(A, B), 2^m points each, as the reference draws them (src/utils.py:64-67): one scrambled
    Sobol' sequence in 2 n_dim dimensions, A its last n_dim columns and B its first."""
    from scipy.stats import qmc
    AB = qmc.Sobol(d=2 * int(n_dim), seed=seed).random_base2(m=int(m))
    return AB[:, n_dim:], AB[:, :n_dim]


def saltelli_points(A, B) -> np.ndarray:
    """The ((d + 2) N, d) stack [A; B; AB_0 .. AB_{d-1}], AB_i = B with column i taken from A."""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError(f"saltelli_points: A {A.shape} and B {B.shape} must be equal (N, d)")
    N, d = A.shape
    out = np.empty((d + 2, N, d), dtype=np.result_type(A, B))
    out[0], out[1] = A, B
    for i in range(d):
        out[2 + i] = B
        out[2 + i, :, i] = A[:, i]
    return out.reshape((d + 2) * N, d)


# ------------------------------------------------------------------------------------------------
# the C call
# ------------------------------------------------------------------------------------------------

def lds_points(d: int) -> int:
    """Largest N whose working set gp_sobol_replicates keeps in LDS (gp_sobol_lds_points)."""
    return int(_capi.lib().gp_sobol_lds_points(int(d)))


def sobol_replicates(fA: torch.Tensor, fB: torch.Tensor, fAB: torch.Tensor, mode=IDENTITY,
                     idx: torch.Tensor | None = None, n_draw: int | None = None,
                     R: int | None = None, seed: int = 0, pcvar: torch.Tensor | None = None,
                     clamp: bool = False, offset: int = 0):
    """Saltelli estimators for R replicates of the design rows (gp_sobol_replicates).

    Output-major operands: ``fA`` / ``fB`` (p, N) and ``fAB`` (d, p, N) float64 on one HIP device,
    unit last stride, one common row stride ldf >= N (``fAB.stride(0)`` >= (p - 1) ldf + N).
    ``mode``: IDENTITY (the point estimate, R = 1), INDEX (rows ``idx`` (R, n_draw) int32, unit
    last stride, range-checked on the device), PHILOX (rows drawn on the device from (seed, offset,
    r, k)) or JACKKNIFE (replicate r leaves row r out, R = N).  ``pcvar`` (p,): also the general
    indices.  Returns (first (R, p, d), total (R, p, d), gfirst (R, d) | None, gtotal | None)."""
    nm = "sobol_replicates"
    if isinstance(mode, str):
        if mode.lower() not in _MODES:
            raise ValueError(f"{nm}: unknown mode {mode!r}")
        mode = _MODES[mode.lower()]
    if mode not in (IDENTITY, INDEX, PHILOX, JACKKNIFE):
        raise ValueError(f"{nm}: unknown mode {mode!r}")
    for name, t, nd in (("fA", fA, 2), ("fB", fB, 2), ("fAB", fAB, 3)):
        if not torch.is_tensor(t) or t.dtype != F64 or t.dim() != nd:
            raise ValueError(f"{nm}: {name} must be a {nd}-d float64 tensor")
    p, N = fA.shape
    d = fAB.shape[0]
    dev = fA.device
    if tuple(fB.shape) != (p, N) or tuple(fAB.shape) != (d, p, N):
        raise ValueError(f"{nm}: fA {tuple(fA.shape)}, fB {tuple(fB.shape)} must be (p, N) and "
                         f"fAB {tuple(fAB.shape)} (d, p, N)")
    if fB.device != dev or fAB.device != dev:
        raise ValueError(f"{nm}: fA, fB and fAB must be on one device")
    if not (2 <= N <= MAX_POINTS) or p < 1 or not (1 <= d <= MAX_DIM):
        raise ValueError(f"{nm}: need 2 <= N <= 2^20, p >= 1, 1 <= d <= {MAX_DIM}; got N = {N}, "
                         f"p = {p}, d = {d}")
    if fA.stride(1) != 1 or fB.stride(1) != 1 or fAB.stride(2) != 1:
        raise ValueError(f"{nm}: operands need a unit last stride (strides {fA.stride()}, "
                         f"{fB.stride()}, {fAB.stride()})")
    ldf = fA.stride(0) if p > 1 else N
    if p > 1 and (ldf < N or fB.stride(0) != ldf or fAB.stride(1) != ldf):
        raise ValueError(f"{nm}: fA, fB and fAB must share one row stride ldf >= N (strides "
                         f"{fA.stride()}, {fB.stride()}, {fAB.stride()})")
    tightAB = (p - 1) * ldf + N
    strideAB = fAB.stride(0) if d > 1 else max(fAB.stride(0), tightAB)
    if strideAB < tightAB:
        raise ValueError(f"{nm}: fAB needs an input stride >= (p - 1) ldf + N (strides "
                         f"{fAB.stride()})")
    if mode == INDEX and (not torch.is_tensor(idx) or idx.dtype != torch.int32 or
                          idx.dim() != 2 or idx.device != dev):
        raise ValueError(f"{nm}: idx must be a 2-d int32 tensor on the operands' device")
    if n_draw is None:
        n_draw = N - 1 if mode == JACKKNIFE else (idx.shape[1] if mode == INDEX else N)
    if R is None:
        if mode == PHILOX:
            raise ValueError(f"{nm}: R is required in this mode")
        R = 1 if mode == IDENTITY else N if mode == JACKKNIFE else idx.shape[0]
    n_draw, R = int(n_draw), int(R)
    if n_draw < 1 or R < 0:
        raise ValueError(f"{nm}: need n_draw >= 1 and R >= 0, got {n_draw}, {R}")
    if mode == IDENTITY and (R != 1 or n_draw != N):
        raise ValueError(f"{nm}: IDENTITY needs R = 1 and n_draw = N")
    if mode == JACKKNIFE and (R != N or n_draw != N - 1):
        raise ValueError(f"{nm}: JACKKNIFE needs R = N and n_draw = N - 1")
    ldi = n_draw
    if mode == INDEX:
        if idx.shape[0] < R or idx.shape[1] != n_draw:
            raise ValueError(f"{nm}: idx {tuple(idx.shape)} must be (R, n_draw) = ({R}, {n_draw})")
        if n_draw > 1 and idx.stride(1) != 1:
            raise ValueError(f"{nm}: idx needs a unit last stride")
        ldi = idx.stride(0) if idx.shape[0] > 1 else max(idx.stride(0), n_draw)
        if ldi < n_draw:
            raise ValueError(f"{nm}: idx needs a row stride >= n_draw")
    elif idx is not None:
        raise ValueError(f"{nm}: idx goes with mode INDEX only")
    if pcvar is not None:
        if not torch.is_tensor(pcvar) or pcvar.dtype != F64 or pcvar.device != dev or \
                not pcvar.is_contiguous() or pcvar.numel() != p:
            raise ValueError(f"{nm}: pcvar must be {p} contiguous float64 values on the operands' "
                             "device")
    if dev.type != "cuda":
        raise ValueError(f"{nm}: the operands must be on a HIP device")
    if mode == INDEX and R > 0 and bool(((idx[:R] < 0) | (idx[:R] >= N)).any()):
        raise ValueError(f"{nm}: idx has entries outside [0, {N})")
    first = torch.empty((R, p, d), dtype=F64, device=dev)
    total = torch.empty((R, p, d), dtype=F64, device=dev)
    gfirst = gtotal = None
    if pcvar is not None:
        gfirst = torch.empty((R, d), dtype=F64, device=dev)
        gtotal = torch.empty((R, d), dtype=F64, device=dev)
    if R == 0:
        return first, total, gfirst, gtotal
    mask = (1 << 64) - 1
    _capi.call("gp_sobol_replicates", fA.data_ptr(), fB.data_ptr(), fAB.data_ptr(), ldf, strideAB,
               N, p, d, mode, idx.data_ptr() if mode == INDEX else None, ldi, n_draw, R,
               int(seed) & mask, int(offset) & mask,
               pcvar.data_ptr() if pcvar is not None else None, int(bool(clamp)),
               first.data_ptr(), total.data_ptr(), p * d,
               gfirst.data_ptr() if pcvar is not None else None,
               gtotal.data_ptr() if pcvar is not None else None, d, _stream(dev))
    return first, total, gfirst, gtotal


# ------------------------------------------------------------------------------------------------
# intervals (scipy.stats.bootstrap's rules; replicates along axis 0)
# ------------------------------------------------------------------------------------------------

def _ndtr(x):
    if torch.is_tensor(x):
        return torch.special.ndtr(x)
    from scipy.special import ndtr
    return ndtr(x)


def _ndtri(x):
    if torch.is_tensor(x):
        return torch.special.ndtri(x)
    from scipy.special import ndtri
    return ndtri(x)


def _percentile_each(boot, alpha):
    """np.percentile(boot[:, e], 100 alpha[e]) for every element e (numpy's linear rule and its
    _lerp); NaN where alpha is NaN.  ``boot`` (R, ...), ``alpha`` (...)."""
    tt = torch.is_tensor(boot)
    R = boot.shape[0]
    if tt:
        srt = torch.sort(boot, dim=0).values
        bad = torch.isnan(alpha)
        q = torch.where(bad, torch.zeros_like(alpha), alpha) * 100 / 100
        pos = q * (R - 1)
        j = torch.floor(pos).clamp(0, R - 1)
        t = pos - j
        j = j.to(torch.int64)
        j1 = (j + 1).clamp(max=R - 1)
        a = torch.gather(srt, 0, j.unsqueeze(0)).squeeze(0)
        b = torch.gather(srt, 0, j1.unsqueeze(0)).squeeze(0)
        diff = b - a
        out = torch.where(t >= 0.5, b - diff * (1 - t), a + diff * t)
        out = torch.where(diff == 0, a, out)
        return torch.where(bad, torch.full_like(out, float("nan")), out)
    srt = np.sort(boot, axis=0)
    alpha = np.asarray(alpha, dtype=np.float64)
    bad = np.isnan(alpha)
    q = np.where(bad, 0.0, alpha) * 100 / 100
    pos = q * (R - 1)
    j = np.clip(np.floor(pos), 0, R - 1)
    t = pos - j
    j = j.astype(np.int64)
    j1 = np.minimum(j + 1, R - 1)
    a = np.take_along_axis(srt, j[None], 0)[0]
    b = np.take_along_axis(srt, j1[None], 0)[0]
    diff = b - a
    with np.errstate(invalid="ignore"):
        out = np.where(t >= 0.5, b - diff * (1 - t), a + diff * t)
    out = np.where(diff == 0, a, out)
    return np.where(bad, np.nan, out)


def percentile_interval(boot, confidence_level: float = 0.95):
    """scipy's ``method="percentile"`` interval: the alpha and 1 - alpha percentiles of the
    bootstrap distribution ``boot`` (R, ...), alpha = (1 - confidence_level) / 2."""
    alpha = (1 - confidence_level) / 2
    if torch.is_tensor(boot):
        lo = torch.full(boot.shape[1:], alpha, dtype=boot.dtype, device=boot.device)
    else:
        boot = np.asarray(boot, dtype=np.float64)
        lo = np.full(boot.shape[1:], alpha)
    return ConfidenceInterval(_percentile_each(boot, lo), _percentile_each(boot, 1 - lo))


def bca_interval(theta_hat, boot, jack, confidence_level: float = 0.95):
    """scipy's bias-corrected and accelerated interval (Efron & Tibshirani 14.3, eq. 15.36) from
    the statistic ``theta_hat`` (...), its bootstrap distribution ``boot`` (R, ...) and its n
    jackknife values ``jack`` (n, ...); numpy arrays or torch tensors (one kind for all three).

    z0 = ndtri((#{boot < theta} + #{boot <= theta}) / (2 R)); a = sum (mean - jack_i)^3 /
    (6 (sum (mean - jack_i)^2)^(3/2)); the endpoints are the ndtr(z0 + (z0 + z) / (1 - a (z0 +
    z))) percentiles of ``boot`` for z = -+ ndtri(alpha).  A degenerate distribution gives NaN."""
    alpha = (1 - confidence_level) / 2
    tt = torch.is_tensor(boot)
    if not tt:
        theta_hat = np.asarray(theta_hat, dtype=np.float64)
        boot = np.asarray(boot, dtype=np.float64)
        jack = np.asarray(jack, dtype=np.float64)
    R, n = boot.shape[0], jack.shape[0]
    th = theta_hat[None]
    cnt = (boot < th).sum(0) + (boot <= th).sum(0)
    z0 = _ndtri((cnt.to(boot.dtype) if tt else cnt) / (2 * R))
    # scipy's scaling of the influence values, kept so that the roundings agree
    U = (n - 1) * (jack.mean(0, keepdim=True) - jack if tt else jack.mean(0, keepdims=True) - jack)
    num = (U ** 3).sum(0) / n ** 3
    den = (U ** 2).sum(0) / n ** 2
    if tt:
        a_hat = 1 / 6 * num / den ** 1.5
        z_a = float(torch.special.ndtri(torch.tensor(alpha, dtype=torch.float64)))
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            a_hat = 1 / 6 * num / den ** 1.5
        z_a = float(_ndtri(alpha))
    n1 = z0 + z_a
    n2 = z0 - z_a
    if tt:
        a1 = _ndtr(z0 + n1 / (1 - a_hat * n1))
        a2 = _ndtr(z0 + n2 / (1 - a_hat * n2))
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            a1 = _ndtr(z0 + n1 / (1 - a_hat * n1))
            a2 = _ndtr(z0 + n2 / (1 - a_hat * n2))
    return ConfidenceInterval(_percentile_each(boot, a1), _percentile_each(boot, a2))


# ------------------------------------------------------------------------------------------------
# the analysis
# ------------------------------------------------------------------------------------------------

@dataclass
class BootstrapStatistic:
    """What the driver reads of a scipy ``BootstrapResult``; the distribution has the replicates
    on its LAST axis, as scipy's."""
    confidence_interval: ConfidenceInterval
    bootstrap_distribution: object
    standard_error: object


_STAT_NAMES = ("first_order", "total_index", "general_first_order", "general_total_index")


@dataclass
class SobolResult:
    """Point estimates (``first_order`` / ``total_index`` (p, d), the general pair (d,) or None)
    and, per statistic name, its :class:`BootstrapStatistic` (``result[name]``; empty without
    resampling).  Tensors live on the device; :meth:`numpy` gives a host copy."""
    first_order: object
    total_index: object
    general_first_order: object
    general_total_index: object
    statistics: dict

    def __getitem__(self, name: str) -> BootstrapStatistic:
        return self.statistics[name]

    def numpy(self) -> "SobolResult":
        def h(x):
            return x.cpu().numpy() if torch.is_tensor(x) else x
        st = {k: BootstrapStatistic(ConfidenceInterval(h(v.confidence_interval.low),
                                                       h(v.confidence_interval.high)),
                                    h(v.bootstrap_distribution), h(v.standard_error))
              for k, v in self.statistics.items()}
        return SobolResult(h(self.first_order), h(self.total_index), h(self.general_first_order),
                           h(self.general_total_index), st)


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise ValueError("sobol_indices: no HIP device (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _fresh_seed() -> int:
    lo, hi = np.random.SeedSequence().generate_state(2, dtype=np.uint32)
    return (int(hi) << 32) | int(lo)


def sobol_indices(fA, fB, fAB, pcvar=None, n_resamples: int = 9999,
                  confidence_level: float = 0.95, method: str = "BCa", seed=None, idx=None,
                  device=None) -> SobolResult:
    """Sobol' indices of model outputs ``fA`` / ``fB`` (N, p) and ``fAB`` (d, N, p) (numpy or
    torch; the reference's orientation) with bootstrap intervals, all on the device.

    The point estimate is one IDENTITY call (unclamped, as the reference's); the bootstrap
    distribution one PHILOX call keyed by ``seed`` (or INDEX with the rows ``idx`` (R, N)); BCa
    adds one JACKKNIFE call.  The resampled statistic clamps V < 0 to 0 as the reference's does,
    so the theta-hat the BCa bias correction compares against is a second, clamped IDENTITY call.
    ``n_resamples = 0``: point estimates only."""
    if method not in ("BCa", "percentile"):
        raise ValueError(f"sobol_indices: method must be 'BCa' or 'percentile', got {method!r}")
    dev = fA.device if torch.is_tensor(fA) else _device(device)

    def dv(x):
        return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(
            device=dev, dtype=F64)
    fA, fB, fAB = dv(fA), dv(fB), dv(fAB)
    if fA.dim() == 1:
        fA, fB, fAB = fA[:, None], fB[:, None], fAB[:, :, None]
    if fA.dim() != 2 or fB.shape != fA.shape or fAB.dim() != 3 or fAB.shape[1:] != fA.shape:
        raise ValueError(f"sobol_indices: fA {tuple(fA.shape)}, fB {tuple(fB.shape)} must be "
                         f"(N, p) and fAB {tuple(fAB.shape)} (d, N, p)")
    N, p = fA.shape
    a = fA.t().contiguous()                              # output-major: the tiny transpose
    b = fB.t().contiguous()
    ab = fAB.transpose(1, 2).contiguous()
    pv = None if pcvar is None else dv(pcvar).reshape(-1).contiguous()
    f0, t0, gf0, gt0 = sobol_replicates(a, b, ab, IDENTITY, pcvar=pv, clamp=False)
    est = {"first_order": f0[0], "total_index": t0[0]}
    if pv is not None:
        est.update(general_first_order=gf0[0], general_total_index=gt0[0])
    stats = {}
    if idx is not None:
        idx = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx).to(
            device=dev, dtype=torch.int32).contiguous()
        n_resamples = idx.shape[0]
    if n_resamples > 0:
        th = sobol_replicates(a, b, ab, IDENTITY, pcvar=pv, clamp=True)
        if idx is not None:
            boot = sobol_replicates(a, b, ab, INDEX, idx=idx, pcvar=pv, clamp=True)
        else:
            seed = _fresh_seed() if seed is None else int(seed)
            boot = sobol_replicates(a, b, ab, PHILOX, R=int(n_resamples), seed=seed, pcvar=pv,
                                    clamp=True)
        jack = sobol_replicates(a, b, ab, JACKKNIFE, pcvar=pv, clamp=True) \
            if method == "BCa" else None
        for k, name in enumerate(_STAT_NAMES):
            if boot[k] is None:
                continue
            if method == "BCa":
                ci = bca_interval(th[k][0], boot[k], jack[k], confidence_level)
            else:
                ci = percentile_interval(boot[k], confidence_level)
            se = torch.std(boot[k], dim=0, unbiased=True) if boot[k].shape[0] > 1 else \
                torch.full_like(boot[k][0], float("nan"))
            stats[name] = BootstrapStatistic(ci, torch.movedim(boot[k], 0, -1), se)
    return SobolResult(est["first_order"], est["total_index"], est.get("general_first_order"),
                       est.get("general_total_index"), stats)


def _evaluate(func, n_dim, m, seed, batched):
    """A, B and the model outputs fA, fB (N, p), fAB (d, N, p), ``func`` called d + 2 times as the
    reference does, or once on the whole stack (``batched``)."""
    A, B = saltelli_design(n_dim, m, seed=seed)
    N = A.shape[0]
    if batched:
        f = np.asarray(func(saltelli_points(A, B)), dtype=np.float64)
        f = f.reshape(n_dim + 2, N, *f.shape[1:])
        return f[0], f[1], f[2:]
    fA = np.asarray(func(A), dtype=np.float64)
    fB = np.asarray(func(B), dtype=np.float64)
    fAB = np.zeros((n_dim,) + fA.shape)
    for ix in range(n_dim):
        C = B.copy()
        C[:, ix] = A[:, ix]
        fAB[ix] = func(C)
    return fA, fB, fAB


def _philox_seed(seed) -> int | None:
    """The resampling key: derived from the design's seed (an int or None; a Generator draws)."""
    if seed is None:
        return None
    if isinstance(seed, (int, np.integer)):
        return int(seed)
    return int(np.random.default_rng(seed).integers(0, 2 ** 63))


def saltelli_sensitivity_indices(func, n_dim, m, bootstrap=True, *, seed=None, n_resamples=9999,
                                 batched=False):
    """Drop-in for the reference's ``utils.saltelli_sensitivity_indices`` (src/utils.py:27-125):
    ``func(x (N, n_dim)) -> (N, p)`` (or (N,)); returns (first_order (p, n_dim), total_index
    (p, n_dim), res) with ``res`` a dict of 'first_order' / 'total_index' bootstrap results
    (``.confidence_interval.low / .high``; 95 % BCa) or None.  ``seed`` fixes the design and the
    resampling; ``batched``: one ``func`` call on :func:`saltelli_points`."""
    fA, fB, fAB = _evaluate(func, int(n_dim), m, seed, batched)
    r = sobol_indices(fA, fB, fAB, None, n_resamples=n_resamples if bootstrap else 0,
                      seed=_philox_seed(seed)).numpy()
    res = {k: r[k] for k in _STAT_NAMES[:2]} if bootstrap else None
    return r.first_order, r.total_index, res


def PCA_saltelli_sensitivity_indices(func, n_dim, m, pcvar, bootstrap=True, *, seed=None,
                                     n_resamples=9999, batched=False):
    """Drop-in for the reference's ``utils.PCA_saltelli_sensitivity_indices``
    (src/utils.py:128-256): returns (first_order (p, n_dim), total_index (p, n_dim),
    gen_first_order (n_dim,), gen_total_index (n_dim,), res), ``res`` a dict with the reference's
    four keys or None."""
    fA, fB, fAB = _evaluate(func, int(n_dim), m, seed, batched)
    r = sobol_indices(fA, fB, fAB, np.asarray(pcvar, dtype=np.float64),
                      n_resamples=n_resamples if bootstrap else 0, seed=_philox_seed(seed)).numpy()
    res = {k: r[k] for k in _STAT_NAMES} if bootstrap else None
    return r.first_order, r.total_index, r.general_first_order, r.general_total_index, res


def emulator_func(model, samples, cast=np.float32, **prediction_kwargs):
    """The driver's ``func`` (sensitivity_indices.py:73-89): x (N, d) -> the mean over the
    posterior samples of the predicted PC weights, one ``EmulatorPrediction`` per call, after the
    reference's float32 cast, as float64 (N, P)."""
    from .emulator import EmulatorPrediction

    def func(x):
        pred = EmulatorPrediction(model=model, samples=samples, t_pred=x, **prediction_kwargs)
        w = pred.w if cast is None else pred.w.astype(cast)
        return np.mean(w, axis=0).astype(np.float64)
    return func


# ------------------------------------------------------------------------------------------------
# the closed form
# ------------------------------------------------------------------------------------------------

def indices_from_moments(E, Q):
    """(mean, variance, first_order, total_index) of the mean function of each group from
    gp_sobol_exact's ``E`` (..., M) and ``Q`` (..., M, M, 2 d + 1): with Eb = mean_a E and
    Qb = mean_ab Q, V = Qb_tot - Eb^2, S_i = (Qb_main_i - Eb^2) / V, T_i = (Qb_tot - Qb_not_i) / V.
    numpy arrays or torch tensors."""
    d = (Q.shape[-1] - 1) // 2
    Eb = E.mean(-1)
    Qb = Q.mean(-2).mean(-2)
    V = Qb[..., 0] - Eb * Eb
    first = (Qb[..., 1:1 + d] - (Eb * Eb)[..., None]) / V[..., None]
    total = (Qb[..., :1] - Qb[..., 1 + d:]) / V[..., None]
    return Eb, V, first, total


@dataclass
class ExactSobolResult:
    """The exact Sobol' indices of the emulator's posterior mean (:func:`exact_indices`).
    ``average="mean"``: ``first_order`` / ``total_index`` (P, d), ``mean`` / ``variance`` (P,), the
    general pair (d,) or None.  ``average="sample"``: the same with a leading axis over the S
    posterior samples.  Tensors live on the device; :meth:`numpy` gives a host copy."""
    first_order: object
    total_index: object
    general_first_order: object
    general_total_index: object
    mean: object
    variance: object
    average: str = "mean"

    @property
    def interaction(self):
        """total_index - first_order: the share of the variance x_i takes part in through
        interactions only."""
        return self.total_index - self.first_order

    def interval(self, confidence_level: float = 0.95) -> dict:
        """Per statistic name the equal-tailed band over the posterior samples
        (``average="sample"`` only): the (1 -+ confidence_level) / 2 quantiles along the S axis
        (numpy's linear rule), as a :class:`ConfidenceInterval`."""
        if self.average != "sample":
            raise ValueError("interval: the band is over the posterior samples; use "
                             "exact_indices(..., average='sample')")
        return {name: percentile_interval(getattr(self, name), confidence_level)
                for name in _STAT_NAMES if getattr(self, name) is not None}

    def numpy(self) -> "ExactSobolResult":
        def h(x):
            return x.cpu().numpy() if torch.is_tensor(x) else x
        return ExactSobolResult(h(self.first_order), h(self.total_index),
                                h(self.general_first_order), h(self.general_total_index),
                                h(self.mean), h(self.variance), self.average)


def exact_indices(model, samples, pcvar=None, average: str = "mean", lo=None, hi=None,
                  budget_bytes: int = 2 << 30, group: int | None = None) -> ExactSobolResult:
    """Sobol' indices of the emulator's posterior mean in closed form (gp_sobol_exact): no design,
    no sampling error, no bootstrap.  The inputs are uniform on the box ``[lo, hi]`` (default the
    unit cube, where the reference's Saltelli design lives).

    ``average="mean"``: the indices of the driver's ``func`` (sensitivity_indices.py:73-89), the
    mean over the posterior samples of the predicted PC weights -- the limit of
    ``PCA_saltelli_sensitivity_indices(emulator_func(model, samples, cast=None), ...)`` as the
    design grows.  ``average="sample"``: the indices of every posterior sample's own mean
    function; :meth:`ExactSobolResult.interval` then gives their posterior spread.  ``pcvar``
    (P,): also the general indices sum_p pcvar_p index_p (utils.py:254-255).

    One difference from the Saltelli path: ``emulator_func`` casts w to float32 per predicted
    point as the driver does; the closed form has no such cast.

    Per group of GPs under ``budget_bytes`` / ``group`` the alpha chain is
    :func:`gladsgp_amd.response.unit_alpha`; then one ``kernels.sobol_exact`` per PC."""
    from . import kernels
    from .emulator import EmulatorModel
    from .response import unit_alpha
    if not isinstance(model, EmulatorModel) or samples is None:
        raise ValueError("exact_indices needs an EmulatorModel and its samples")
    if average not in ("mean", "sample"):
        raise ValueError(f"average: expected 'mean' or 'sample', got {average!r}")
    dev = model.device
    d = model.d
    X = model.data.sim_data.t_dev.contiguous()

    def box(v):
        if v is None:
            return None
        return torch.as_tensor(np.broadcast_to(np.asarray(_host(v), dtype=np.float64),
                                               (d,)).copy(), dtype=F64, device=dev)
    if (lo is None) != (hi is None):
        lo = 0.0 if lo is None else lo
        hi = 1.0 if hi is None else hi
    lo, hi = box(lo), box(hi)
    alpha, beta_u, s_u, S, P = unit_alpha(model, samples, budget_bytes, group)
    # the S samples of a PC consecutive: unit (j, s)
    pm = lambda a: a.reshape(S, P, -1).transpose(0, 1).reshape(P * S, -1).contiguous()  # noqa
    alpha, beta_u, s_u = pm(alpha), pm(beta_u), pm(s_u).reshape(-1)
    M = S if average == "mean" else 1
    E = torch.empty(P * S, dtype=F64, device=dev)
    Q = torch.empty((P * S // M, M, M, 2 * d + 1), dtype=F64, device=dev)
    gp = S // M                                          # groups per PC
    for j in range(P):
        u = slice(j * S, (j + 1) * S)
        kernels.sobol_exact(X, alpha[u], beta_u[u], s_u[u], group=M, lo=lo, hi=hi,
                            out=(E[u], Q[j * gp:(j + 1) * gp]))
    mean, var, first, total = indices_from_moments(E.reshape(P, gp, M), Q.reshape(P, gp, M, M, -1))
    if average == "mean":
        mean, var, first, total = mean[:, 0], var[:, 0], first[:, 0], total[:, 0]
    else:                                                # (P, S, ..) -> (S, P, ..)
        mean, var = mean.t().contiguous(), var.t().contiguous()
        first, total = first.transpose(0, 1).contiguous(), total.transpose(0, 1).contiguous()
    gfirst = gtotal = None
    if pcvar is not None:
        pv = torch.as_tensor(np.asarray(_host(pcvar), dtype=np.float64).reshape(-1), dtype=F64,
                             device=dev)
        if pv.numel() != P:
            raise ValueError(f"pcvar: expected {P} values, got {pv.numel()}")
        gfirst = (pv[:, None] * first).sum(-2)
        gtotal = (pv[:, None] * total).sum(-2)
    return ExactSobolResult(first, total, gfirst, gtotal, mean, var, average)


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x
