"""Mean-response surfaces of the emulator: main effects and input pairs, on libgpfit.

Reference usage being replaced (``experiments/synthetic/analysis/mean_response.py``):
  * ``compute_mean_response`` (lines 82-138): per input dimension, a SepiaEmulatorPrediction at
    11 targets x 20 Latin-hypercube integration points, averaged over the posterior samples and
    over the integration points                              -> :func:`mean_response`
  * ``compute_mean_response_pairs`` (lines 159-208): per input pair, one SepiaEmulatorPrediction
    of 10 points per node of an 11 x 11 grid                 -> :func:`mean_response_pairs`

Only the predictive mean is needed and the ARD kernel is a product over dimensions, so with
``alpha = A^-1 w_hat`` per (sample, PC) GP the average over the integration points has a closed
form (gp_mean_response, include/gpfit.h): no test point is materialised, and one factorisation
per GP serves every effect.  Per group of GPs: ``kernels.gram`` -> ``cholesky_inverse`` ->
``check`` -> ``kernels.alpha``; then one ``kernels.mean_response`` over all of them.

One difference from the reference: in the main-effect path it casts ``.w`` to float32 per
predicted point before averaging over the integration points (``GPpred.w =
GPpred.w.astype(np.float32)``, line 127); here the average is taken in fp64.  The results agree to
the float32 rounding of w.  (The reference's float32 ``xpred`` is reproduced: ``round_f32``.)
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import kernels
from .emulator import EmulatorModel, EmulatorPrediction, _np, gp_params

F64 = torch.float64


def integration_design(n_cols: int, n_integrate: int, seed: int = 20240418) -> np.ndarray:
    """The reference's integration points (mean_response.py:86-88, 167-169):
    ``qmc.LatinHypercube(n_cols, optimization='random-cd', scramble=False, seed=seed)
    .random(n_integrate)``, (n_integrate, n_cols) float64, on the host (scipy).  The design is a
    function of its arguments alone and scipy's random-cd optimisation takes tens of
    milliseconds, more than the surfaces themselves: an integer seed's design is computed once
    per process and a copy returned."""
    if n_cols < 1:
        return np.zeros((int(n_integrate), 0))
    if isinstance(seed, (int, np.integer)):
        return _design(int(n_cols), int(n_integrate), int(seed)).copy()
    return _design.__wrapped__(int(n_cols), int(n_integrate), seed)


@functools.lru_cache(maxsize=64)
def _design(n_cols: int, n_integrate: int, seed):
    from scipy.stats import qmc
    sampler = qmc.LatinHypercube(n_cols, optimization="random-cd", scramble=False, seed=seed)
    return sampler.random(n=n_integrate)


class MeanResponsePrediction(EmulatorPrediction):
    """The surfaces as an :class:`EmulatorPrediction` whose m "points" are the grid nodes of
    every effect in turn (m = E T for main effects, E T^2 for pairs): ``.w`` (S, m, P) is the
    integrated posterior mean of the PC weights per posterior sample, ``get_y()`` and
    ``summary(q)`` (the band over the posterior samples) work unchanged, and :meth:`response`
    gives the reference's arrays.  The variance is zero: an average of predictive means has no
    marginal draw to make, so there is no ``realize``."""

    def __init__(self, model: EmulatorModel, samples: dict, mean_u: torch.Tensor, grid: tuple,
                 effects, targets: np.ndarray, design):
        self.model = model
        S = np.asarray(samples["lamUz"]).reshape(-1, model.P).shape[0]
        self.S, self.m, self.P = S, mean_u.shape[1], model.P
        self.shard = "units"
        self.lamWOs = np.asarray(samples["lamWOs"], dtype=np.float64).reshape(S)
        self.grid = tuple(grid)              # (E, T) or (E, T, T)
        self.effects = effects
        self.targets = targets
        self.design = design
        self._set_results(None, False, 0, (mean_u, torch.zeros_like(mean_u)))

    def sample_w(self, seed=None, offset=1):
        raise ValueError("realize: a mean-response surface is an average of predictive means; "
                         "it has no marginal draw")

    def response(self, std: bool = False) -> np.ndarray:
        """Mean over the posterior samples of ``(w K) sd + mu``, (E, T, ny) for main effects or
        (E, T, T, ny) for pairs.  For the reference's scalar models (ny = 1)
        ``response()[..., 0]`` is ``Y_integrated_mean[j]`` (E, T) / ``y_response_pair`` per pair,
        indexed [i1, i2] with x_d1 = xi[i2], x_d2 = xi[i1] as the reference's meshgrid."""
        mean = self.summary(0.5, std=std, add_error=False)[0]
        return np.asarray(mean, dtype=np.float64).reshape(self.grid + (-1,))


def unit_alpha(model, samples, budget_bytes: int = 2 << 30, group: int | None = None):
    """``alpha = A^-1 w_hat`` of every (sample, PC) GP of ``samples``, the weights of its posterior
    mean: per group of GPs under ``budget_bytes`` (at most ``group``) ``kernels.gram`` ->
    ``cholesky_inverse`` -> ``check`` -> ``kernels.alpha``.  Returns (alpha (S P, n), beta
    (S P, d), s (S P,), S, P) on the model's device, the units (sample, PC) in sample-major
    order."""
    dev = model.device
    X = model.data.sim_data.t_dev
    n, d = model.n, model.d
    beta, s, delta, _ = gp_params(samples, _np(model.LamSim), d, model.P, True)
    S, P = s.shape
    U = S * P
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa
    # units (s, j) in s-major order
    beta_u, s_u, delta_u = t(beta.reshape(U, -1)), t(s.reshape(-1)), t(delta.reshape(-1))
    w_u = model.w_hat.transpose(0, 1).contiguous().repeat(S, 1)     # (S P, n)
    npad = kernels.padded_n(n)
    g = max(1, int(budget_bytes // (8 * (n * n + npad * npad))))
    if group is not None:
        g = max(1, min(g, int(group)))
    alpha = torch.empty((U, n), dtype=F64, device=dev)
    for a in range(0, U, g):
        b = min(U, a + g)
        ch = kernels.cholesky_inverse(kernels.gram(X, beta_u[a:b], s_u[a:b], delta_u[a:b],
                                                   batch=b - a))
        ch.check()
        kernels.alpha(ch, w_u[a:b], out=alpha[a:b])
    return alpha, beta_u, s_u, S, P


def _surfaces(model, samples, effects, nfree, order, targets, ntarget, design, nintegrate,
              round_f32, budget_bytes, group):
    if not isinstance(model, EmulatorModel) or samples is None:
        raise ValueError("mean_response needs an EmulatorModel and its samples")
    dev = model.device
    X = model.data.sim_data.t_dev
    n, d = model.n, model.d
    nc = d - nfree
    if nc < 0:
        raise ValueError(f"pairs need a model with at least 2 inputs, got d = {d}")
    xi = np.linspace(0.0, 1.0, int(ntarget)) if targets is None else \
        np.asarray(targets, dtype=np.float64).reshape(-1)
    if nc == 0:
        design = None
    elif design is None:
        design = integration_design(nc, nintegrate)
    else:
        design = np.asarray(design, dtype=np.float64)
        if design.ndim != 2 or design.shape[1] != nc:
            raise ValueError(f"design: expected (I, {nc}), got {design.shape}")
    if round_f32:
        # the reference writes its points into a float32 xpred (mean_response.py:122, 195)
        xi = xi.astype(np.float32).astype(np.float64)
        design = None if design is None else design.astype(np.float32).astype(np.float64)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa
    alpha, beta_u, s_u, S, P = unit_alpha(model, samples, budget_bytes, group)
    U = S * P
    t1 = t(xi)
    effects = np.asarray(effects, dtype=np.int64).reshape((-1, 2) if nfree == 2 else (-1,))
    res =kernels.mean_response(X.contiguous(), alpha, beta_u, s_u, effects, t1,
                                t1 if nfree == 2 else None,
                                None if design is None else t(design), order=order)
    E, T = res.shape[1], xi.size
    grid = (E, T) if nfree == 1 else (E, T, T)
    return MeanResponsePrediction(model, samples, res.reshape(U, -1), grid, effects, xi, design)


def mean_response(model: EmulatorModel, samples: dict, ntarget: int = 11, nintegrate: int = 20,
                  dims=None, targets=None, design=None, round_f32: bool = True,
                  budget_bytes: int = 2 << 30, group: int | None = None):
    """Main-effect surfaces (compute_mean_response, mean_response.py:82-138): for every input
    dimension of ``dims`` (default all), the emulator's posterior mean at ``targets`` (default
    ``linspace(0, 1, ntarget)``) averaged over the ``design`` (default
    ``integration_design(d - 1, nintegrate)``) placed in the other dimensions by the reference's
    cyclic rule: integration column c takes dimension (dim + 1 + c) mod d.  ``round_f32`` rounds
    the targets and the design to float32 and widens them again, as the reference's float32
    ``xpred`` does.  Returns a :class:`MeanResponsePrediction`; ``.response()[..., 0]`` is the
    reference's ``Y_integrated_mean[j]`` up to the float32 cast of w noted in the module
    docstring.  ``budget_bytes`` / ``group`` bound the GPs per batched factorisation as in
    ``predict_units``.  Single process: there is no ``ctx``."""
    d = model.d
    dims = list(range(d)) if dims is None else [int(k) for k in np.atleast_1d(dims)]
    return _surfaces(model, samples, dims, 1, "cyclic", targets, ntarget, design, nintegrate,
                     round_f32, budget_bytes, group)


def mean_response_pairs(model: EmulatorModel, samples: dict, pairs, ntarget: int = 11,
                        nintegrate: int = 10, targets=None, design=None, round_f32: bool = True,
                        budget_bytes: int = 2 << 30, group: int | None = None):
    """Pair surfaces (compute_mean_response_pairs, mean_response.py:159-208): for every (d1, d2)
    of ``pairs`` the posterior mean on the ``targets`` x ``targets`` grid averaged over the
    ``design`` (default ``integration_design(d - 2, nintegrate)``) placed in the other dimensions
    in ascending order.  The surface of a pair is indexed [i1, i2] with x_d1 = xi[i2] and
    x_d2 = xi[i1], as the reference's ``meshgrid``; ``.response()[k, :, :, 0]`` is its
    ``y_response_pair``.  Other arguments as :func:`mean_response`."""
    pairs = [(int(p[0]), int(p[1])) for p in pairs]
    return _surfaces(model, samples, pairs, 2, "ascending", targets, ntarget, design, nintegrate,
                     round_f32, budget_bytes, group)
