"""Multivariate GP emulator surface (the SEPIA objects the reference drives), on libgpfit.

Reference usage being replaced (SEPIA fork, un-vendored, ``requirements-cc.txt:55``):
  * ``SepiaData(t_sim, y_sim, y_ind_sim)`` + ``standardize_y`` + ``create_K_basis(K)``
    (``src/model.py:57-102``)                              -> :class:`EmulatorData`
  * ``SepiaModel(data)``, ``.get_samples(numsamples, nburn)``, ``.save_model_info`` /
    ``.restore_model_info`` (``src/model.py:106, 149, 238``; ``assess_all_models.py:471``)
                                                           -> :class:`EmulatorModel`
  * ``SepiaEmulatorPrediction(model=, samples=, t_pred=)`` with ``.w`` (S, m, P) and
    ``.get_y()`` (S, m, ny) (``time_predictions.py:76-79``, ``sensitivity_indices.py:85-88``,
    ``assess_all_models.py:489-492``)                      -> :class:`EmulatorPrediction`

The GPMSA sim-only model, per MCMC sample s and principal component j (one independent GP
each), with betaU (S, (d+1) P) reshaped C-order to (S, d+1, P), row 0 the dummy x
(``mcmc_diagnostics_advanced.py:57``):
  Sigma_j = (1/lamUz_j) exp(-sum_k beta_kj (t_ik - t_i'k)^2)
            + (1/lamWs_j + 1/(lamWOs LamSim_j)) I                       (training block)
  k*_j    = (1/lamUz_j) exp(-sum_k beta_kj (t*_k - t_ik)^2)              (cross-covariance)
  mean    = k*_j^T Sigma_j^-1 w_hat_j,  var = 1/lamUz_j [+ 1/lamWs_j] - k*_j^T Sigma_j^-1 k*_j
``pred_nugget`` selects whether 1/lamWs is part of the predictive prior variance (SEPIA's
exact choice is not verifiable offline — SURVEY §8c — so it is a flag, default on).

Differences from SEPIA: by default ``.w`` is the posterior MEAN per (sample, PC) and ``.var``
the marginal variance (SEPIA returns one joint random draw over the m_b x m_b covariance of a
call, which does not scale to m = 100k).  ``realize=True`` makes ``.w`` one marginal draw per
(sample, point, PC) instead (gp_realize, Philox4x32-10 on the device, seeded by ``seed``), so the
reference's quantile / coverage statistics over ``get_y()`` (assess_all_models.py:489-500) keep
the GP's predictive spread.  ``realize="joint"`` is SEPIA's own form for the block sizes it is
used at (m <= ``joint_max_points``): the full m x m predictive covariance of every (sample, PC)
GP (gp_predict_cov) and joint draws from it (gp_potrf + gp_mvn_draw), with ``.cov()`` and
``.linear_functional()`` for what needs the correlation between test points.  SEPIA draws
through an SVD of the covariance, this package through its Cholesky factor plus a jitter: the
draws agree in distribution, not number for number.  ``.mean`` always holds the posterior mean.
``.w`` is assignable, as the reference's callers do
(``preds.w = preds.w.astype(np.float32)``, time_predictions.py:78, assess_all_models.py:490,
513): ``get_y()`` then reconstructs from the assigned values and returns that dtype.  All
arithmetic runs in libgpfit (fp64); the (sample, PC) pairs are one batched Gram ->
Cholesky/L^-1 -> predict.

Repeat chains (``EmulatorModel.do_mcmc_chains``, the run of mcmc_diagnostics_advanced.py:50-54):
chain 0 starts at the current values; every later chain, unless the caller gives its start,
starts at the current values with each element multiplied by exp(0.5 z), z ~ N(0, 1) from
``model.rng``, clipped into the parameter's bounds.  This dispersed-start rule is *unpinned*:
SEPIA's own restart rule (``do_mcmc(no_init=False)``) cannot be checked offline.
"""
from __future__ import annotations

import copy
import os

import numpy as np
import torch

from . import blas, kernels
from . import dist as gdist
from . import mcmc, modelio
from .blas import CM, gemm
from .mcmc import ModelParams, SepiaParam  # noqa: F401  (re-exported for drop-in imports)

F64 = torch.float64


def _dev(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("the emulator runs on a HIP device (libgpfit); none found")
    return torch.device("cuda", torch.cuda.current_device())


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _to_host(t: torch.Tensor, dtype) -> np.ndarray:
    """Device tensor -> numpy in ``dtype``: narrowed on the device first (a float32 field crosses
    PCIe at half the bytes and skips a host conversion pass), copied into page-locked memory
    (one DMA, no pageable bounce; the returned array keeps its pinned block alive)."""
    tt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    src = t.to(tt).contiguous()
    host = torch.empty(src.shape, dtype=tt, pin_memory=True)
    host.copy_(src)
    return host.numpy()


def _to_device_f64(x, device) -> torch.Tensor:
    """float64 device copy of ``x``: host arrays cross PCIe in their own dtype (float32
    ensembles at half the bytes) and are widened on the device, not on the host."""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=F64).contiguous()
    a = np.ascontiguousarray(np.asarray(x))
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return torch.from_numpy(a).to(device).to(F64).contiguous()


class SimData:
    """Simulation block: design, raw and standardised outputs, PCA basis (SEPIA sim_data).

    ``t`` / ``y`` are host (numpy) arrays in the caller's dtype, as SEPIA's are — the
    reference's drivers run numpy on them (``np.std(model.data.sim_data.y, ddof=1, axis=0)``,
    time_predictions.py:65, assess_all_models.py:465); ``t_dev`` / ``y_dev`` are the float64
    device copies every kernel reads."""

    def __init__(self, t_sim, y_sim, y_ind_sim, device):
        self.device = device
        self.t_dev = _to_device_f64(t_sim, device)
        self.y_dev = _to_device_f64(y_sim, device)
        self._t_host = None if torch.is_tensor(t_sim) else np.asarray(t_sim)
        self._y_host = None if torch.is_tensor(y_sim) else np.asarray(y_sim)
        self.y_ind = np.asarray(y_ind_sim)
        self.y_mean = None
        self.y_sd = None
        self.y_std = None
        self.K = None          # (P, ny) basis

    @property
    def t(self) -> np.ndarray:
        if self._t_host is None:
            self._t_host = self.t_dev.cpu().numpy()
        return self._t_host

    @property
    def y(self) -> np.ndarray:
        if self._y_host is None:
            self._y_host = self.y_dev.cpu().numpy()
        return self._y_host

    @property
    def n(self) -> int:
        return self.t_dev.shape[0]


class EmulatorData:
    """Mirror of the SepiaData pieces src/model.py uses (sim-only, x = dummy)."""

    def __init__(self, t_sim, y_sim, y_ind_sim=None, device=None):
        device = _dev(device)
        y_ind_sim = np.linspace(0, 1, np.shape(y_sim)[1]) if y_ind_sim is None else y_ind_sim
        self.sim_data = SimData(t_sim, y_sim, y_ind_sim, device)
        self.device = device

    def standardize_y(self, y_mean=None, y_sd=None, sd_threshold=1e-6):
        """y_std = (y - mu)/sd with mu/sd from the ensemble when not given (model.py:60-73)."""
        sd_ = self.sim_data
        if y_mean is None or y_sd is None:
            mu, sd = blas.sim_stats(sd_.y_dev, sd_threshold)
        else:
            mu = torch.as_tensor(_np(y_mean), dtype=F64, device=self.device).contiguous()
            sd = torch.as_tensor(_np(y_sd), dtype=F64, device=self.device).contiguous()
        sd_.y_mean, sd_.y_sd = mu, sd
        # rows padded to a multiple of 16 doubles (128 B): every row of the ensemble starts
        # 16-B aligned, so the randomized SVD's ensemble-streaming products read it with 16-B
        # loads (the 16-B form of blas.hip's gemm_tsk_kernel); y_std is a (n x ny) view of the
        # padded buffer
        n, ny = sd_.y_dev.shape
        ld = (ny + 15) // 16 * 16
        out = torch.empty((n, ld), dtype=F64, device=sd_.y_dev.device)[:, :ny]
        sd_.y_std = blas.standardize(sd_.y_dev, mu, sd, out=out)

    def create_K_basis(self, K):
        """Set the PCA basis K (P x ny) — SEPIA create_K_basis (model.py:102)."""
        self.sim_data.K = (K.to(device=self.device, dtype=F64).contiguous() if torch.is_tensor(K)
                           else torch.as_tensor(np.asarray(K), dtype=F64,
                                                device=self.device).contiguous())


def pc_weights(data: EmulatorData):
    """w_hat = y_std pinv(K) (n x P) and LamSim = diag(K K^T) — model.py:219; SEPIA's w.

    pinv(K) = K^T (K K^T)^-1 for a full-row-rank basis: two MFMA GEMMs and the P x P
    Cholesky inverse (K K^T)^-1 = L^-T L^-1.
    """
    sd_ = data.sim_data
    K = CM.of_rowmajor(sd_.K)             # (ny x P) column-major view of K^T
    Ys = CM.of_rowmajor(sd_.y_std)        # (ny x n)
    P = sd_.K.shape[0]
    KKt = gemm(True, False, K, K)         # (P x P) = K K^T
    lam = torch.diagonal(KKt.logical()).contiguous().clone()
    YK = gemm(True, False, Ys, K)         # (n x P) = y_std K^T
    ch = kernels.cholesky_inverse(KKt.t[:P, :P].reshape(1, P, P).contiguous())
    ch.check()
    Linv = CM(ch.linv_buf[0], P, P, ch.linv_buf.shape[1])
    T = gemm(False, True, YK, Linv)       # (n x P) = y_std K^T L^-T
    W = gemm(False, False, T, Linv)       # (n x P) = y_std K^T L^-T L^-1
    return W, lam


class EmulatorModel:
    """Mirror of the SepiaModel surface the reference uses (sim-only)."""

    param_names = ("betaU", "lamUz", "lamWs", "lamWOs")

    def __init__(self, data: EmulatorData):
        self.data = data
        sd_ = data.sim_data
        if sd_.K is None or sd_.y_std is None:
            raise ValueError("EmulatorModel needs standardised y and a K basis")
        self.device = data.device
        self.w_hat_cm, lam = pc_weights(data)          # (n x P) column-major
        self.LamSim = lam
        self.n, self.d = sd_.t_dev.shape
        self.P = sd_.K.shape[0]
        # GPMSA default starting values, priors and steps (see gladsgp_amd.mcmc)
        self.params = ModelParams(self.d, self.P)
        self.samples = None
        self.rng = np.random.default_rng()

    # ---------------------------------------------------------------------------- sampling
    def _sampler(self) -> mcmc.GPUSampler:
        return mcmc.GPUSampler(self.data.sim_data.t_dev, self.w_hat.transpose(0, 1).contiguous(),
                               self.LamSim, self.params)

    def tune_step_sizes(self, n_burn, n_levels, prog=False, diagnostics=False,
                        update_vals=True):
        """SEPIA tune_step_sizes (src/model.py:234): per-element Metropolis step sizes from
        n_levels x n_burn sweeps on the GPU (algorithm: gladsgp_amd.mcmc module doc)."""
        sm = self._sampler()
        mcmc.tune_step_sizes(sm, int(n_burn), int(n_levels), self.rng)
        self.tune_info = sm.last_tune
        if diagnostics:
            for k, a in sm.last_tune["accepts"].items():
                print(f"tune {k}: acceptance per level (rows = step scale "
                      f"{sm.last_tune['scales'].tolist()}):\n{a / n_burn}")
        if update_vals:
            sm.write_back()

    def do_mcmc(self, nsamp, prog=False, do_propMH=True, no_init=False):
        """SEPIA do_mcmc (src/model.py:235): ``nsamp`` component-wise Metropolis sweeps on the
        GPU, appended to ``samples`` (betaU (N, (d+1) P), lamUz/lamWs (N, P), lamWOs (N, 1),
        logPost (N, 1)); the last state becomes the current parameter values."""
        sm = self._sampler()
        new = sm.run(int(nsamp), self.rng)
        sm.write_back()
        if self.samples is None:
            self.samples = new
        else:
            self.samples = {k: np.concatenate([self.samples[k], new[k]]) for k in new}

    def do_mcmc_chains(self, nsamp, nchains, starts=None, seeds=None):
        """``nchains`` chains of this model in one ensemble (mcmc.EnsembleSampler), ``nsamp``
        sweeps each, stored as ``self.chains``: betaU (C, N, (d+1) P), lamUz / lamWs (C, N, P),
        lamWOs / logPost (C, N, 1).  ``samples``, the current parameter values and ``do_mcmc``
        are untouched.  Chain 0 starts at the current values; chain c > 0 at ``starts[c]`` (a
        dict name -> values) if given, otherwise at the dispersed start of the module doc.
        Chain c draws from ``np.random.default_rng(seeds[c])``; by default the seeds are spawned
        from ``self.rng``.  This is the repeat-chain run of mcmc_diagnostics_advanced.py:50-54;
        ``chain_diagnostics`` gives R-hat and the effective sample size of the result."""
        C = int(nchains)
        plist = []
        for c in range(C):
            pr = copy.deepcopy(self.params)
            if c > 0:
                for k in ModelParams.names:
                    p = getattr(pr, k)
                    if starts is not None and starts[c] is not None:
                        pr[k] = starts[c][k]
                    else:
                        z = self.rng.standard_normal(p.val_shape)
                        p.val = np.clip(p.val * np.exp(0.5 * z), p.bounds[0], p.bounds[1])
            plist.append(pr)
        if seeds is None:
            seeds = self.rng.bit_generator.seed_seq.spawn(C)
        if len(seeds) != C:
            raise ValueError(f"{len(seeds)} seeds for {C} chains")
        w = self.w_hat.transpose(0, 1).contiguous()                     # (P, n)
        sm = mcmc.EnsembleSampler(self.data.sim_data.t_dev, w[None].expand(C, -1, -1),
                                  self.LamSim.reshape(1, -1).expand(C, -1), plist)
        self.chains = sm.run(int(nsamp), [np.random.default_rng(s) for s in seeds])
        return self.chains

    def chain_diagnostics(self, nburn=0) -> dict:
        """Split-R-hat and effective sample size of ``self.chains`` after ``nburn`` draws
        (mcmc.rhat / mcmc.ess): {"rhat": {name: (width,)}, "ess": {name: (width,)}} for betaU,
        lamUz, lamWs, lamWOs and logPost."""
        if getattr(self, "chains", None) is None:
            raise ValueError("model has no chains (do_mcmc_chains first)")
        return {"rhat": {k: mcmc.rhat(v, nburn) for k, v in self.chains.items()},
                "ess": {k: mcmc.ess(v, nburn) for k, v in self.chains.items()}}

    @property
    def w_hat(self) -> torch.Tensor:
        """(n, P) PC weights of the training runs."""
        return self.w_hat_cm.logical()

    # ---------------------------------------------------------------------------------- I/O
    def set_samples(self, samples: dict):
        self.samples = {k: np.asarray(v, dtype=np.float64) for k, v in samples.items()}

    def get_samples(self, numsamples=None, nburn=0):
        """Posterior samples after ``nburn``, optionally ``numsamples`` evenly spaced."""
        if self.samples is None:
            raise ValueError("model has no MCMC samples (restore_model_info or set_samples)")
        tot = len(self.samples["lamUz"])
        idx = np.arange(nburn, tot)
        if numsamples is not None and numsamples < len(idx):
            idx = idx[np.linspace(0, len(idx) - 1, numsamples).astype(int)]
        return {k: v[idx] for k, v in self.samples.items()}

    def save_model_info(self, path):
        """Samples, current values and step sizes as ``path + '.npz'`` (plain arrays,
        gladsgp_amd.modelio)."""
        modelio.save_model_npz(path, self.samples,
                               {k: getattr(self.params, k).val for k in ModelParams.names},
                               {k: getattr(self.params, k).mcmcStepParam
                                for k in ModelParams.names})

    def restore_model_info(self, path):
        """Read ``path + '.npz'`` written by save_model_info or by
        tools/export_sepia_samples.py from a SEPIA fit (gladsgp_amd.modelio)."""
        samples, params, steps = modelio.load_model_npz(path)
        for k, v in params.items():
            self.params[k] = v
        for k, v in steps.items():
            p = getattr(self.params, k)
            p.mcmcStepParam = np.broadcast_to(v, p.val_shape).copy()
        self.samples = samples or None

    # ------------------------------------------------------------------------- likelihood
    def log_likelihood(self, params=None) -> float:
        """Sum over PCs of the Gaussian log-likelihood of w_hat_j (no 2pi term, no priors).

        Building block of SEPIA's logLik for the sim-only model (driven by do_mcmc,
        src/model.py:234-235): one batched Gram -> Cholesky -> nll over the P GPs.
        """
        pr = self.params.values() if params is None else params
        samples = {k: np.asarray(pr[k]).reshape(1, -1) for k in self.param_names}
        beta, s, delta, _ = gp_params(samples, _np(self.LamSim), self.d, self.P, False)
        X = self.data.sim_data.t_dev
        G = kernels.gram(X, torch.as_tensor(beta[0], device=self.device),
                         torch.as_tensor(s[0], device=self.device),
                         torch.as_tensor(delta[0], device=self.device), batch=self.P)
        ch = kernels.cholesky_inverse(G)
        ch.check()
        w = self.w_hat.transpose(0, 1).contiguous()           # (P, n)
        return -float(kernels.nll(ch, w).sum().item())

    def log_likelihood_grad(self, params=None) -> dict:
        """Gradient of :meth:`log_likelihood` (the log-likelihood summed over PCs, no priors) in
        the SEPIA parameters: a dict with the keys and shapes of ``params.values()`` -- betaU
        (d + 1, P) with 0 in the dummy-x row, lamUz and lamWs (1, P), lamWOs (1, 1).

        One batched kernels.nll_value_grad over the P GPs gives dNLL_j / d(s_j, delta_j, beta_jk);
        the chain rule through :func:`gp_params` (s = 1 / lamUz, delta_j = 1 / lamWs_j +
        1 / (lamWOs LamSim_j)) and the sign of the log-likelihood give
        d/dbetaU[1 + k, j] = -dNLL_j/dbeta_k, d/dlamUz_j = dNLL_j/ds / lamUz_j^2,
        d/dlamWs_j = dNLL_j/ddelta / lamWs_j^2 and d/dlamWOs = sum_j dNLL_j/ddelta /
        (lamWOs^2 LamSim_j).  Raises like :meth:`log_likelihood` where a Gram is not positive
        definite."""
        pr = self.params.values() if params is None else params
        samples = {k: np.asarray(pr[k]).reshape(1, -1) for k in self.param_names}
        lam = _np(self.LamSim).reshape(-1)
        beta, s, delta, _ = gp_params(samples, lam, self.d, self.P, False)
        dev = self.device
        w = self.w_hat.transpose(0, 1).contiguous()           # (P, n)
        _, g, info = kernels.nll_value_grad(
            self.data.sim_data.t_dev, torch.as_tensor(beta[0], device=dev).contiguous(),
            torch.as_tensor(s[0], device=dev).contiguous(),
            torch.as_tensor(delta[0], device=dev).contiguous(), w)
        kernels.check_info(info)
        g = g.cpu().numpy()                                   # (P, d + 2)
        lamUz, lamWs = samples["lamUz"].reshape(-1), samples["lamWs"].reshape(-1)
        lamWOs = float(samples["lamWOs"].reshape(-1)[0])
        betaU = np.zeros((self.d + 1, self.P))
        betaU[1:] = -g[:, 2:].T
        return {"betaU": betaU, "lamUz": (g[:, 0] / lamUz ** 2).reshape(1, -1),
                "lamWs": (g[:, 1] / lamWs ** 2).reshape(1, -1),
                "lamWOs": np.sum(g[:, 1] / (lamWOs ** 2 * lam)).reshape(1, 1)}


def fit_ensemble(models, n_burn, n_levels, nsamp, tune=True):
    """Tune and sample a list of EmulatorModels on one design together: the drop-in for the
    inner loop of fit_scalar_models.py:457-473 (16 scalar emulators per ensemble size, each a
    ``tune_step_sizes(100, 10)`` + ``do_mcmc(512)``), as one mcmc.EnsembleSampler whose every
    gp_loglik call carries all models' problems.  The models must share ``t``, P and the priors,
    bounds and step types (ValueError names the field that differs); each is driven by its own
    ``model.rng`` and ends with ``samples``, parameter values, step sizes and ``tune_info`` as if
    it had run ``tune_step_sizes(n_burn, n_levels)`` + ``do_mcmc(nsamp)`` alone."""
    models = list(models)
    if not models:
        return models
    X = models[0].data.sim_data.t_dev
    mcmc.check_shared_priors([m.params for m in models])
    for c, m in enumerate(models[1:], start=1):
        if m.data.sim_data.t_dev.shape != X.shape or not torch.equal(m.data.sim_data.t_dev, X):
            raise ValueError(f"ensemble: model {c} differs from model 0 in t (the design)")
    w = torch.stack([m.w_hat.transpose(0, 1) for m in models]).contiguous()      # (C, P, n)
    lam = torch.stack([m.LamSim.reshape(-1) for m in models])
    sm = mcmc.EnsembleSampler(X, w, lam, [m.params for m in models])
    rngs = [m.rng for m in models]
    if tune:
        mcmc.tune_step_sizes_ensemble(sm, int(n_burn), int(n_levels), rngs)
        for m, info in zip(models, sm.last_tune):
            m.tune_info = info
        sm.write_back()
        sm.init_state()             # do_mcmc starts a sampler from the written-back values
    new = sm.run(int(nsamp), rngs)
    sm.write_back()
    for c, m in enumerate(models):
        mine = {k: v[c] for k, v in new.items()}
        m.samples = mine if m.samples is None else {
            k: np.concatenate([m.samples[k], mine[k]]) for k in mine}
    return models


def gp_params(samples, LamSim, d, P, pred_nugget=True):
    """Per (sample, PC) kernel parameters: beta (S, P, d), s, delta, s_pred (S, P).

    Parameter marshalling only (host, O(S P d)): the covariance arithmetic is in libgpfit.
    """
    bu = np.asarray(samples["betaU"], dtype=np.float64)
    S = bu.shape[0]
    beta = bu.reshape(S, d + 1, P)[:, 1:, :].transpose(0, 2, 1).copy()
    lamUz = np.asarray(samples["lamUz"], dtype=np.float64).reshape(S, P)
    lamWs = np.asarray(samples["lamWs"], dtype=np.float64).reshape(S, P)
    lamWOs = np.asarray(samples["lamWOs"], dtype=np.float64).reshape(S, 1)
    lam = np.asarray(LamSim, dtype=np.float64).reshape(1, P)
    s = 1.0 / lamUz
    delta = 1.0 / lamWs + 1.0 / (lamWOs * lam)
    s_pred = s + (1.0 / lamWs if pred_nugget else 0.0)
    return beta, s, delta, s_pred


def predict_units(X, Xs, w_units, beta_u, s_u, delta_u, sp_u, budget_bytes=2 << 30,
                  m_chunk=0, group=None, fctx: kernels.FitPredictContext | None = None,
                  workspace: kernels.PredictWorkspace | None = None):
    """Posterior mean / variance of a list of GPs sharing X and Xs: returns (U, m) x 2.

    Units are processed in groups bounded by ``budget_bytes`` of Gram + L^-1 storage, and by
    ``group`` GPs per group when given; each group is one gp_fit_predict (batched Gram ->
    factorisation -> cross-covariance / TRMM / mean + variance), whose cross-covariance runs on
    ``fctx``'s own stream beside the factorisation when a context is given (bit-identical to
    gram -> potrf -> predict on one stream: tests/test_gpu_c4.py).
    """
    dev = X.device
    U = beta_u.shape[0]
    n = X.shape[0]
    m = Xs.shape[0]
    npad = kernels.padded_n(n)
    per = 8 * (n * n + npad * npad)
    g = max(1, int(budget_bytes // per))
    if group is not None:
        g = max(1, min(g, int(group)))
    mean = torch.empty((U, m), dtype=F64, device=dev)
    var = torch.empty((U, m), dtype=F64, device=dev)
    ws = workspace if workspace is not None else kernels.PredictWorkspace()
    for a in range(0, U, g):
        b = min(U, a + g)
        kernels.fit_predict(X, Xs, beta_u[a:b], s_u[a:b], delta_u[a:b], sp_u[a:b],
                            w_units[a:b], m_chunk=m_chunk, workspace=ws,
                            out=(mean[a:b], var[a:b]), ctx=fctx, check=True)
    return mean, var


class EmulatorPrediction:
    """Predictions of the P PC-GPs for each posterior sample at ``t_pred`` (m x d).

    ``ctx`` (a :class:`gladsgp_amd.dist.Context`) shards the work over ranks; rank 0 receives
    the gathered (S, m, P) results, other ranks hold ``None``:
      * units (S P) >= ranks: the (sample, PC) units are dealt round-robin (SURVEY §8e,
        multivariate emulator);
      * fewer units than ranks (the reference's scalar GPs: P = 1 with few samples,
        fit_scalar_models.py:477-481, mean_response.py:114-126) with m >= ranks: the test points
        are split instead, every rank predicting every unit on its contiguous block
        (``shard="points"``, SURVEY §8e single-output GP; see gladsgp_amd.sharded).
    ``shard`` forces "units" or "points".  ``group`` caps the GPs per batched factorisation.
    ``fctx`` / ``workspace``: a caller-owned gp_fit_predict context (cross-covariance beside the
    factorisation) and prediction workspace, reused across calls.

    ``realize="joint"`` (single device, m <= ``joint_max_points``): ``.w`` is draw 0 of ``nsamp``
    joint draws over the m test points per (sample, PC); per group of units under
    ``budget_bytes`` the chain is gram -> cholesky_inverse -> predict -> predict_cov -> gp_potrf
    -> mvn_draw.  ``.mean`` / ``.var`` have the default mode's bits.  Unit u = s P + j draws from
    its own slice of the normal stream, so the draws do not depend on ``group`` /
    ``budget_bytes``.  ``joint_jitter`` (a multiple of s added to the covariance's diagonal)
    defaults to 0 with ``pred_nugget`` and 1e-8 without; a non-positive pivot raises
    :class:`kernels.JointNotPositiveDefinite`.  See :meth:`sample_w`, :meth:`cov`,
    :meth:`linear_functional`.
    """

    joint_max_points = 4096
    joint_jitter_default = 1e-8     # without the prediction nugget, a multiple of s

    def __init__(self, model: EmulatorModel = None, samples: dict = None, t_pred=None,
                 pred_nugget: bool = True, ctx: gdist.Context | None = None,
                 budget_bytes: int = 2 << 30, m_chunk: int = 0, realize=False,
                 seed: int | None = None, group: int | None = None, shard: str | None = None,
                 fctx: kernels.FitPredictContext | None = None,
                 workspace: kernels.PredictWorkspace | None = None,
                 joint_jitter: float | None = None, nsamp: int = 1):
        if model is None or samples is None or t_pred is None:
            raise ValueError("EmulatorPrediction needs model, samples and t_pred")
        if isinstance(realize, str):
            if realize != "joint":
                raise ValueError(f"realize must be False, True or 'joint', got {realize!r}")
            self._init_joint(model, samples, t_pred, pred_nugget, ctx, budget_bytes, seed, group,
                             workspace, joint_jitter, nsamp)
            return
        self.model = model
        dev = model.device
        X = model.data.sim_data.t_dev
        Xs = (t_pred.to(device=dev, dtype=F64) if torch.is_tensor(t_pred) else
              torch.as_tensor(np.asarray(t_pred), dtype=F64, device=dev))
        Xs = Xs.reshape(-1, model.d).contiguous()
        beta, s, delta, sp = gp_params(samples, _np(model.LamSim), model.d, model.P,
                                       pred_nugget)
        S, P = s.shape
        self.S, self.m, self.P = S, Xs.shape[0], P
        self.lamWOs = np.asarray(samples["lamWOs"], dtype=np.float64).reshape(S)
        units = [(a, j) for a in range(S) for j in range(P)]
        dist_on = ctx is not None and ctx.distributed
        rank, world = (ctx.rank, ctx.world) if dist_on else (0, 1)
        if shard is None:
            shard = "points" if (dist_on and len(units) < world and self.m >= world) else "units"
        if shard not in ("units", "points"):
            raise ValueError(f"shard must be 'units' or 'points', got {shard!r}")
        self.shard = shard if dist_on else "units"
        w_hat = model.w_hat.transpose(0, 1).contiguous()       # (P, n)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa
        if self.shard == "points":
            # every unit on this rank's contiguous block of the test points
            lo, hi = gdist.shard_range(self.m, rank, world)
            sel_s = np.array([u[0] for u in units])
            sel_j = np.array([u[1] for u in units])
            jj = torch.as_tensor(sel_j, device=dev)
            mean_l, var_l = predict_units(X, Xs[lo:hi].contiguous(), w_hat[jj].contiguous(),
                                          t(beta[sel_s, sel_j]), t(s[sel_s, sel_j]),
                                          t(delta[sel_s, sel_j]), t(sp[sel_s, sel_j]),
                                          budget_bytes, m_chunk, group, fctx, workspace)
        else:
            mine = gdist.shard_units(len(units), rank, world)
            if mine:
                sel_s = np.array([units[u][0] for u in mine])
                sel_j = np.array([units[u][1] for u in mine])
                jj = torch.as_tensor(sel_j, device=dev)
                mean_l, var_l = predict_units(X, Xs, w_hat[jj].contiguous(),
                                              t(beta[sel_s, sel_j]), t(s[sel_s, sel_j]),
                                              t(delta[sel_s, sel_j]), t(sp[sel_s, sel_j]),
                                              budget_bytes, m_chunk, group, fctx, workspace)
            else:
                mean_l = torch.empty((0, self.m), dtype=F64, device=dev)
                var_l = torch.empty((0, self.m), dtype=F64, device=dev)
        self._set_results(ctx, realize, seed,
                          assemble_points(ctx, mean_l, var_l, self.m) if self.shard == "points"
                          else assemble_units(ctx, mean_l, var_l, len(units)))

    # ------------------------------------------------------------------------ joint mode
    def _init_joint(self, model, samples, t_pred, pred_nugget, ctx, budget_bytes, seed, group,
                    workspace, joint_jitter, nsamp) -> None:
        if ctx is not None:
            raise ValueError("ctx: joint draws are not sharded over devices (pass None)")
        self.model = model
        dev = model.device
        Xs = (t_pred.to(device=dev, dtype=F64) if torch.is_tensor(t_pred) else
              torch.as_tensor(np.asarray(t_pred), dtype=F64, device=dev))
        Xs = Xs.reshape(-1, model.d).contiguous()
        m = Xs.shape[0]
        if m > self.joint_max_points:
            raise ValueError(
                f"realize='joint': {m} test points exceed joint_max_points = "
                f"{self.joint_max_points} (an m x m covariance per (sample, PC)); predict in "
                "blocks, or use the marginal mode (realize=True)")
        if int(nsamp) < 1:
            raise ValueError("nsamp must be at least 1")
        beta, s, delta, sp = gp_params(samples, _np(model.LamSim), model.d, model.P, pred_nugget)
        S, P = s.shape
        self.S, self.m, self.P = S, m, P
        self.shard = "units"
        self.lamWOs = np.asarray(samples["lamWOs"], dtype=np.float64).reshape(S)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa
        self.joint_jitter = float((0.0 if pred_nugget else self.joint_jitter_default)
                                  if joint_jitter is None else joint_jitter)
        w_hat = model.w_hat.transpose(0, 1).contiguous()       # (P, n)
        n = model.n
        npad = kernels.padded_n(n)
        per = 8 * (n * n + npad * npad + m * m) + \
            int(kernels._capi.lib().gp_predict_cov_ws_bytes(n, max(m, 1), 1))
        g = max(1, int(budget_bytes // per))
        if group is not None:
            g = max(1, min(g, int(group)))
        # units (s, j) in s-major order
        self._joint = dict(
            X=model.data.sim_data.t_dev, Xs=Xs, beta=t(beta.reshape(S * P, -1)),
            s=t(s.reshape(-1)), delta=t(delta.reshape(-1)), sp=t(sp.reshape(-1)),
            jit=t(s.reshape(-1) * self.joint_jitter), w=w_hat.repeat(S, 1), g=g,
            ws=workspace if workspace is not None else kernels.PredictWorkspace())
        U = S * P
        mean = torch.empty((U, m), dtype=F64, device=dev)
        var = torch.empty((U, m), dtype=F64, device=dev)
        self._set_results(None, False, seed, (mean, var), fill=False)
        self.realized = "joint"
        self.nsamp = int(nsamp)
        draws = self._joint_draws(self.seed, 0, self.nsamp, mean_out=(mean, var))
        self.mean_dev = mean.reshape(S, P, m).permute(0, 2, 1).contiguous()
        self.var_dev = var.reshape(S, P, m).permute(0, 2, 1).contiguous()
        self.joint_w_dev = draws                               # (nsamp, S, m, P)
        self.w_dev = draws[0]

    def _joint_groups(self, mean_out=None):
        """The chain of one group of units at a time: yields (a, b, mean (b - a, m), C
        (b - a, m, m)), C in a buffer the caller may overwrite."""
        J = self._joint
        U, m = self.S * self.P, self.m
        for a in range(0, U, J["g"]):
            b = min(U, a + J["g"])
            ch = kernels.cholesky_inverse(kernels.gram(J["X"], J["beta"][a:b], J["s"][a:b],
                                                       J["delta"][a:b], batch=b - a))
            ch.check()
            if mean_out is not None:
                out = (mean_out[0][a:b], mean_out[1][a:b])
                kernels.predict(ch, J["X"], J["Xs"], J["beta"][a:b], J["s"][a:b], J["sp"][a:b],
                                J["w"][a:b], workspace=J["ws"], out=out)
                mean = out[0]
            else:
                mean = self.mean_dev.permute(0, 2, 1).reshape(U, m)[a:b].contiguous()
            C = kernels.predict_cov(ch, J["X"], J["Xs"], J["beta"][a:b], J["s"][a:b],
                                    J["sp"][a:b], J["jit"][a:b], workspace=J["ws"])
            yield a, b, mean, C

    def _joint_draws(self, seed, offset, nsamp, mean_out=None) -> torch.Tensor:
        """(nsamp, S, m, P) joint draws: unit u = s P + j reads the normals of stream unit u."""
        S, P, m = self.S, self.P, self.m
        out = torch.empty((S * P, nsamp, m), dtype=F64, device=self.model.device)
        for a, b, mean, C in self._joint_groups(mean_out):
            info, _ = kernels.cholesky_inplace(C)
            kernels.check_joint_info(info, a, P, self.joint_jitter)
            kernels.mvn_draw(C, mean, seed, offset, nsamp, unit0=a, out=out[a:b])
        return out.reshape(S, P, nsamp, m).permute(2, 0, 3, 1).contiguous()

    def _need_joint(self, what: str) -> None:
        if getattr(self, "realized", False) != "joint" or self.mean_dev is None:
            raise ValueError(f"{what} needs a prediction made with realize='joint'")

    def cov(self, to_host: bool = True):
        """(S, P, m, m): the joint predictive covariance of the m test points per (sample, PC)
        (``joint_jitter`` s on the diagonal included), computed on demand, a group of units at a
        time (gp_predict_cov); ``to_host=False`` returns the device tensor."""
        self._need_joint("cov()")
        S, P, m = self.S, self.P, self.m
        if to_host:
            out = np.empty((S * P, m, m))
            for a, b, _, C in self._joint_groups():
                out[a:b] = C.cpu().numpy()
            return out.reshape(S, P, m, m)
        out = torch.empty((S * P, m, m), dtype=F64, device=self.model.device)
        for a, b, _, C in self._joint_groups():
            out[a:b] = C
        return out.reshape(S, P, m, m)

    def linear_functional(self, a):
        """Posterior mean a^T mu and variance a^T C a of a weighted sum over the test points
        per (sample, PC): ``a`` (m,) gives two (S, P) arrays, ``a`` (k, m) two (k, S, P) arrays
        (e.g. ``np.full(m, 1 / m)``: the average over the points).  The covariance is formed a
        group of units at a time and never held for all of them."""
        self._need_joint("linear_functional()")
        S, P, m = self.S, self.P, self.m
        dev = self.model.device
        A = torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)
        single = A.dim() == 1
        A = A.reshape(-1, m)
        k = A.shape[0]
        mu = torch.einsum("km,smp->ksp", A, self.mean_dev)
        var = torch.empty((k, S * P), dtype=F64, device=dev)
        for lo, hi, _, C in self._joint_groups():
            var[:, lo:hi] = torch.einsum("ki,uij,kj->ku", A, C, A)
        var = var.reshape(k, S, P)
        if single:
            mu, var = mu[0], var[0]
        return mu.cpu().numpy(), var.cpu().numpy()

    def _set_results(self, ctx, realize, seed, both, fill: bool = True) -> None:
        """The tail every prediction shares: ``both`` = (mean, var) of the (sample, PC) units in
        s-major order, each (S P, m) (None on the ranks that hold no result) -> the (S, m, P)
        device arrays and the state ``.w`` / ``get_y()`` / ``summary()`` work from."""
        S, P = self.S, self.P
        self.ctx = ctx
        self.realized = bool(realize)
        self.seed = int(np.random.SeedSequence().entropy & (2 ** 63 - 1)) if seed is None \
            else int(seed)
        self._w_dtype = np.dtype(np.float64)
        if both is None:
            self.mean_dev = self.w_dev = self.var_dev = None
            return
        if not fill:                      # joint mode fills the arrays after its own chain
            return
        mean_u, var_u = both
        # units are (s, j) in s-major order -> (S, P, m) -> (S, m, P)
        self.mean_dev = mean_u.reshape(S, P, self.m).permute(0, 2, 1).contiguous()
        self.var_dev = var_u.reshape(S, P, self.m).permute(0, 2, 1).contiguous()
        self.w_dev = (kernels.realize(self.mean_dev, self.var_dev, self.seed) if self.realized
                      else self.mean_dev)

    @property
    def w(self) -> np.ndarray:
        """(S, m, P) PC weights as the reference consumes ``.w`` (numpy): the posterior mean,
        or one marginal draw per entry with ``realize=True``, or whatever was assigned."""
        return None if self.w_dev is None else self.w_dev.cpu().numpy().astype(self._w_dtype,
                                                                              copy=False)

    @w.setter
    def w(self, value) -> None:
        """Assign the PC weights ``get_y()`` reconstructs from (the reference casts them with
        ``preds.w = preds.w.astype(np.float32)`` first): kept on the device as float64 copies of
        the assigned values; ``get_y()`` returns the assigned dtype."""
        a = np.asarray(value) if not torch.is_tensor(value) else value
        if tuple(a.shape) != (self.S, self.m, self.P):
            raise ValueError(f"w: expected shape {(self.S, self.m, self.P)}, got {tuple(a.shape)}")
        self._w_dtype = np.dtype(a.dtype if not torch.is_tensor(a) else
                                 torch.empty((), dtype=a.dtype).numpy().dtype)
        self.w_dev = _to_device_f64(a, self.model.device)

    @property
    def mean(self) -> np.ndarray:
        """(S, m, P) posterior mean of the PC weights."""
        return None if self.mean_dev is None else self.mean_dev.cpu().numpy()

    @property
    def var(self) -> np.ndarray:
        return None if self.var_dev is None else self.var_dev.cpu().numpy()

    def get_mu_sigma(self):
        return self.mean, self.var

    def sample_w(self, seed: int | None = None, offset: int = 1, joint: bool = False,
                 nsamp: int = 1) -> np.ndarray:
        """A fresh marginal realisation per (sample, point, PC), mean + sqrt(var) N(0, 1), on
        the device (gp_realize; ``offset`` selects an independent stream for one seed).
        ``joint=True`` (a prediction made with ``realize="joint"``): ``nsamp`` joint draws over
        the test points per (sample, PC), shape (nsamp, S, m, P) (gp_mvn_draw)."""
        seed = self.seed if seed is None else int(seed)
        if joint:
            self._need_joint("sample_w(joint=True)")
            if int(nsamp) < 1:
                raise ValueError("nsamp must be at least 1")
            return self._joint_draws(seed, offset, int(nsamp)).cpu().numpy()
        return kernels.realize(self.mean_dev, self.var_dev, seed, offset).cpu().numpy()

    def error_draws(self, rng=None, per_point: bool = True) -> np.ndarray:
        """Standardised residual error of the reference's predictions: one N(0, 1/sqrt(lamWOs_s))
        draw per posterior sample s (``time_predictions.py:84-87``) or per (sample, test point)
        (``per_point``, ``assess_all_models.py:493-497``), shape (S, m) / (S, 1).  The
        reference scales it by sd_y in physical units; get_y(add_error=True) does the same."""
        rng = np.random.default_rng() if rng is None else rng
        cols = self.m if per_point else 1
        return rng.standard_normal((self.S, cols)) / np.sqrt(self.lamWOs)[:, None]

    def get_y(self, std: bool = False, w=None, add_error: bool = False, rng=None,
              per_point: bool = True, ctx="inherit", gather: bool = True,
              to_host: bool = True):
        """Field reconstruction y = (w K) sd + mu, shape (S, m, ny) — SEPIA get_y().

        ``add_error`` adds the reference's PC-truncation error term (error_draws, times sd_y
        in physical units): y = (w K + e) sd + mu, one scalar e per (sample[, point]).

        Distributed (``ctx``, by default the prediction's; SURVEY §8e "field reconstruction"):
        rank 0's w (and error draws) are broadcast, rank r reconstructs the output columns
        ``shard_range(ny, r, N)`` with its slice of K, and with ``gather`` rank 0 receives the
        whole (S, m, ny) field (other ranks None); ``gather=False`` returns every rank's own
        (S, m, ny_r) column block (``self.y_cols`` holds its range).

        ``to_host=False`` returns the device tensor instead of numpy (no PCIe copy).  With at
        most gp_field_max_pcs() PCs the product, error term, back-transform and narrowing are
        one kernel (gp_field: every output element written once, in its final dtype).
        """
        sd_ = self.model.data.sim_data
        dev = self.model.device
        ctx = self.ctx if isinstance(ctx, str) else ctx
        dist_on = ctx is not None and ctx.distributed
        S, m, P = self.S, self.m, self.P
        if dist_on:
            flag = torch.tensor([1 if self._w_dtype == np.float32 else 0], device=dev)
            gdist.broadcast_(ctx, flag)
            f32 = bool(flag.item()) and w is None
            if ctx.rank == 0:
                wd = (self.w_dev if w is None else _to_device_f64(w, dev)).contiguous()
            else:
                wd = torch.empty((S, m, P), dtype=F64, device=dev)
            gdist.broadcast_(ctx, wd)
            ny = sd_.K.shape[1]
            c0, c1 = gdist.shard_range(ny, ctx.rank, ctx.world)
        else:
            f32 = w is None and self._w_dtype == np.float32
            wd = self.w_dev if w is None else _to_device_f64(w, dev)
            c0, c1 = 0, sd_.K.shape[1]
        out_dtype = np.float32 if f32 else np.float64
        self.y_cols = (c0, c1)
        e = None
        if add_error:
            cols = m if per_point else 1
            if not dist_on or ctx.rank == 0:
                e = torch.as_tensor(self.error_draws(rng, per_point), dtype=F64, device=dev)
            else:
                e = torch.empty((S, cols), dtype=F64, device=dev)
            if dist_on:
                gdist.broadcast_(ctx, e)
            e = (e.expand(S, m) if e.shape[1] == 1 else e).reshape(S * m).contiguous()
        mu = sd = None
        if not std:
            mu, sd = sd_.y_mean[c0:c1].contiguous(), sd_.y_sd[c0:c1].contiguous()
        y = self._field_rows(wd.reshape(S * m, P).contiguous(), c0, c1, sd, mu, e, f32)
        if dist_on and gather:
            counts = [gdist.shard_range(sd_.K.shape[1], r, ctx.world) for r in range(ctx.world)]
            y = gdist.gather_cols(ctx, y.contiguous(), [b - a for a, b in counts])
            if y is None:
                return None
        if not to_host:
            return y.reshape(S, m, -1)
        return _to_host(y.reshape(S, m, -1), out_dtype)

    def _field_rows(self, w2: torch.Tensor, c0: int, c1: int, sd, mu, e, f32: bool):
        """(w2 K[:, c0:c1] + e) sd + mu for rows x P weights (sd / mu None: standardised), on the
        device: gp_field up to gp_field_max_pcs() PCs, the generic GEMM + back-transform (fp64)
        beyond."""
        sd_ = self.model.data.sim_data
        rows, P = w2.shape
        if P <= blas.field_max_pcs():
            # one pass: y = (w K + e) sd + mu, written once in the output dtype (K's column
            # block read in place through its row stride)
            return blas.field(w2, sd_.K[:, c0:c1], sd, mu, e, f32=f32)
        K = sd_.K if (c0, c1) == (0, sd_.K.shape[1]) else sd_.K[:, c0:c1].contiguous()
        Wc = CM.of_rowmajor(w2)                              # (P x rows)
        Kc = CM.of_rowmajor(K)                               # (ny_r x P)
        Yc = gemm(False, False, Kc, Wc)                      # (ny_r x rows) = (w K)^T
        y = Yc.t[:rows, : c1 - c0]                           # (rows, ny_r) row-major
        if e is not None:
            y = y + e.reshape(rows, 1)                       # one scalar per row
        if sd is not None:
            y = blas.standardize(y.contiguous(), mu, sd, inverse=True)
        return y

    def summary(self, q=0.025, std: bool = False, add_error: bool = True, rng=None,
                per_point: bool = True, w=None, to_host: bool = True, out=None):
        """(mean, lower, upper), each (m, ny): the mean of get_y() and the q / 1 - q quantiles
        (``q`` a float, or a pair (q_lo, q_hi)) of get_y() + error over the posterior samples --
        the loop body of assess_all_models.py:489-500 / plot_test_error.py:77-87 -- without the
        (S, m, ny) field: one kernel (gp_field_summary) reads w and K once and writes the three
        (m, ny) arrays.

        The error draws are get_y(add_error=True, rng=..., per_point=...)'s (one error_draws call:
        the same seed gives the same draws); the mean carries no error term, as in the reference.
        The dtype follows get_y(): float32 after ``preds.w = preds.w.astype(np.float32)``.
        ``out``: three device tensors (m, ny) of that dtype to write into; ``to_host=False``
        returns device tensors.  With more than gp_field_max_pcs() PCs, or a tail deeper than
        gp_field_summary_max_tail() order statistics, the field is built (fp64) in blocks of test
        points of at most 1 GiB and reduced with torch.sort / mean: the same results to rounding.
        Distributed predictions: computed on rank 0 (which holds w), None on the other ranks."""
        ctx = self.ctx
        if ctx is not None and ctx.distributed and ctx.rank != 0:
            return None
        sd_ = self.model.data.sim_data
        dev = self.model.device
        m, ny = self.m, sd_.K.shape[1]
        wd, sd, mu, e, q_lo, q_hi, f32 = self._summary_inputs("summary", q, std, add_error, rng,
                                                              per_point, w)
        dt = torch.float32 if f32 else F64
        if out is None:
            out = tuple(torch.empty((m, ny), dtype=dt, device=dev) for _ in range(3))
        if self._summary_fused(q_lo, q_hi):
            blas.field_summary(wd, sd_.K, sd, mu, e, q=(q_lo, q_hi), f32=f32, out=out)
        else:
            self._summary_blocks(wd, sd, mu, e, q_lo, q_hi, out)
        if not to_host:
            return out
        return tuple(_to_host(t, np.float32 if f32 else np.float64) for t in out)

    def _summary_inputs(self, fn, q, std, add_error, rng, per_point, w):
        """The operands summary() and score() hand to the kernel: (w (S, m, P) fp64 on the
        device, sd, mu, the S m error scalars or None, q_lo, q_hi, float32 outputs?).  One
        error_draws call: the same ``rng`` gives the same draws in both and in get_y()."""
        sd_ = self.model.data.sim_data
        dev = self.model.device
        S, m = self.S, self.m
        f32 = w is None and self._w_dtype == np.float32
        wd = (self.w_dev if w is None else _to_device_f64(w, dev)).contiguous()
        q_lo, q_hi = blas._band(q)
        if not (0.0 <= q_lo <= q_hi <= 1.0):
            raise ValueError(f"{fn}: need 0 <= q_lo <= q_hi <= 1, got ({q_lo}, {q_hi})")
        e = None
        if add_error:
            e = torch.as_tensor(self.error_draws(rng, per_point), dtype=F64, device=dev)
            e = (e.expand(S, m) if e.shape[1] == 1 else e).reshape(S * m).contiguous()
        mu = sd = None
        if not std:
            mu, sd = sd_.y_mean.contiguous(), sd_.y_sd.contiguous()
        return wd, sd, mu, e, q_lo, q_hi, f32

    def _summary_fused(self, q_lo, q_hi) -> bool:
        """Whether gp_field_summary / gp_field_score take this prediction (PCs and tail depth)."""
        return self.P <= blas.field_max_pcs() and \
            max(blas.summary_tail_depths(self.S, q_lo, q_hi)) <= blas.field_summary_max_tail()

    def score(self, y_true, q=0.025, mape_floor=None, std: bool = False, add_error: bool = True,
              rng=None, per_point: bool = True, w=None, maps: bool = False,
              to_host: bool = True, cols: bool = True):
        """Test-error scores of summary(q, ...) against ``y_true`` (m, ny) -- RMSE, MAPE, mean
        quantiles, coverage per test point and RMSE, coverage, band width per node, the block
        assess_all_models.py:524-552 and plot_integrated_RMSE.py:108-116 compute from three
        (m, ny) arrays -- as a :class:`gladsgp_amd.score.FieldScore`, in summary()'s one pass and
        without the arrays: the kernel (gp_field_score) writes m x 8 and ny x 4 sums.

        ``y_true``: numpy or a device tensor, float32 or float64 (a host array is uploaded in its
        own dtype), NaN where there is no truth; None scores the prediction alone (mean
        quantiles and widths: the integration-point loop of assess_all_models.py:504-521).
        ``mape_floor``: absolute percentage errors count where ``not (y < mape_floor)`` (the
        reference's ``inner_mape[y_test < lq] = nan``); None counts every valid element.  q, std,
        add_error, rng, per_point, w and the float32 rule are summary()'s: the same ``rng`` gives
        the same error draws.  ``maps=True`` also returns summary()'s three arrays (``.maps``),
        the same bits, from the same pass.  Cross-validated predictions leave the simulations in no
        fold (NaN weights) out of the pass: their rows are NaN with zero counts, they enter no
        per-node sum, and the per-node means are over the ``n_scored`` other points.  ``to_host=False`` keeps the raw sums and maps on the device.
        Beyond the kernel's limits (PCs, tail depth) the maps are built as summary() builds them
        and reduced with torch: the same results to rounding.  Distributed predictions: computed
        on rank 0, None on the other ranks."""
        from . import score as gscore
        ctx = self.ctx
        if ctx is not None and ctx.distributed and ctx.rank != 0:
            return None
        sd_ = self.model.data.sim_data
        dev = self.model.device
        S, m, P = self.S, self.m, self.P
        ny = sd_.K.shape[1]
        wd, sd, mu, e, q_lo, q_hi, f32 = self._summary_inputs("score", q, std, add_error, rng,
                                                              per_point, w)
        Y = None
        if y_true is not None:
            Y = y_true if torch.is_tensor(y_true) else torch.as_tensor(np.asarray(y_true))
            if Y.dtype not in (torch.float32, F64):
                Y = Y.to(F64)
            if tuple(Y.shape) != (m, ny):
                raise ValueError(f"score: y_true must be {(m, ny)}, got {tuple(Y.shape)}")
            Y = Y.to(dev)
            if ny > 1 and Y.stride(1) != 1:
                Y = Y.contiguous()
        floor = -np.inf if mape_floor is None else float(mape_floor)
        keep = self._points_with_prediction(wd)
        part = keep is not None and not bool(keep.all())
        if part:
            wd = wd[:, keep].contiguous()
            e = None if e is None else e.reshape(S, m)[:, keep].reshape(-1).contiguous()
            Y = None if Y is None else Y[keep]
        mk = wd.shape[1]
        dt = torch.float32 if f32 else F64
        fused = self._summary_fused(q_lo, q_hi)
        out = None
        if maps or not fused:
            out = tuple(torch.empty((mk, ny), dtype=dt, device=dev) for _ in range(3))
        if fused:
            res = blas.field_score(wd, sd_.K, sd, mu, e, Y, q=(q_lo, q_hi), mape_floor=floor,
                                   f32=f32, out=out, cols=cols)
            rows, colt = res[0], res[1]
        else:
            self._summary_blocks(wd, sd, mu, e, q_lo, q_hi, out)
            rows, colt = gscore.sums_from_maps(*out, Y, floor, cols=cols)
        if part:
            rows = gscore.rows_without_prediction(rows, keep, m)
            if maps:
                full = tuple(torch.full((m, ny), float("nan"), dtype=dt, device=dev)
                             for _ in range(3))
                for f, o in zip(full, out):
                    f[keep] = o
                out = full
        if to_host:
            rows = rows.cpu().numpy()
            colt = None if colt is None else colt.cpu().numpy()
            if maps:
                out = tuple(_to_host(t, np.float32 if f32 else np.float64) for t in out)
        return gscore.FieldScore(rows, colt, ny, out if maps else None, n_scored=mk)

    def _points_with_prediction(self, wd):
        """score(): a bool (m,) mask of the test points to score, or None for all of them.  Every
        point of an ordinary prediction has weights, so nothing is looked at here;
        EmulatorXvalPrediction leaves out the simulations in no fold."""
        return None

    def _summary_blocks(self, wd, sd, mu, e, q_lo, q_hi, out) -> None:
        """summary()'s generic route: the fp64 field of a block of test points (at most 1 GiB),
        its mean and, from the sorted samples, numpy's linear-rule quantiles."""
        S, m, P = wd.shape
        ny = self.model.data.sim_data.K.shape[1]
        mb = max(1, (1 << 30) // max(1, 8 * S * ny))
        ev = None if e is None else e.reshape(S, m)
        for a in range(0, m, mb):
            b = min(m, a + mb)
            w2 = wd[:, a:b].reshape(S * (b - a), P).contiguous()
            y = self._field_rows(w2, 0, ny, sd, mu, None, False).reshape(S, b - a, ny)
            out[0][a:b] = y.mean(dim=0)
            if ev is not None:
                del y
                eb = ev[:, a:b].reshape(S * (b - a)).contiguous()
                y = self._field_rows(w2, 0, ny, sd, mu, eb, False).reshape(S, b - a, ny)
            z = torch.sort(y, dim=0).values
            del y
            for qq, dst in ((q_lo, out[1]), (q_hi, out[2])):
                pos = qq * (S - 1)
                j = int(np.floor(pos))
                t = pos - j
                lo_v, hi_v = z[j], z[min(j + 1, S - 1)]
                d = hi_v - lo_v
                dst[a:b] = lo_v + d * t if t < 0.5 else hi_v - d * (1.0 - t)


def assemble_units(ctx, mean_l: torch.Tensor, var_l: torch.Tensor, n_units: int):
    """Gather per-rank (mean, var) rows of round-robin-dealt units back into unit order.

    Single process: identity.  Distributed: one gather to rank 0 (RCCL on GPUs, gloo on CPU);
    returns None on the other ranks.
    """
    if ctx is None or not ctx.distributed:
        return mean_l, var_l
    world = ctx.world
    m = mean_l.shape[1]
    counts = [len(gdist.shard_units(n_units, r, world)) for r in range(world)]
    both = torch.stack([mean_l, var_l], dim=1) if mean_l.shape[0] else \
        torch.empty((0, 2, m), dtype=mean_l.dtype, device=mean_l.device)
    allb = gdist.gather_rows(ctx, both, counts)
    if allb is None:
        return None
    allb = unit_order(allb, n_units, world)
    return allb[:, 0], allb[:, 1]


def assemble_points(ctx, mean_l: torch.Tensor, var_l: torch.Tensor, m: int):
    """Gather every rank's (U, m_r) test-point block of all units to rank 0 as (U, m) x 2
    (one gather; None on the other ranks)."""
    if ctx is None or not ctx.distributed:
        return mean_l, var_l
    counts = [b - a for a, b in (gdist.shard_range(m, r, ctx.world) for r in range(ctx.world))]
    both = torch.stack([mean_l, var_l], dim=0).contiguous()   # (2, U, m_r)
    allb = gdist.gather_cols(ctx, both, counts)
    if allb is None:
        return None
    return allb[0], allb[1]


def unit_order(rank_major: torch.Tensor, n_units: int, world: int) -> torch.Tensor:
    """Rows gathered rank by rank (rank r's round-robin units shard_units(n_units, r, world) in
    order) -> rows in unit order."""
    order = np.concatenate([gdist.shard_units(n_units, r, world) for r in range(world)])
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    return rank_major[torch.as_tensor(inv, device=rank_major.device)]


class EmulatorXvalPrediction(EmulatorPrediction):
    """Cross-validated predictions of the n training simulations (SEPIA's
    SepiaXvalEmulatorPrediction, assess_all_models.py:32, include_trunc_error.py:15): for every
    fold F of ``leave_out_inds`` (a list of index lists; None = leave-one-out) and every
    (sample, PC) GP, E[w_F | the other simulations] and its marginal variance, with the
    hyperparameters, the PCA basis and w_hat of the full model (SEPIA refits neither per fold).

    SEPIA refits one sub-model per fold; here each group of units is one gram -> potrf_inv ->
    xval (gp_xval: every fold in closed form from L^-1).  The result is an
    :class:`EmulatorPrediction` whose m = n points are the training simulations: row i of ``.w``
    / ``.mean`` / ``.var`` is simulation i (rows in no fold are NaN), and ``get_y()`` /
    ``summary()`` give the cross-validated field.  The variance is the one EmulatorPrediction
    reports at a new point placed at t_i (``pred_nugget`` as there).  Folds hold at most
    kernels.xval_max_fold() simulations.  Single device: ``ctx`` must be None."""

    def __init__(self, leave_out_inds=None, model: EmulatorModel = None, samples: dict = None,
                 pred_nugget: bool = True, budget_bytes: int = 2 << 30,
                 group: int | None = None, ctx=None, realize: bool = False,
                 seed: int | None = None):
        if ctx is not None:
            raise ValueError("ctx: cross-validation is not sharded over devices (pass None)")
        if model is None or samples is None:
            raise ValueError("EmulatorXvalPrediction needs model and samples")
        self.model = model
        dev = model.device
        X = model.data.sim_data.t_dev
        n = model.n
        beta, s, delta, sp = gp_params(samples, _np(model.LamSim), model.d, model.P, pred_nugget)
        S, P = s.shape
        self.S, self.m, self.P = S, n, P
        self.shard = "units"
        self.lamWOs = np.asarray(samples["lamWOs"], dtype=np.float64).reshape(S)
        self.leave_out_inds = None if leave_out_inds is None else \
            [[int(i) for i in np.atleast_1d(f)] for f in leave_out_inds]
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)  # noqa
        # units (s, j) in s-major order
        beta_u, s_u, delta_u = t(beta.reshape(S * P, -1)), t(s.reshape(-1)), t(delta.reshape(-1))
        shift_u = t((s + delta - sp).reshape(-1))
        w_hat = model.w_hat.transpose(0, 1).contiguous()       # (P, n)
        w_u = w_hat.repeat(S, 1)                               # (S P, n)
        U = S * P
        npad = kernels.padded_n(n)
        g = max(1, int(budget_bytes // (8 * (n * n + npad * npad))))
        if group is not None:
            g = max(1, min(g, int(group)))
        mean = torch.full((U, n), float("nan"), dtype=F64, device=dev)
        var = torch.full((U, n), float("nan"), dtype=F64, device=dev)
        for a in range(0, U, g):
            b = min(U, a + g)
            ch = kernels.cholesky_inverse(kernels.gram(X, beta_u[a:b], s_u[a:b], delta_u[a:b],
                                                       batch=b - a))
            ch.check()
            kernels.xval(ch, w_u[a:b], self.leave_out_inds, shift_u[a:b],
                         out=(mean[a:b], var[a:b]))
        self.shift_dev = shift_u.reshape(S, 1, P)
        self._set_results(None, realize, seed, (mean, var))

    def score(self, y_true=None, q=0.025, mape_floor=None, std: bool = False, **kw):
        """EmulatorPrediction.score() of the cross-validated field against the training
        simulations themselves (``y_true`` None: sim_data.y, or the standardised y_std with
        ``std``): include_trunc_error.py's and assess_all_models.py:32's use of the
        cross-validated predictions.  Simulations in no fold have NaN rows and zero counts and
        are left out of the per-node statistics.  Because None selects the training simulations
        here, the prediction-only score of the base class (no truth at all) is not reachable
        through this method: call ``EmulatorPrediction.score(xval, None, ...)`` for it."""
        if y_true is None:
            sd_ = self.model.data.sim_data
            y_true = sd_.y_std if std else sd_.y_dev       # sim_data.y, already on the device
        return super().score(y_true, q=q, mape_floor=mape_floor, std=std, **kw)

    def _points_with_prediction(self, wd):
        return ~torch.isnan(wd).any(dim=2).any(dim=0)

    @property
    def standardized_residuals(self) -> np.ndarray:
        """(S, n, P): (w_hat - mean) / sqrt(var + shift), the PC-space residual of every
        held-out simulation in units of the spread of the observed w_hat_i (shift = s + delta -
        s_pred takes the predictive variance back to that of the observation)."""
        w_hat = self.model.w_hat.unsqueeze(0)                  # (1, n, P)
        r = (w_hat - self.mean_dev) / torch.sqrt(self.var_dev + self.shift_dev)
        return r.cpu().numpy()


# SEPIA-compatible aliases for drop-in call sites
SepiaEmulatorPrediction = EmulatorPrediction
SepiaXvalEmulatorPrediction = EmulatorXvalPrediction


def default_data_dir():
    return os.path.join(os.getcwd(), "data")
