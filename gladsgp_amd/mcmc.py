"""Metropolis fit of the sim-only GPMSA emulator on the GPU (SEPIA's do_mcmc / tune_step_sizes).

Reference usage replaced (``src/model.py:218-238``)::

    model.params.lamWOs = SepiaParam(val=pc_prec, name='lamWOs', val_shape=(1, 1),
        dist='Gamma', params=[50, 50/pc_prec], bounds=[1., np.inf], mcmcStepParam=10,
        mcmcStepType='Uniform')
    model.params.mcmcList = [model.params.betaU, model.params.lamUz, model.params.lamWs,
                             model.params.lamWOs]
    model.tune_step_sizes(100, 5)
    model.do_mcmc(512)

SEPIA (``timghill/SEPIA@ffe3b60``) is not available offline, so the
sampler is restated from the GPMSA model it implements; every constant below that the
reference's own files do not pin is marked *unpinned*.

Model (per principal component j = 0..P-1, one GP each, w_hat_j = PC weights of the n runs)::

    Sigma_j = (1/lamUz_j) exp(-sum_k betaU[k+1, j] (t_ik - t_i'k)^2)
              + (1/lamWs_j + 1/(lamWOs LamSim_j)) I
    loglik  = sum_j  -1/2 log|Sigma_j| - 1/2 w_hat_j^T Sigma_j^-1 w_hat_j           

betaU is (d+1, P); row 0 belongs to the dummy x input, whose differences are all zero, so it
only moves under its prior (the reference's sample layout ``(S, (d+1) P)``, C order,
``mcmc_diagnostics_advanced.py:57``).

Priors (log densities up to constants) and proposals:

  ===========  ===================================  ==========  ===========  ============
  param        prior                                bounds      step (dflt)  step type
  ===========  ===================================  ==========  ===========  ============
  betaU        Beta(1, 0.1) on rho = exp(-beta/4)   [0, inf)    0.1          BetaRho
  lamUz        Gamma(5, 5)                          [0.3, inf)  5            Uniform
  lamWs        Gamma(3, 0.003)                      [60, 1e5]   100          Uniform
  lamWOs       Gamma(5, 0.005); the reference       [60, 1e5]   100          Uniform
               overrides it with Gamma(50, 50/pc_prec), [1, inf), step 10 (model.py:225-229)
  ===========  ===================================  ==========  ===========  ============

The default step sizes are pinned by ``examples/03...ipynb:192-208``; the prior families,
parameters and bounds are the GPMSA defaults and are *unpinned*.  Gamma is (shape, rate).
Proposals: ``Uniform`` x' = x + step (u - 1/2); ``BetaRho`` the same move on rho, then
beta' = -4 log rho'.  A proposal outside the bounds is rejected.  Acceptance:
log u < log post(x') - log post(x).

Sweep (one MCMC iteration) = component-wise Metropolis over mcmcList in order: betaU row by
row, then lamUz, lamWs, lamWOs.  Given lamWOs the P GPs are independent, so the P elements of
one betaU row (or of lamUz, lamWs) are proposed together and accepted or rejected one by one:
that is the same Markov kernel as updating them one after another, evaluated as ONE batched
gp_loglik (Gram -> Cholesky -> quadratic form for the P GPs).  lamWOs touches every GP and is
accepted on the sum.  The whole sweep is stream-ordered device work: no host synchronisation,
proposals and accept/reject are device tensor ops on uniforms drawn on the host from a seeded
numpy Generator (so a CPU restatement fed the same uniforms reproduces the chain).

tune_step_sizes(n_burn, n_levels): after n_burn burn-in sweeps at the default steps, for each
level l the steps are default * 2^e_l, e_l evenly spaced in [-(n_levels-1)/2, (n_levels-1)/2];
n_burn sweeps are run at each level continuing the chain, acceptances are counted per element, and a binomial logistic regression of acceptance on
log(step) gives the step whose predicted acceptance is 1/e (logit = log(1/(e-1))), anchored by
one pseudo-acceptance far below and one pseudo-rejection far above the ladder so that a
parameter accepted (or rejected) at every level still gets an extrapolated step; the result
is clamped to the anchors' span, to 1 for BetaRho moves (rho lives in (0, 1]) and to the bound
width for a bounded parameter.  Burn-in, ladder base, target, regularisation and clamps are
*unpinned* (GPMSA's stepsize procedure).
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _capi, kernels

F64 = torch.float64
TARGET_LOGIT = math.log(1.0 / (math.e - 1.0))   # acceptance 1/e
RHO_MAX = 0.999                                  # rho clipped in the Beta prior (beta -> 0)


class SepiaParam:
    """One model parameter: value, prior and Metropolis step (SEPIA's SepiaParam surface).

    Signature as the reference calls it (``src/model.py:225-229``).
    """

    def __init__(self, val, name, val_shape, dist="Normal", params=None, bounds=None,
                 mcmcStepParam=0.1, mcmcStepType="Uniform", fixed=None):
        self.name = name
        self.val_shape = tuple(val_shape)
        self.val = np.broadcast_to(np.asarray(val, dtype=np.float64), self.val_shape).copy()
        if dist not in ("Gamma", "Beta", "Uniform", "Normal"):
            raise ValueError(f"unsupported prior {dist!r}")
        self.dist = dist
        self.params = [float(p) for p in (params if params is not None else [0.0, 1.0])]
        b = bounds if bounds is not None else [-np.inf, np.inf]
        self.bounds = (float(b[0]), float(b[1]))
        self.mcmcStepParam = np.broadcast_to(np.asarray(mcmcStepParam, dtype=np.float64),
                                             self.val_shape).copy()
        if mcmcStepType not in ("Uniform", "BetaRho"):
            raise ValueError(f"unsupported step type {mcmcStepType!r}")
        self.mcmcStepType = mcmcStepType
        self.fixed = np.zeros(self.val_shape, bool) if fixed is None else np.asarray(fixed, bool)

    def __repr__(self):
        return (f"SepiaParam({self.name}, shape={self.val_shape}, {self.dist}{self.params}, "
                f"bounds={self.bounds}, step={self.mcmcStepType})")


class ModelParams:
    """``model.params``: attributes betaU, lamUz, lamWs, lamWOs and ``mcmcList``."""

    names = ("betaU", "lamUz", "lamWs", "lamWOs")

    def __init__(self, d: int, P: int):
        # GPMSA / SEPIA defaults (step sizes pinned by 03...ipynb:192-208; the rest unpinned)
        self.betaU = SepiaParam(0.1, "betaU", (d + 1, P), "Beta", [1.0, 0.1], [0.0, np.inf],
                                0.1, "BetaRho")
        self.lamUz = SepiaParam(1.0, "lamUz", (1, P), "Gamma", [5.0, 5.0], [0.3, np.inf],
                                5.0, "Uniform")
        self.lamWs = SepiaParam(1000.0, "lamWs", (1, P), "Gamma", [3.0, 0.003], [60.0, 1e5],
                                100.0, "Uniform")
        self.lamWOs = SepiaParam(1000.0, "lamWOs", (1, 1), "Gamma", [5.0, 0.005], [60.0, 1e5],
                                 100.0, "Uniform")
        self.mcmcList = [self.betaU, self.lamUz, self.lamWs, self.lamWOs]

    def __getitem__(self, name):          # dict-style access to values
        return getattr(self, name).val

    def __setitem__(self, name, value):
        p = getattr(self, name)
        p.val = np.broadcast_to(np.asarray(value, dtype=np.float64), p.val_shape).copy()

    def values(self) -> dict:
        return {k: getattr(self, k).val.copy() for k in self.names}


# ------------------------------------------------------------------------------ priors (torch)
def log_prior(p: SepiaParam, x: torch.Tensor) -> torch.Tensor:
    """Elementwise log prior density of parameter ``p`` at values ``x`` (device tensor)."""
    a, b = p.params
    if p.dist == "Gamma":
        return (a - 1.0) * torch.log(x) - b * x
    if p.dist == "Beta":                    # on rho = exp(-x / 4)
        rho = torch.clamp(torch.exp(-x / 4.0), max=RHO_MAX)
        return (a - 1.0) * torch.log(rho) + (b - 1.0) * torch.log1p(-rho)
    if p.dist == "Normal":
        return -0.5 * ((x - a) / b) ** 2
    return torch.zeros_like(x)              # Uniform on the bounds


def propose(p: SepiaParam, x: torch.Tensor, step: torch.Tensor, u: torch.Tensor):
    """Candidate values and in-bounds mask for a Metropolis move of ``p``."""
    if p.mcmcStepType == "BetaRho":
        rho = torch.exp(-x / 4.0) + step * (u - 0.5)
        ok = (rho > 0.0) & (rho <= 1.0)
        cand = -4.0 * torch.log(torch.where(ok, rho, torch.ones_like(rho)))
    else:
        cand = x + step * (u - 0.5)
        ok = torch.ones_like(cand, dtype=torch.bool)
    lo, hi = p.bounds
    ok = ok & (cand >= lo) & (cand <= hi)
    return torch.where(ok, cand, x), ok


# --------------------------------------------------------------------------- device sampler
@dataclass
class ChainState:
    """Device-resident chain state; updated in place so a captured sweep graph stays valid."""

    betaU: torch.Tensor        # (d+1, P)
    lamUz: torch.Tensor        # (P,)
    lamWs: torch.Tensor        # (P,)
    lamWOs: torch.Tensor       # (1,)
    ll: torch.Tensor           # (P,) current per-GP log-likelihood
    acc: dict = field(default_factory=dict)   # per-element acceptance counters (device)


def uniforms_per_sweep(d: int, P: int) -> int:
    """Uniform draws one sweep consumes: (proposal, acceptance) per updated element."""
    return 2 * ((d + 1) * P + 2 * P + 1)


def default_spec(n: int, P: int, updates: int) -> int:
    """Speculative group size with the least modelled sweep time: ceil(updates / s) batched
    gp_loglik calls of (2^s - 1) P problems each, a call costing the longer of the
    factorisation's chain (~25 us per 64-column step) and its work (~4.8 us per n = 512 problem,
    scaled by n^3).  Fitted on MI355X (profiles/r06/r06al_ab_spec.log: 24 problems 0.21 ms, 56
    0.26, 120 0.58 at n = 512); it picks spec 3 at the fit's n = 512, P = 8.  Speed only: every
    spec gives the same chain."""
    def sweep(s):
        call = max(0.025 * -(-n // 64), 0.0048 * (2 ** s - 1) * P * (n / 512.0) ** 3)
        return -(-updates // s) * call
    return min(range(1, _capi.MCMC_MAX_GROUP + 1), key=sweep)


class _ChainSweeps:
    """What GPUSampler (one chain) and EnsembleSampler (many) share: C chains on one design
    X (n, d), each with its own PC weights ``w[c]`` (P, n), ``lam[c]`` (P,), state, step sizes,
    counters and uniforms (``params[c]``: a ModelParams holding chain c's values and steps), all
    in static device buffers with a leading chain axis, and the fused sweep over them: one
    gp_mcmc_ens_* launch of C workgroups around each batched gp_loglik of all chains' state sets
    (csrc/mcmc.hip), run eagerly, as a replayed HIP graph of one sweep, or in graphs of
    ``block`` sweeps.

    The batch is chain-major, and gp_loglik is issued in slices of whole chains of at most
    ``max_batch`` problems (None: all chains in one call).  Slices of equal size share one
    workspace (the workspace's layout depends on its batch, so sizes cannot share).  A chain's
    results do not depend on the others: the kernels touch one chain's memory per workgroup, and a
    likelihood does not depend on the batch it is evaluated in.
    """

    def __init__(self, X: torch.Tensor, w: torch.Tensor, lam: torch.Tensor, params: list,
                 use_graph: bool | None, spec: int, fused: bool, max_batch: int | None):
        self.X = X.contiguous()
        self.dev = self.X.device
        self.C, self.P, self.n = w.shape                                # w: (C, P, n)
        self.d = self.X.shape[1]
        self._params = params
        C, P, d = self.C, self.P, self.d
        self.lam = lam.to(self.dev, F64).reshape(C, P).contiguous()
        self.nu = uniforms_per_sweep(d, P)
        self.u = torch.zeros((C, self.nu), dtype=F64, device=self.dev)   # static uniforms
        self.steps = {k: torch.zeros((C,) + getattr(params[0], k).val_shape, dtype=F64,
                                     device=self.dev) for k in ModelParams.names}
        self.set_steps(1.0)
        # the recorded state, one flat row per chain: betaU (d+1, P) | lamUz | lamWs | lamWOs |
        # log post (so a sample is recorded with one copy)
        self._cols = {"betaU": (0, (d + 1) * P)}
        o = (d + 1) * P
        for k, w_ in (("lamUz", P), ("lamWs", P), ("lamWOs", 1), ("logPost", 1)):
            self._cols[k] = (o, o + w_)
            o += w_
        self._flat = torch.zeros((C, o), dtype=F64, device=self.dev)
        self._ll = torch.zeros((C, P), dtype=F64, device=self.dev)      # per-GP log-likelihood
        # acceptance counters indexed by update code (gp_mcmc_state.acc)
        self._acc = torch.zeros((C, d + 4, P), dtype=F64, device=self.dev)
        self._scratch = torch.zeros((C, 3 * _capi.MCMC_MAX_GROUP * P), dtype=F64,
                                    device=self.dev)
        self.st = None
        if use_graph is None:
            use_graph = os.environ.get("GPFIT_MCMC_GRAPH", "1") == "1"
        self.use_graph = bool(use_graph) and self.dev.type == "cuda"
        self.graph = None
        # sweeps per replayed graph in run() (GPFIT_MCMC_BLOCK; 1: one sweep per replay)
        self.block = max(1, int(os.environ.get("GPFIT_MCMC_BLOCK", "16")))
        # decide + next prep in one launch (gp_mcmc_ens_step); GPFIT_MCMC_MERGE=0: two
        self._merge = os.environ.get("GPFIT_MCMC_MERGE", "1") == "1"
        self._bgraph = {}
        self.fused = fused
        self.spec = spec
        self.max_batch = max_batch
        # the likelihood-changing updates of a sweep by update code, in mcmcList order: betaU
        # rows 1 .. d, lamUz, lamWs, lamWOs (betaU row 0, the dummy x, moves under its prior
        # alone)
        codes = list(range(1, d + 4))
        self.groups = [codes[i:i + spec] for i in range(0, len(codes), spec)]
        self._ws = {}
        self._gbuf = {}
        for sets in {1} | {2 ** len(g) - 1 for g in self.groups}:   # 1: init_state's call
            R = sets * P
            self._gbuf[sets] = dict(
                chunk=C if max_batch is None else max(1, max_batch // R),
                beta=torch.empty((C * R, d), dtype=F64, device=self.dev),
                s=torch.empty(C * R, dtype=F64, device=self.dev),
                delta=torch.empty(C * R, dtype=F64, device=self.dev),
                ll=torch.empty(C * R, dtype=F64, device=self.dev),
                w=w[:, None].expand(C, sets, P, self.n).reshape(C * R, self.n).contiguous())
            for c0 in range(0, C, self._gbuf[sets]["chunk"]):
                B = (min(C, c0 + self._gbuf[sets]["chunk"]) - c0) * R
                if B not in self._ws:
                    self._ws[B] = kernels.LoglikWorkspace(self.n, B, self.dev)
        T = self._T = _capi.McmcStrides()
        T.betaU = T.lamUz = T.lamWs = T.lamWOs = T.lp = self._flat.shape[1]
        T.ll, T.lam, T.u, T.acc, T.scratch = P, P, self.nu, (d + 4) * P, self._scratch.shape[1]
        T.step_betaU, T.step_lamUz, T.step_lamWs, T.step_lamWOs = (d + 1) * P, P, P, 1
        self._kinds = [(ctypes.c_int * len(g))(*g) for g in self.groups]

    def _t(self, a) -> torch.Tensor:
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.dev)

    def _view(self, name: str) -> torch.Tensor:
        a, b = self._cols[name]
        return self._flat[:, a:b]

    # -- state (per chain) ---------------------------------------------------------------
    def init_state(self):
        """Every chain's state from its params' current values, ll from one sliced gp_loglik."""
        C, P, d = self.C, self.P, self.d
        for k in ModelParams.names:
            self._view(k).copy_(self._t(np.stack([getattr(pr, k).val.reshape(-1)
                                                  for pr in self._params])))
        buf = self._gbuf[1]
        betaU = self._view("betaU").reshape(C, d + 1, P)
        buf["beta"].view(C, P, d).copy_(betaU[:, 1:].transpose(1, 2))
        torch.reciprocal(self._view("lamUz"), out=buf["s"].view(C, P))
        torch.add(torch.reciprocal(self._view("lamWs")),
                  torch.reciprocal(self._view("lamWOs") * self.lam), out=buf["delta"].view(C, P))
        self._loglik(1)
        self._ll.copy_(buf["ll"].view(C, P))
        if self.st is None:
            self.st = self._flat                # the states: one flat row per chain
        self.reset_counts()

    def reset_counts(self) -> None:
        self._acc.zero_()

    def _counts(self) -> list:
        """Per chain, the acceptance counts by update: ("betaU", row), lamUz, lamWs (P,) and
        lamWOs (1,)."""
        a, d = self._acc.cpu().numpy(), self.d
        out = []
        for c in range(self.C):
            cnt = {("betaU", k): a[c, k].copy() for k in range(d + 1)}
            cnt.update({"lamUz": a[c, d + 1].copy(), "lamWs": a[c, d + 2].copy(),
                        "lamWOs": a[c, d + 3, :1].copy()})
            out.append(cnt)
        return out

    def set_steps(self, scale: float = 1.0) -> None:
        for k in ModelParams.names:
            self.steps[k].copy_(self._t(np.stack([getattr(pr, k).mcmcStepParam * scale
                                                  for pr in self._params])))

    def write_back(self) -> None:
        flat = self._flat.cpu().numpy()
        for c, pr in enumerate(self._params):
            for k in ModelParams.names:
                a, b = self._cols[k]
                p = getattr(pr, k)
                p.val = flat[c, a:b].reshape(p.val_shape).copy()

    # -- one sweep -----------------------------------------------------------------------
    def _loglik(self, sets: int) -> None:
        """gp_loglik over the chain-major batch of ``sets`` state sets per chain, in slices of
        whole chains."""
        buf, R = self._gbuf[sets], sets * self.P
        for c0 in range(0, self.C, buf["chunk"]):
            r0, r1 = c0 * R, min(self.C, c0 + buf["chunk"]) * R
            kernels.loglik(self.X, buf["beta"][r0:r1], buf["s"][r0:r1], buf["delta"][r0:r1],
                           buf["w"][r0:r1], self._ws[r1 - r0], out=buf["ll"][r0:r1])

    def _state_struct(self) -> "_capi.McmcState":
        """gp_mcmc_state of chain 0 over the static buffers and the shared priors (self._T: the
        strides to the other chains)."""
        pr = self._params[0]
        S = _capi.McmcState()
        for nm, t in (("betaU", self._view("betaU")), ("lamUz", self._view("lamUz")),
                      ("lamWs", self._view("lamWs")), ("lamWOs", self._view("lamWOs")),
                      ("ll", self._ll), ("lam", self.lam), ("u", self.u),
                      ("step_betaU", self.steps["betaU"]), ("step_lamUz", self.steps["lamUz"]),
                      ("step_lamWs", self.steps["lamWs"]), ("step_lamWOs", self.steps["lamWOs"]),
                      ("acc", self._acc), ("lp", self._view("logPost")),
                      ("scratch", self._scratch)):
            if t.dtype != F64:
                raise TypeError(f"mcmc state buffer {nm} must be float64")
            setattr(S, nm, t.data_ptr())
        if not self.u.is_contiguous() or self.u.shape != (self.C, self.nu):
            raise TypeError("uniforms must be a contiguous (C, nu) block")
        S.P, S.d = self.P, self.d
        for i, nm in enumerate(ModelParams.names):
            p = getattr(pr, nm)
            S.dist[i] = _capi.MCMC_DIST[p.dist]
            S.steptype[i] = _capi.MCMC_STEP[p.mcmcStepType]
            S.pa[i], S.pb[i] = p.params
            S.lo[i], S.hi[i] = p.bounds
        return S

    def _sweep(self) -> None:
        """One component-wise Metropolis sweep of every chain on the static buffers (graph-
        capturable: no allocation that outlives it, no host synchronisation, in-place state
        updates), each speculative group's proposals and decisions in one-workgroup-per-chain
        kernels around its gp_loglik (csrc/mcmc.hip): the first group's gp_mcmc_ens_prep, then
        after each gp_loglik one gp_mcmc_ens_step (this group's decisions + the next group's
        proposals; gp_mcmc_ens_decide after the last), so 2 + gp_loglik's launches per group
        instead of the ~100 of the tensor-op form (GPUSampler._sweep_torch, which also says what
        a speculative group is)."""
        self._S = self._state_struct()          # kept alive: the library reads it per call
        S, T, C = ctypes.addressof(self._S), ctypes.addressof(self._T), self.C
        stream = kernels._stream(self.dev)
        last = len(self.groups) - 1
        kinds = [ctypes.addressof(k) for k in self._kinds]
        bufs = [self._gbuf[2 ** len(g) - 1] for g in self.groups]

        def outs(b):
            return b["beta"].data_ptr(), b["s"].data_ptr(), b["delta"].data_ptr()

        _capi.call("gp_mcmc_ens_prep", S, T, C, kinds[0], len(self.groups[0]), 1,
                   *outs(bufs[0]), stream)
        for gi, grp in enumerate(self.groups):
            self._loglik(2 ** len(grp) - 1)
            ll = bufs[gi]["ll"].data_ptr()
            if gi == last or not self._merge:
                _capi.call("gp_mcmc_ens_decide", S, T, C, kinds[gi], len(grp), int(gi == last),
                           ll, stream)
                if gi < last:
                    _capi.call("gp_mcmc_ens_prep", S, T, C, kinds[gi + 1],
                               len(self.groups[gi + 1]), 0, *outs(bufs[gi + 1]), stream)
            else:
                _capi.call("gp_mcmc_ens_step", S, T, C, kinds[gi], len(grp), 0, ll, S,
                           kinds[gi + 1], len(self.groups[gi + 1]), 0, *outs(bufs[gi + 1]),
                           stream)

    def _capture(self) -> None:
        """Record one sweep as a graph (capture does not execute it: the chains are untouched)."""
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._sweep()
        self.graph = g

    def sweep(self) -> None:
        if self.use_graph:
            if self.graph is None:
                self._capture()
            self.graph.replay()
        else:
            self._sweep()

    def _capture_block(self, record: bool) -> None:
        """Record ``block`` sweeps as one graph: sweep j reads the (C, nu) uniforms of row j of a
        static block and (``record``) copies the flat states into row j of a static record block.
        One replay per block instead of one per sweep, and one copy per recorded sample instead of
        one uniform upload + five record copies.  Fit: 1.368 ms per sweep at 16 sweeps per replay
        vs 1.373-1.375 at one (the flat one-copy record in both), 1.374-1.383 at 32
        (profiles/r05/r05_block_fit.log): the host keeps the queue full either way."""
        B = self.block
        if not hasattr(self, "_ublk"):
            self._ublk = torch.zeros((B, self.C, self.nu), dtype=F64, device=self.dev)
            self._rblk = torch.zeros((B,) + tuple(self._flat.shape), dtype=F64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        u0 = self.u
        try:
            with torch.cuda.graph(g):
                for j in range(B):
                    self.u = self._ublk[j]
                    self._sweep()
                    if record:
                        self._rblk[j].copy_(self._flat)
        finally:
            self.u = u0
        self._bgraph[record] = g

    # -- chains --------------------------------------------------------------------------
    def _run(self, nsamp: int, rngs: list, record: bool = True, block: int = 64):
        """``nsamp`` sweeps of every chain from the current states (init_state() first if there
        are none); chain c consumes ``rngs[c].random((rows, nu))`` in blocks of ``block`` rows.
        Returns, when ``record``, the samples dict (numpy) with a leading chain axis: betaU
        (C, N, (d+1) P), lamUz, lamWs (C, N, P), lamWOs, logPost (C, N, 1)."""
        if len(rngs) != self.C:
            raise ValueError(f"{len(rngs)} generators for {self.C} chains")
        if self.st is None:
            self.init_state()
        if record:
            rec = torch.empty((nsamp,) + tuple(self._flat.shape), dtype=F64, device=self.dev)
        B = self.block if self.use_graph and self.block > 1 else 0
        for a in range(0, nsamp, block):
            b = min(nsamp, a + block)
            U = self._t(np.stack([r.random((b - a, self.nu)) for r in rngs], axis=1))
            i = a
            while B and b - i >= B:                     # whole graph blocks
                if record not in self._bgraph:
                    self._capture_block(record)
                self._ublk.copy_(U[i - a:i - a + B])
                self._bgraph[record].replay()
                if record:
                    rec[i:i + B].copy_(self._rblk)
                i += B
            for i in range(i, b):                       # the rest one sweep at a time
                self.u.copy_(U[i - a])
                self.sweep()
                if record:
                    rec[i].copy_(self._flat)
        # one host check per run: a factorisation that gave up (info = -1) would otherwise be a
        # silently rejected proposal (ll = NaN); a non-PD proposal (ll = -inf) is a rejection
        for ws in self._ws.values():
            ws.check_status()
        if not record:
            return None
        rec = rec.cpu().numpy().transpose(1, 0, 2)
        return {k: rec[:, :, a:b].copy() for k, (a, b) in self._cols.items()}


class GPUSampler(_ChainSweeps):
    """Component-wise Metropolis over the P PC-GPs of one emulator, all state on the device: the
    one-chain case of _ChainSweeps, plus the tensor-op form of the sweep.

    One sweep is ~11 batched gp_loglik calls plus elementwise proposal / accept work: a few
    hundred small launches.  By default (``use_graph`` None; GPFIT_MCMC_GRAPH=0 opts out) the
    sweep is captured once as a HIP graph (torch.cuda.CUDAGraph) over static buffers -- chain
    state, uniforms, step sizes, counters -- and replayed: at the timing.csv configuration
    (n = 512, P = 8) 3.75 vs 4.04-4.26 ms per sweep eager, the fit 5.0-5.4 vs 5.7-6.3 s
    (profiles/r03/ab_mcmc_graph.log; round 2 measured the opposite while the factorisation
    still allocated its scratch inside every call).  Both paths run the same in-place sweep.

    ``spec`` (default: default_spec(n, P, d + 3); GPFIT_MCMC_SPEC overrides): likelihood-
    changing updates per batched gp_loglik, evaluated speculatively for every outcome of the
    group's earlier updates (see _sweep_torch).  At n = 512 a factorisation is latency-bound (its
    64-column chain), so evaluating 3P problems costs about what P did: spec 2 took a sweep from
    11 gp_loglik calls to 6, 3.79 -> 2.86 ms per sweep (profiles/r03/ab_mcmc_spec.log).  With
    the in-chain likelihood (round 6) 7P = 56 problems cost 0.26 ms per call against 0.21 for
    24, so spec 3 (4 calls) wins at P = 8: 1.278 -> 1.054 ms per sweep, the fit 1.67 -> 1.41-1.44
    s (profiles/r06/r06al_ab_spec.log).

    ``fused`` (default on a HIP device; GPFIT_MCMC_FUSED=0 opts out): the sweep of the kernels in
    csrc/mcmc.hip; otherwise, and on any other device, the tensor-op sweep.
    """

    def __init__(self, X: torch.Tensor, w_hat: torch.Tensor, LamSim: torch.Tensor,
                 params: ModelParams, use_graph: bool | None = None, spec: int | None = None,
                 fused: bool | None = None):
        self.w = w_hat.contiguous()                 # (P, n)
        P, n = self.w.shape
        if spec is None:
            spec = int(os.environ.get("GPFIT_MCMC_SPEC", "0")) or default_spec(n, P,
                                                                               X.shape[1] + 3)
        if spec < 1:
            raise ValueError("spec (updates per speculative group) must be >= 1")
        if fused is None:
            fused = os.environ.get("GPFIT_MCMC_FUSED", "1") == "1"
        fused = fused and X.device.type == "cuda"
        if fused and spec > _capi.MCMC_MAX_GROUP:
            raise ValueError(f"spec > {_capi.MCMC_MAX_GROUP} needs fused=False")
        super().__init__(X, self.w[None], LamSim, [params], use_graph, spec, fused, None)
        self.params = params
        self.lp = self._view("logPost")[0]          # log posterior

    # -- state ---------------------------------------------------------------------------
    def init_state(self) -> ChainState:
        """Chain state from params' current values (its views are made once; later calls copy)."""
        if self.st is None:
            d, P, acc = self.d, self.P, self._acc[0]
            views = [self._view(k)[0].view(shape) for k, shape in
                     (("betaU", (d + 1, P)), ("lamUz", P), ("lamWs", P), ("lamWOs", 1))]
            self.st = ChainState(*views, self._ll[0])
            self.st.acc = {("betaU", k): acc[k] for k in range(d + 1)}
            self.st.acc.update({"lamUz": acc[d + 1], "lamWs": acc[d + 2],
                                "lamWOs": acc[d + 3, :1]})
        super().init_state()
        return self.st

    def counts(self) -> dict:
        return self._counts()[0]

    def log_post(self) -> torch.Tensor:
        pr, st = self.params, self.st
        lp = st.ll.sum()
        lp = lp + log_prior(pr.betaU, st.betaU).sum() + log_prior(pr.lamUz, st.lamUz).sum()
        lp = lp + log_prior(pr.lamWs, st.lamWs).sum() + log_prior(pr.lamWOs, st.lamWOs).sum()
        return lp

    # -- one sweep -----------------------------------------------------------------------
    def _fill(self, buf: dict, slot: int, st: dict) -> None:
        """Model inputs (beta, s, delta) of the P GPs at parameter state ``st`` into rows
        slot P .. (slot + 1) P of a speculative group's batch."""
        sl = slice(slot * self.P, (slot + 1) * self.P)
        buf["beta"][sl].copy_(st["betaU"][1:].transpose(0, 1))
        torch.reciprocal(st["lamUz"], out=buf["s"][sl])
        torch.add(torch.reciprocal(st["lamWs"]), torch.reciprocal(st["lamWOs"] * self.lam[0]),
                  out=buf["delta"][sl])

    @staticmethod
    def _with(st: dict, u, cand) -> dict:
        """Parameter state ``st`` with update ``u``'s element(s) set to ``cand``."""
        name, k = u
        out = dict(st)
        if name == "betaU":
            b = st["betaU"].clone()
            b[k] = cand
            out["betaU"] = b
        else:
            out[name] = cand
        return out

    def _update(self, code: int):
        """(parameter name, betaU row or None) of an update code."""
        d = self.d
        return ("betaU", code) if code <= d else (("lamUz", "lamWs", "lamWOs")[code - d - 1], None)

    def _propose(self, u, take):
        pr, st, P = self.params, self.st, self.P
        name, k = u
        p = getattr(pr, name)
        step = self.steps[name][0]
        if name == "betaU":
            cur, step, m = st.betaU[k], step[k], P
        elif name == "lamWOs":
            cur, step, m = st.lamWOs, step.reshape(1), 1
        else:
            cur, step, m = getattr(st, name), step.reshape(P), P
        up, ua = take(m), take(m)
        cand, ok = propose(p, cur, step, up)
        return cand, ok, log_prior(p, cand) - log_prior(p, cur), ua, cur

    def _accept(self, u, prop, ll_new) -> torch.Tensor:
        """Metropolis decision for update ``u`` given the proposal's per-GP likelihood."""
        st = self.st
        cand, ok, dlp, ua, cur = prop
        name, k = u
        if name == "lamWOs":                 # shared by every GP: accepted on the sum
            acc = ok & (torch.log(ua) < (ll_new - st.ll).sum() + dlp.sum())
        else:
            acc = ok & (torch.log(ua) < ll_new - st.ll + dlp)
        cur.copy_(torch.where(acc, cand, cur))
        st.ll.copy_(torch.where(acc, ll_new, st.ll))
        st.acc[("betaU", k) if name == "betaU" else name].add_(acc.to(F64))
        return acc

    def _sweep(self) -> None:
        if self.fused:
            super()._sweep()
        else:
            self._sweep_torch()

    def _sweep_torch(self) -> None:
        """One component-wise Metropolis sweep on the static buffers (graph-capturable: no
        allocation that outlives it, no host synchronisation, in-place state updates), as
        tensor ops (the host-logic reference of the fused sweep; runs on any device).

        Speculative groups: the updates u_1 .. u_g of a group are proposed together and ONE
        batched gp_loglik evaluates, for every i, u_i's proposal at each of the 2^(i-1)
        accept/reject outcomes of u_1 .. u_i-1 (2^g - 1 parameter states x P GPs); the
        decisions are then taken in order, each reading the likelihood of the outcome that
        actually happened (per GP: the P GPs are independent given lamWOs, whose decision is
        one for all).  Proposals, uniforms and decisions are those of the one-update-at-a-time
        sweep, so the chain is the same Markov chain, draw for draw; what changes is that the
        factorisations, whose latency (a 64-column chain step per tile) bounds a sweep at
        n = 512, are issued g at a time (spec = 1: one call per update)."""
        st, P, u = self.st, self.P, self.u[0]
        o = 0

        def take(k):
            nonlocal o
            r = u[o:o + k]
            o += k
            return r

        # betaU row 0 (the dummy x): the likelihood does not depend on it
        cand, ok, dlp, ua, cur = self._propose(("betaU", 0), take)
        acc = ok & (torch.log(ua) < dlp)
        cur.copy_(torch.where(acc, cand, cur))
        st.acc[("betaU", 0)].add_(acc.to(F64))
        for codes in self.groups:
            grp = [self._update(c) for c in codes]
            props = [self._propose(g, take) for g in grp]
            sets = 2 ** len(grp) - 1
            buf = self._gbuf[sets]
            s0 = {"betaU": st.betaU, "lamUz": st.lamUz, "lamWs": st.lamWs, "lamWOs": st.lamWOs}
            slot, base = 0, []
            for i, g in enumerate(grp):
                base.append(slot)
                for pat in range(2 ** i):         # outcome pattern of the group's earlier updates
                    sx = s0
                    for j in range(i):
                        if (pat >> j) & 1:
                            sx = self._with(sx, grp[j], props[j][0])
                    self._fill(buf, slot, self._with(sx, g, props[i][0]))
                    slot += 1
            self._loglik(sets)
            ll_all = buf["ll"].view(-1, P)
            pat = None
            for i, g in enumerate(grp):
                ll_i = ll_all[base[i]:base[i] + 2 ** i]
                ll_new = ll_i[0] if pat is None else ll_i.gather(0, pat.view(1, P)).view(P)
                acc = self._accept(g, props[i], ll_new).expand(P).long() << i
                pat = acc if pat is None else pat + acc
        self.lp.copy_(self.log_post().reshape(1))

    # -- chains --------------------------------------------------------------------------
    def run(self, nsamp: int, rng: np.random.Generator, record: bool = True, block: int = 64):
        """``nsamp`` sweeps from the current state (init_state() first if there is none);
        returns the samples dict (numpy), betaU (N, (d+1) P) ... logPost (N, 1), when
        ``record``."""
        rec = self._run(nsamp, [rng], record, block)
        return {k: v[0] for k, v in rec.items()} if record else None


# --------------------------------------------------------------------------- step tuning
def logistic_step(log_steps: np.ndarray, accepts: np.ndarray, trials: int,
                  target_logit: float = TARGET_LOGIT, pseudo: float = 0.5,
                  anchor: float = math.log(100.0)) -> float:
    """Step whose fitted acceptance probability hits the target: binomial logit regression of
    acceptance on log step (IRLS).  ``pseudo`` successes/failures per level keep the fit
    finite when a level accepts everything or nothing, and two anchor observations (one
    acceptance at ``anchor`` below the smallest step, one rejection ``anchor`` above the
    largest) give the fit a slope when every level accepts (or rejects) almost always, so it
    extrapolates instead of stalling at the ladder's end.  Returns exp(log step*)."""
    xl = np.asarray(log_steps, dtype=np.float64)
    x = np.concatenate([xl, [xl.min() - anchor, xl.max() + anchor]])
    yk = np.concatenate([np.asarray(accepts, dtype=np.float64) + pseudo, [1.0, 0.0]])
    nk = np.concatenate([np.full(len(xl), float(trials) + 2.0 * pseudo), [1.0, 1.0]])
    A = np.stack([np.ones_like(x), x], axis=1)
    bvec = np.zeros(2)
    for _ in range(100):
        eta = A @ bvec
        p = 1.0 / (1.0 + np.exp(-eta))
        wgt = nk * p * (1.0 - p)
        grad = A.T @ (yk - nk * p)
        H = A.T @ (A * wgt[:, None])
        try:
            dlt = np.linalg.solve(H, grad)
        except np.linalg.LinAlgError:
            break
        bvec = bvec + dlt
        if np.max(np.abs(dlt)) < 1e-10:
            break
    b0, b1 = bvec
    if not np.all(np.isfinite(bvec)) or b1 >= -1e-12:
        rate = (yk / nk)[: len(xl)]
        return float(np.exp(xl[int(np.argmin(np.abs(rate - 1.0 / math.e)))]))
    return float(np.exp((target_logit - b0) / b1))


def _ladder(n_levels: int) -> np.ndarray:
    """Step-scale exponents of the tuning ladder: n_levels evenly spaced around 0."""
    return np.linspace(-(n_levels - 1) / 2.0, (n_levels - 1) / 2.0, n_levels)


def _fit_chain_steps(pr: ModelParams, base: dict, ex: np.ndarray, counts: list, n_burn: int):
    """The per-element logistic fits of one chain (_tune): ``counts`` holds the chain's counts
    dict (GPUSampler.counts()) per ladder level,
    ``base`` the steps the ladder scaled.  Returns (new steps per parameter, the tune record)."""
    logs = {k: np.log(base[k][None] * (2.0 ** ex).reshape((-1,) + (1,) * base[k].ndim))
            for k in base}
    d, P = pr.betaU.val_shape[0] - 1, pr.betaU.val_shape[1]
    new = {k: base[k].copy() for k in base}

    def fit(name, x, acc):
        # clamp: the anchors' span, rho's range for BetaRho moves, the bound width
        p = getattr(pr, name)
        st_ = logistic_step(x, acc, n_burn)
        lo_c, hi_c = math.exp(x.min() - math.log(100.0)), math.exp(x.max() + math.log(100.0))
        if p.mcmcStepType == "BetaRho":
            hi_c = min(hi_c, 1.0)
        elif np.isfinite(p.bounds[0]) and np.isfinite(p.bounds[1]):
            hi_c = min(hi_c, p.bounds[1] - p.bounds[0])
        return float(np.clip(st_, lo_c, max(hi_c, lo_c)))

    for k in range(d + 1):
        for j in range(P):
            acc = np.array([c[("betaU", k)][j] for c in counts])
            new["betaU"][k, j] = fit("betaU", logs["betaU"][:, k, j], acc)
    for name in ("lamUz", "lamWs"):
        for j in range(P):
            acc = np.array([c[name][j] for c in counts])
            new[name][0, j] = fit(name, logs[name][:, 0, j], acc)
    acc = np.array([c["lamWOs"][0] for c in counts])
    new["lamWOs"][0, 0] = fit("lamWOs", logs["lamWOs"][:, 0, 0], acc)
    info = {"scales": 2.0 ** ex, "trials": n_burn, "base": base, "new": new,
            "accepts": {
                "betaU": np.array([[c[("betaU", k)] for k in range(d + 1)] for c in counts]),
                "lamUz": np.array([c["lamUz"] for c in counts]),
                "lamWs": np.array([c["lamWs"] for c in counts]),
                "lamWOs": np.array([c["lamWOs"] for c in counts])}}
    return new, info


def _tune(sampler: _ChainSweeps, n_burn: int, n_levels: int, rngs: list) -> list:
    """GPMSA-style step-size tuning (see module doc) of every chain of ``sampler``, stepped
    together: updates each chain's params' mcmcStepParam in place, leaves the chains at the
    states reached and returns the per-chain tune records."""
    if sampler.st is None:
        sampler.init_state()
    ex = _ladder(n_levels)
    bases = [{k: getattr(pr, k).mcmcStepParam.copy() for k in ModelParams.names}
             for pr in sampler._params]
    # burn-in at the default steps first: acceptance counted while the chain is still
    # travelling from the start values would make the smallest-step level look worst
    sampler.set_steps(1.0)
    sampler._run(n_burn, rngs, record=False)
    counts = []
    for e in ex:
        sampler.set_steps(2.0 ** e)
        sampler.reset_counts()
        sampler._run(n_burn, rngs, record=False)
        counts.append(sampler._counts())
    infos = []
    for c, pr in enumerate(sampler._params):
        new, info = _fit_chain_steps(pr, bases[c], ex, [lev[c] for lev in counts], n_burn)
        for k in new:
            getattr(pr, k).mcmcStepParam = new[k]
        infos.append(info)
    sampler.set_steps(1.0)
    sampler.reset_counts()
    return infos


def tune_step_sizes(sampler: GPUSampler, n_burn: int, n_levels: int,
                    rng: np.random.Generator) -> None:
    """Tune the lone sampler's steps (_tune); ``sampler.last_tune`` is the tune record."""
    sampler.last_tune = _tune(sampler, n_burn, n_levels, [rng])[0]


# ------------------------------------------------------------------------ ensemble sampler
_SHARED_FIELDS = ("val_shape", "dist", "params", "bounds", "mcmcStepType")


def check_shared_priors(params: list) -> None:
    """Raise ValueError naming the first field in which a ModelParams of the list differs from
    the first one: an ensemble shares d and P (val_shape), the prior families and parameters,
    the bounds and the step types; values and step sizes are per chain."""
    for c, pr in enumerate(params[1:], start=1):
        for nm in ModelParams.names:
            for f in _SHARED_FIELDS:
                a, b = getattr(getattr(params[0], nm), f), getattr(getattr(pr, nm), f)
                if (a if isinstance(a, str) else tuple(a)) != (b if isinstance(b, str)
                                                               else tuple(b)):
                    raise ValueError(f"ensemble: model {c} differs from model 0 in {nm}.{f} "
                                     f"({b!r} != {a!r})")


def loglik_max_batch(n: int, dev: torch.device) -> int | None:
    """Largest gp_loglik batch at order n that the persistent factorisation takes on the current
    stream of ``dev`` (gp_pp_plan_stream: GP_PP_PLAN_ELIGIBLE), or None when n itself is beyond
    its range (every batch then takes the blocked path, so there is nothing to stay within).  A
    larger batch silently takes the blocked sweep + L^-1 path: much slower, and equal to the
    in-chain path only to 1e-11."""
    out = (ctypes.c_longlong * len(_capi.PP_PLAN))()
    stream = kernels._stream(dev)

    def plan(batch):
        rc = _capi.lib().gp_pp_plan_stream(n, batch, 0, -1, out, stream)
        if rc:
            raise _capi.GPFitError("gp_pp_plan_stream", rc)
        return dict(zip(_capi.PP_PLAN, out))

    first = plan(1)
    if not first["eligible"]:
        return None
    # the chains hold one workgroup per problem and need as many workers again
    best = max(1, int(first["resident"]) // 2)
    while best > 1 and not plan(best)["eligible"]:
        best -= 1
    return best


class EnsembleSampler(_ChainSweeps):
    """C chains stepped together: one gp_mcmc_ens_* launch of C workgroups around each batched
    gp_loglik of all chains' state sets, instead of C GPUSamplers one after another.

    The chains share X (n, d), P, the prior families / parameters / bounds and the step types;
    each has its own PC weights ``w_hat[c]`` (P, n), ``LamSim[c]`` (P,), state, step sizes,
    counters and uniforms (``params[c]``: a ModelParams holding chain c's values and steps).  C
    repeat chains of one model and C scalar models on one design are the same thing with equal
    or different ``w_hat``.  Chain c is the Markov chain a lone GPUSampler produces from the same
    generator: both run _ChainSweeps' sweep, and a chain does not depend on the others.

    Fused sweep only, on a HIP device.  ``max_batch`` is by default the largest batch the
    persistent factorisation takes (loglik_max_batch; beyond it gp_loglik falls back to a much
    slower path).  The default group size starts from default_spec(n, C P, d + 3) and is lowered
    while one chain's (2^spec - 1) P problems exceed ``max_batch``.
    """

    def __init__(self, X: torch.Tensor, w_hat: torch.Tensor, LamSim: torch.Tensor, params: list,
                 use_graph: bool | None = None, spec: int | None = None,
                 max_batch: int | None = None):
        if X.device.type != "cuda":
            raise ValueError("EnsembleSampler runs the fused sweep: it needs a HIP device")
        self.w = w_hat.to(X.device, F64).contiguous()                   # (C, P, n)
        if self.w.dim() != 3:
            raise ValueError("w_hat must be (C, P, n)")
        C, P, n = self.w.shape
        d = X.shape[1]
        self.params = params = list(params)
        if len(params) != C:
            raise ValueError(f"{len(params)} ModelParams for {C} chains")
        if not 1 <= C <= _capi.MCMC_MAX_CHAINS:
            raise ValueError(f"1 .. {_capi.MCMC_MAX_CHAINS} chains (GPFIT_MCMC_MAX_CHAINS)")
        check_shared_priors(params)
        if params[0].betaU.val_shape != (d + 1, P):
            raise ValueError(f"params are for (d, P) = ({params[0].betaU.val_shape[0] - 1}, "
                             f"{params[0].betaU.val_shape[1]}), the data for ({d}, {P})")
        if X.shape[0] != n:
            raise ValueError("X and w_hat disagree on n")
        # slices of whole chains within the persistent factorisation's range
        limit = loglik_max_batch(n, X.device) if max_batch is None else int(max_batch)
        max_batch = C * (2 ** _capi.MCMC_MAX_GROUP - 1) * P if limit is None else limit
        if P > max_batch:
            raise ValueError(f"one chain's {P} GPs do not fit a gp_loglik batch of at most "
                             f"{max_batch} problems (max_batch; by default the persistent "
                             "factorisation's range on this stream)")
        given = spec if spec is not None else int(os.environ.get("GPFIT_MCMC_SPEC", "0"))
        if given:
            if not 1 <= given <= _capi.MCMC_MAX_GROUP:
                raise ValueError(f"spec must be 1 .. {_capi.MCMC_MAX_GROUP}")
            if (2 ** given - 1) * P > max_batch:
                raise ValueError(f"spec {given}: one chain's {(2 ** given - 1) * P} problems "
                                 f"exceed the gp_loglik batch limit {max_batch}")
            spec = given
        else:
            spec = default_spec(n, C * P, d + 3)
            while (2 ** spec - 1) * P > max_batch:
                spec -= 1
        super().__init__(X, self.w, LamSim, params, use_graph, spec, True, max_batch)

    def counts(self) -> list:
        """Per chain, GPUSampler.counts()'s dict."""
        return self._counts()

    def run(self, nsamp: int, rngs: list, record: bool = True, block: int = 64):
        """``nsamp`` sweeps of every chain from the current states; chain c consumes
        ``rngs[c].random((rows, nu))`` block by block exactly as GPUSampler.run consumes its one
        generator.  Returns, when ``record``, the samples dict with a leading chain axis: betaU
        (C, N, (d+1) P), lamUz, lamWs (C, N, P), lamWOs, logPost (C, N, 1)."""
        return self._run(nsamp, rngs, record, block)


def tune_step_sizes_ensemble(sampler: EnsembleSampler, n_burn: int, n_levels: int,
                             rngs: list) -> None:
    """tune_step_sizes over a whole ensemble (_tune); ``sampler.last_tune`` is the list of
    per-chain tune records."""
    sampler.last_tune = _tune(sampler, n_burn, n_levels, rngs)


# ------------------------------------------------------------------ convergence diagnostics
def _draws(chains, nburn: int) -> np.ndarray:
    x = np.asarray(chains, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("chains must be (C, N) or (C, N, K)")
    return x[:, int(nburn):]


def rhat(chains, nburn: int = 0) -> np.ndarray:
    """Split-R-hat per parameter element (Gelman et al. 2013, Bayesian Data Analysis 3rd ed.,
    section 11.4).  ``chains`` is (C, N, K) (or (C, N)); the first ``nburn`` draws are dropped,
    leaving N' per chain.  With h = N' // 2 each chain gives two sequences, its first h and its
    last h draws (the middle draw of an odd N' is unused): m = 2 C sequences x_j of length h, with
    means xbar_j, grand mean xbar and variances s_j^2 (divisor h - 1).  Then::

        B = h / (m - 1) sum_j (xbar_j - xbar)^2        W = 1/m sum_j s_j^2
        var+ = (h - 1) / h W + B / h                   R-hat = sqrt(var+ / W)

    Returns (K,) (a scalar array for (C, N)); NaN where W = 0 (a constant chain) or h < 2."""
    x = _draws(chains, nburn)
    C, N, K = x.shape
    h = N // 2
    if h < 2:
        return np.full(np.shape(chains)[2:], np.nan)
    seq = np.concatenate([x[:, :h], x[:, N - h:]], axis=0)              # (2 C, h, K)
    m = seq.shape[0]
    means = seq.mean(axis=1)
    B = h / (m - 1.0) * ((means - means.mean(axis=0)) ** 2).sum(axis=0)
    W = seq.var(axis=1, ddof=1).mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.sqrt(((h - 1.0) / h * W + B / h) / W)
    return out.reshape(np.shape(chains)[2:])


def _autocov_fft(x: np.ndarray) -> np.ndarray:
    """Biased autocovariance along axis 1 of (C, N, K): a[c, t] = 1/N sum_{i < N - t}
    (x[c, i] - xbar_c)(x[c, i + t] - xbar_c), by FFT of the zero-padded centred series."""
    N = x.shape[1]
    z = x - x.mean(axis=1, keepdims=True)
    f = np.fft.rfft(z, n=2 * N, axis=1)
    return np.fft.irfft(f * np.conj(f), n=2 * N, axis=1)[:, :N] / N


def ess(chains, nburn: int = 0) -> np.ndarray:
    """Effective sample size per parameter element.  ``chains`` is (C, N, K) (or (C, N)); after
    dropping ``nburn`` draws, per chain c: mean xbar_c and the biased autocovariance
    a_c(t) = 1/N sum_{i=1}^{N-t} (x_{c,i} - xbar_c)(x_{c,i+t} - xbar_c) (computed by FFT).  With::

        W = N / (N - 1) mean_c a_c(0)
        var+ = (N - 1) / N W + var_c(xbar_c)           (divisor C - 1; 0 for C = 1)
        rho_0 = 1,   rho_t = 1 - (W - mean_c a_c(t)) / var+      (t = 1 .. N - 1)

    (the chain-averaged autocorrelations of Gelman et al. 2013, eq. 11.7, in autocovariance
    form), the sum is cut by Geyer's (1992) initial positive sequence: P_k = rho_2k + rho_2k+1,
    k = 0 .. (N // 2) - 1; K = the first k >= 1 with P_k <= 0 (all pairs if none is)::

        tau = -1 + 2 sum_{k < K} P_k                   ESS = C N / tau

    Returns (K,) (a scalar array for (C, N)); NaN where var+ = 0 (a constant chain) or N < 4."""
    x = _draws(chains, nburn)
    C, N, K = x.shape
    shape = np.shape(chains)[2:]
    if N < 4:
        return np.full(shape, np.nan)
    acov = _autocov_fft(x)                                              # (C, N, K)
    W = N / (N - 1.0) * acov[:, 0].mean(axis=0)
    between = x.mean(axis=1).var(axis=0, ddof=1) if C > 1 else np.zeros(K)
    varp = (N - 1.0) / N * W + between
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = 1.0 - (W[None] - acov.mean(axis=0)) / varp[None]          # (N, K)
    rho[0] = 1.0
    npair = N // 2
    pairs = rho[0:2 * npair:2] + rho[1:2 * npair:2]                     # (npair, K)
    out = np.full(K, np.nan)
    for e in range(K):
        if not varp[e] > 0:
            continue
        stop = np.flatnonzero(pairs[1:, e] <= 0)
        kk = stop[0] + 1 if stop.size else npair
        out[e] = C * N / (-1.0 + 2.0 * pairs[:kk, e].sum())
    return out.reshape(shape)
