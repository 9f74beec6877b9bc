"""Maximum-likelihood GP — drop-in for the GPmodule surface of BASELINE config 1.

Reference usage (``examples/02_univariate_GP_regression.ipynb`` cell 5, raw :80-85; GPmodule is
un-vendored, ``requirements-cc.txt:20``)::

    GPmodel = GPmodule.GP(covariance=GPmodule.squared_exponential, cov_para={'nugget': 1e-3})
    fit_maxl = GPmodel.fit(x, y, x0)        # x0 = [variance, length scale] start
    print(GPmodel.minimize_res)             # scipy OptimizeResult: fun -3.989954265337257
    ypred = GPmodel.predictor(xpred)
    epred = GPmodel.error(xpred)

and cell 9 uses ``GPmodel.covariance(x1, x2, theta)``, ``GPmodel.theta``, ``GPmodel.K`` and
``GPmodel.K_inv``.

Model (restated; pinned by the notebook's printed optimum, ``tests/golden/nb02_known_answer``):
``K(theta) = theta0^2 exp(-|dx|^2 / (2 theta1^2)) + nugget^2 I`` and the objective
``NLL(theta) = 1/2 y^T K^-1 y + 1/2 log|K|`` (no 2 pi term), minimised by BFGS from ``x0``.
Every objective evaluation runs on the GPU: Gram (gp_gram_ardse) -> Cholesky + L^-1
(gp_potrf_inv) -> quadratic form + logdet (gp_nll); scipy drives the optimisation on the host
(the reference does the same with numpy).  ``predictor`` / ``error`` are gp_predict's posterior
mean and sqrt(marginal variance) at the fitted theta (cell 9's formulas, diagonal only; the
prior variance at a prediction point is theta0^2 — whether GPmodule adds the nugget there is not
recorded anywhere in the reference: parity for ``error`` is unpinned at the 1e-6 level).

Beyond the reference: ``fit(..., jac=True)`` gives scipy the analytic gradient (gp_nll_grad, one
factorisation per value-and-gradient evaluation) instead of letting it difference the objective,
and ``GP(..., ard=True)`` fits one length scale per input column, theta = [theta0, l_1 .. l_d].
"""
from __future__ import annotations

import numpy as np
import scipy.optimize as sopt
import torch

from . import kernels

F64 = torch.float64


def _theta_to_kernel(theta, nugget):
    """(s, beta, delta) of the unified ARD-SE form for GPmodule's squared exponential."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    return theta[0] ** 2, 1.0 / (2.0 * theta[1] ** 2), nugget ** 2


def _kernel_params(theta, nugget, d, ard=False):
    """(s, beta (d,), delta): one length scale for every column, or with ``ard`` theta =
    [theta0, l_1 .. l_d] and beta_k = 1 / (2 l_k^2)."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if not ard:
        s, beta, delta = _theta_to_kernel(theta, nugget)
        return s, np.full(d, beta), delta
    if theta.size != d + 1:
        raise ValueError(f"theta: ard=True takes [theta0, l_1 .. l_{d}], got {theta.size} values")
    return theta[0] ** 2, 1.0 / (2.0 * theta[1:] ** 2), nugget ** 2


def squared_exponential(x1, x2, theta, nugget: float = 0.0, device=None):
    """theta0^2 exp(-|x1_i - x2_j|^2 / (2 theta1^2)) (+ nugget^2 on the diagonal when x1 is x2)
    as a numpy (n1, n2) matrix, built by the gp_cross_ardse kernel.  A theta of more than two
    values is [theta0, l_1 .. l_d], one length scale per column (GP(ard=True))."""
    dev = _device(device)
    a = np.asarray(x1, dtype=np.float64)
    b = np.asarray(x2, dtype=np.float64)
    a = a.reshape(a.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    d = a.shape[1]
    s, beta, delta = _kernel_params(theta, nugget, d, np.size(theta) > 2)
    Kt = kernels.cross(torch.as_tensor(b, device=dev), torch.as_tensor(a, device=dev),
                       torch.as_tensor(beta, device=dev).reshape(1, d), s)   # (1, n1, n2)
    K = Kt[0].cpu().numpy()
    if x1 is x2 and delta:
        K[np.diag_indices_from(K)] += delta
    return K


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("gladsgp_amd.gpmodule runs on a HIP device (libgpfit); none found")
    return torch.device("cuda", torch.cuda.current_device())


class GP:
    """GPmodule.GP mirror (fit by maximum likelihood, predict at new points)."""

    def __init__(self, covariance=squared_exponential, cov_para=None, device=None,
                 ard: bool = False):
        if covariance is not squared_exponential:
            raise NotImplementedError("only the squared-exponential covariance is on the GPU path")
        self.covariance_fn = covariance
        self.cov_para = dict(cov_para or {})
        self.nugget = float(self.cov_para.get("nugget", 0.0))
        self.device = _device(device)
        self.ard = bool(ard)        # theta = [theta0, l_1 .. l_d], one length scale per column
        self.theta = None
        self.minimize_res = None
        self.nfev_gpu = 0

    # ------------------------------------------------------------------------------ kernels
    def covariance(self, x1, x2, theta):
        return squared_exponential(x1, x2, theta, self.nugget if x1 is x2 else 0.0,
                                   self.device)

    def _params(self, theta):
        """(s, beta as a (1, d) device tensor, delta) at theta."""
        d = self._X.shape[1]
        s, beta, delta = _kernel_params(theta, self.nugget, d, self.ard)
        return s, torch.as_tensor(beta, device=self.device).reshape(1, d), delta

    def _factor(self, theta):
        s, beta, delta = self._params(theta)
        G = kernels.gram(self._X, beta, s, delta)
        return kernels.cholesky_inverse(G), s, beta

    def negloglik(self, theta) -> float:
        """1/2 y^T K^-1 y + 1/2 log|K| at theta (inf where K is not positive definite)."""
        ch, _, _ = self._factor(theta)
        v = kernels.nll(ch, self._y)
        self.nfev_gpu += 1
        if int(ch.info[0]) != 0:
            return np.inf
        return float(v[0])

    def negloglik_grad(self, theta):
        """(f, g): the objective of :meth:`negloglik` and its gradient in theta, from one
        factorisation (kernels.nll_value_grad: the analytic gradient in s, delta, beta on the
        GPU) and the chain rule through s = theta0^2 and beta_k = 1 / (2 l_k^2):
        g_0 = 2 theta0 dNLL/ds, g_1 = -theta1^-3 sum_k dNLL/dbeta_k (``ard``: g_{1+k} =
        -l_k^-3 dNLL/dbeta_k).  (inf, zeros) where K is not positive definite."""
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        s, beta, delta = self._params(theta)
        one = lambda v: torch.full((1,), float(v), dtype=F64, device=self.device)  # noqa: E731
        val, grad, info = kernels.nll_value_grad(self._X, beta, one(s), one(delta), self._y)
        self.nfev_gpu += 1
        out = torch.cat([val, grad[0], info.to(F64)]).cpu().numpy()    # the one host sync
        if out[-1] != 0:
            return np.inf, np.zeros(theta.size)
        gb = out[3:-1]
        gl = -gb / theta[1:] ** 3 if self.ard else np.array([-np.sum(gb) / theta[1] ** 3])
        return float(out[0]), np.concatenate([[2.0 * theta[0] * out[1]], gl])

    # ---------------------------------------------------------------------------- surface
    def set_data(self, x, y):
        """The training data :meth:`negloglik` and :meth:`negloglik_grad` evaluate on
        (:meth:`fit` sets it itself)."""
        x = np.asarray(x, dtype=np.float64)
        self._x = x.reshape(x.shape[0], -1)
        self._X = torch.as_tensor(self._x, device=self.device).contiguous()
        self._y_np = np.asarray(y, dtype=np.float64).reshape(-1)
        self._y = torch.as_tensor(self._y_np, device=self.device).reshape(1, -1)

    def fit(self, x, y, x0, method: str = "BFGS", jac: bool = False, **minimize_kw):
        """Maximum-likelihood theta from start x0 (scipy BFGS over the GPU objective).
        Returns the fitted theta; the scipy result is ``self.minimize_res``.  ``jac=True`` hands
        scipy :meth:`negloglik_grad` (value and analytic gradient per evaluation) instead of
        letting it difference the bare objective."""
        self.set_data(x, y)
        if jac:
            res = sopt.minimize(self.negloglik_grad, np.asarray(x0, dtype=np.float64),
                                method=method, jac=True, **minimize_kw)
        else:
            res = sopt.minimize(self.negloglik, np.asarray(x0, dtype=np.float64), method=method,
                                **minimize_kw)
        self.minimize_res = res
        self.theta = np.asarray(res.x, dtype=np.float64)
        ch, s, beta = self._factor(self.theta)
        ch.check()
        self._chol, self._s, self._beta = ch, s, beta
        return self.theta

    @property
    def K(self) -> np.ndarray:
        """Training covariance at the fitted theta, nugget^2 on the diagonal (numpy)."""
        return self.covariance(self._x, self._x, self.theta)

    @property
    def K_inv(self) -> np.ndarray:
        """K^-1 = L^-T L^-1 from the GPU factorisation (numpy; small-n diagnostics)."""
        Li = self._chol.Linv[0].cpu().numpy()
        return Li.T @ Li

    def _predict(self, xpred):
        xp = np.asarray(xpred, dtype=np.float64)
        xp = xp.reshape(xp.shape[0], -1)
        mean, var = kernels.predict(self._chol, self._X,
                                    torch.as_tensor(xp, device=self.device), self._beta,
                                    self._s, self._s, self._y)
        return mean[0].cpu().numpy(), var[0].cpu().numpy()

    def sobol_indices(self, lo=None, hi=None):
        """(first_order (d,), total_index (d,)): the Sobol' indices of the posterior mean at the
        fitted theta under inputs uniform on the box ``[lo, hi]`` (default the unit cube), in
        closed form (gp_sobol_exact, one unit): no design and no sampling error."""
        from .sensitivity import indices_from_moments
        d = self._X.shape[1]
        one = lambda v: torch.full((1,), float(v), dtype=F64, device=self.device)  # noqa: E731
        box = lambda v: None if v is None else torch.as_tensor(                    # noqa: E731
            np.broadcast_to(np.asarray(v, dtype=np.float64), (d,)).copy(), device=self.device)
        if (lo is None) != (hi is None):
            lo, hi = (0.0 if lo is None else lo), (1.0 if hi is None else hi)
        E, Q = kernels.sobol_exact(self._X, kernels.alpha(self._chol, self._y), self._beta,
                                   one(self._s), lo=box(lo), hi=box(hi))
        _, _, first, total = indices_from_moments(E.reshape(1, 1), Q)
        return first[0].cpu().numpy(), total[0].cpu().numpy()

    def predictor(self, xpred) -> np.ndarray:
        """Posterior mean K(xpred, x) K^-1 y at the fitted theta, shape (m,)."""
        return self._predict(xpred)[0]

    def error(self, xpred) -> np.ndarray:
        """Posterior standard error sqrt(diag(K(xp, xp) - K(xp, x) K^-1 K(x, xp))), shape (m,)."""
        return np.sqrt(np.maximum(self._predict(xpred)[1], 0.0))
