"""Tensor-level entry points over libgpfit (device memory and streams from PyTorch-ROCm).

PyTorch is plumbing here: it owns the device buffers and the current HIP stream; every
arithmetic step runs in the HIP kernels behind :mod:`gladsgp_amd._capi`.

Layout convention: libgpfit is column-major (LAPACK).  A column-major n x n matrix M is held in
a torch tensor ``buf`` of shape (batch, n_cols, ld) with ``buf[b, j, i] = M[i, j]``; the
logical matrix is ``buf.transpose(-1, -2)``.  Symmetric matrices (the Gram) look the same
either way.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _capi

F64 = torch.float64


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a HIP device tensor (got {t.device}); "
                         "libgpfit has no CPU path")


def _as_f64(x, device, name) -> torch.Tensor:
    t = torch.as_tensor(x, dtype=F64, device=device)
    _check_device(t, name)
    return t.contiguous()


def _per_batch(x, batch: int, device, name) -> torch.Tensor:
    t = _as_f64(x, device, name).reshape(-1)
    if t.numel() == 1 and batch > 1:
        t = t.expand(batch).contiguous()
    if t.numel() != batch:
        raise ValueError(f"{name}: expected {batch} values, got {t.numel()}")
    return t


def _beta(beta, batch: int, d: int, device) -> torch.Tensor:
    t = _as_f64(beta, device, "beta")
    if t.dim() == 1:
        t = t.reshape(1, -1)
    if t.shape[0] == 1 and batch > 1:
        t = t.expand(batch, t.shape[1]).contiguous()
    if tuple(t.shape) != (batch, d):
        raise ValueError(f"beta: expected shape ({batch}, {d}), got {tuple(t.shape)}")
    return t


def padded_n(n: int) -> int:
    return _capi.lib().gp_padded_n(int(n))


def gram(X: torch.Tensor, beta, s, delta, batch: int | None = None) -> torch.Tensor:
    """G[b] = s[b] exp(-sum_k beta[b,k] (x_i - x_j)_k^2) + delta[b] I   -> (batch, n, n)."""
    X = _as_f64(X, None if not torch.is_tensor(X) else X.device, "X")
    n, d = X.shape
    bt = torch.as_tensor(beta)
    batch = batch or (bt.shape[0] if bt.dim() == 2 else 1)
    dev = X.device
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    d_t = _per_batch(delta, batch, dev, "delta")
    G = torch.empty((batch, n, n), dtype=F64, device=dev)
    _capi.call("gp_gram_ardse", X.data_ptr(), n, d, d, beta_t.data_ptr(), d, s_t.data_ptr(),
               d_t.data_ptr(), G.data_ptr(), n, n * n, batch, _stream(dev))
    return G


def cross(X: torch.Tensor, Xs: torch.Tensor, beta, s, batch: int | None = None) -> torch.Tensor:
    """K*^T[b] (n x m) held column-major: returns tensor (batch, m, n), [b, j, i] = K*[j, i]."""
    X = _as_f64(X, X.device, "X")
    Xs = _as_f64(Xs, X.device, "Xs")
    n, d = X.shape
    m = Xs.shape[0]
    bt = torch.as_tensor(beta)
    batch = batch or (bt.shape[0] if bt.dim() == 2 else 1)
    beta_t = _beta(beta, batch, d, X.device)
    s_t = _per_batch(s, batch, X.device, "s")
    Kt = torch.empty((batch, m, n), dtype=F64, device=X.device)
    _capi.call("gp_cross_ardse", X.data_ptr(), n, d, Xs.data_ptr(), m, d, d, beta_t.data_ptr(),
               d, s_t.data_ptr(), Kt.data_ptr(), n, m * n, batch, _stream(X.device))
    return Kt


@dataclass
class Cholesky:
    """Result of :func:`cholesky_inverse` (buffers are column-major, see module doc)."""

    n: int
    a_buf: torch.Tensor      # (batch, n, n): lower triangle holds L (col-major)
    linv_buf: torch.Tensor   # (batch, npad, npad): L^-1 (col-major, zero-padded)
    info: torch.Tensor       # (batch,) int32, LAPACK potrf info
    logdet: torch.Tensor     # (batch,) float64, log|A|

    @property
    def L(self) -> torch.Tensor:
        return torch.tril(self.a_buf.transpose(-1, -2))

    @property
    def Linv(self) -> torch.Tensor:
        return self.linv_buf.transpose(-1, -2)[:, : self.n, : self.n]

    def check(self) -> None:
        check_info(self.info)


class FactorizationInternalError(RuntimeError):
    """info = -1: the persistent factorisation gave up on a bounded wait (an internal error of
    the library, never a property of the matrix)."""


def check_info(info: torch.Tensor) -> None:
    """Raise for any problem whose factorisation did not succeed: info = -1 is an internal
    error (:class:`FactorizationInternalError`), info = j > 0 the LAPACK non-positive-definite
    pivot (ValueError).  Synchronises with the device."""
    vals = info.cpu()
    bad = torch.nonzero(vals).flatten().tolist()
    if not bad:
        return
    internal = [b for b in bad if int(vals[b]) < 0]
    if internal:
        raise FactorizationInternalError(
            f"internal factorisation error (info = -1: a bounded wait of the persistent kernel "
            f"gave up) for problems {internal}; results are invalid")
    raise ValueError(f"matrix not positive definite (info={vals[bad].tolist()} for "
                     f"problems {bad})")


class Workspace:
    """Reusable device scratch (grown on demand, never shrunk; 256-B aligned torch storage)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        return self.buf


_SCRATCH = {}


def _scratch(name: str, device, nbytes: int) -> torch.Tensor:
    """The per-device scratch of the entry point family ``name``, reused across calls on the
    current stream."""
    return _SCRATCH.setdefault((name, str(device)), Workspace()).get(nbytes, device)


def cholesky_inverse(G: torch.Tensor, overwrite: bool = True,
                     workspace: Workspace | None = None) -> Cholesky:
    """Blocked MFMA Cholesky A = L L^T with L^-1, logdet and LAPACK info per problem
    (gp_potrf_inv_ws: the factorisation's scratch comes from ``workspace``, by default a
    per-device one reused across calls on the current stream)."""
    _check_device(G, "G")
    if G.dtype != F64:
        raise TypeError("G must be float64")
    if G.dim() == 2:
        G = G.unsqueeze(0)
    batch, n, n2 = G.shape
    if n != n2:
        raise ValueError("G must be square")
    A = G if (overwrite and G.is_contiguous()) else G.contiguous().clone()
    npad = padded_n(n)
    Linv = torch.empty((batch, npad, npad), dtype=F64, device=G.device)
    info = torch.empty(batch, dtype=torch.int32, device=G.device)
    logdet = torch.empty(batch, dtype=F64, device=G.device)
    nbytes = int(_capi.lib().gp_potrf_inv_ws_bytes(n, batch))
    ws = (workspace.get(nbytes, G.device) if workspace is not None
          else _scratch("potrf", G.device, nbytes))
    _capi.call("gp_potrf_inv_ws", A.data_ptr(), n, n, n * n, Linv.data_ptr(), npad, npad * npad,
               batch, info.data_ptr(), logdet.data_ptr(), ws.data_ptr(), ws.numel(),
               _stream(G.device))
    return Cholesky(n, A, Linv, info, logdet)


PredictWorkspace = Workspace   # scratch of predict / fit_predict / predict_prepare


_DEFAULT_WS = PredictWorkspace()


@dataclass
class PackedLinv:
    """L^-1 in the tile-packed layout (gp_pack_linv: column c of the padded buffer from row
    16 floor(c/16) on, about half the padded square) -- the single-GP broadcast's payload, which
    :func:`predict` reads in place -- with, optionally, z = L^-1 w (gp_predict_z)."""

    n: int
    buf: torch.Tensor                 # (batch, gp_linv_packed_elems(n)) float64
    info: torch.Tensor                # (batch,) int32
    z: torch.Tensor | None = None     # (batch, padded_n(n)) float64

    def check(self) -> None:
        check_info(self.info)


def linv_packed_elems(n: int) -> int:
    return int(_capi.lib().gp_linv_packed_elems(int(n)))


def pack_linv(chol: Cholesky, out: torch.Tensor | None = None) -> torch.Tensor:
    """The tile-packed L^-1 of every problem: (batch, gp_linv_packed_elems(n)) (gp_pack_linv)."""
    batch, npad = chol.linv_buf.shape[0], chol.linv_buf.shape[1]
    E = linv_packed_elems(chol.n)
    if out is None:
        out = torch.empty((batch, E), dtype=F64, device=chol.linv_buf.device)
    for b in range(batch):
        _capi.call("gp_pack_linv", chol.linv_buf[b].data_ptr(), chol.n, npad,
                   out[b].data_ptr(), _stream(out.device))
    return out


def predict_z(chol, w, out: torch.Tensor | None = None) -> torch.Tensor:
    """z = L^-1 w per problem, (batch, padded_n(n)), zero past n, with exactly the arithmetic
    :func:`predict` applies internally (gp_predict_z); ``chol`` a Cholesky or a PackedLinv."""
    packed = isinstance(chol, PackedLinv)
    L = chol.buf if packed else chol.linv_buf
    dev, batch, n = L.device, L.shape[0], chol.n
    npad = padded_n(n)
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    if out is None:
        out = torch.empty((batch, npad), dtype=F64, device=dev)
    nbytes = int(_capi.lib().gp_predict_z_ws_bytes(n, batch))
    ws = _scratch("z", dev, nbytes)
    _capi.call("gp_predict_z", L.data_ptr(), npad, L.stride(0),
               _capi.LINV_PACKED if packed else _capi.LINV_PADDED, n, w_t.data_ptr(), n,
               out.data_ptr(), out.stride(0) if batch > 1 else npad, batch, ws.data_ptr(),
               ws.numel(), _stream(dev))
    return out


def predict(chol, X: torch.Tensor, Xs: torch.Tensor, beta, s, s_pred, w,
            m_chunk: int = 0, workspace: PredictWorkspace | None = None,
            out: tuple[torch.Tensor, torch.Tensor] | None = None,
            z: torch.Tensor | None = None):
    """Posterior mean / marginal variance at Xs for every problem: returns (batch, m) x 2.

    ``chol`` is a :class:`Cholesky` (padded L^-1) or a :class:`PackedLinv` (read in place);
    ``z`` (or the PackedLinv's own) is L^-1 w from :func:`predict_z`, which then skips the
    library's own (``w`` is not read).  Every form gives bit-identical results (gp_predict_ex).
    """
    packed = isinstance(chol, PackedLinv)
    L = chol.buf if packed else chol.linv_buf
    if z is None and packed:
        z = chol.z
    dev = L.device
    X = _as_f64(X, dev, "X")
    Xs = _as_f64(Xs, dev, "Xs")
    n, d = X.shape
    if n != chol.n:
        raise ValueError("X rows do not match the factorisation")
    m = Xs.shape[0]
    batch = L.shape[0]
    npad = padded_n(n)
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    sp_t = _per_batch(s_pred, batch, dev, "s_pred")
    w_t = None
    if z is None:
        w_t = _as_f64(w, dev, "w")
        if w_t.dim() == 1:
            w_t = w_t.reshape(1, -1)
        if tuple(w_t.shape) != (batch, n):
            raise ValueError(f"w: expected shape ({batch}, {n}), got {tuple(w_t.shape)}")
    else:
        z = z.reshape(batch, -1)
        if z.dtype != F64 or z.device != dev or z.shape[1] < npad or z.stride(1) != 1:
            raise ValueError(f"z: expected float64 ({batch}, {npad}) rows on {dev}")
    if out is None:
        mean = torch.empty((batch, m), dtype=F64, device=dev)
        var = torch.empty((batch, m), dtype=F64, device=dev)
    else:
        mean, var = out
    nbytes = _capi.lib().gp_predict_ws_bytes(n, m, batch, int(m_chunk))
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    _capi.call("gp_predict_ex", L.data_ptr(), npad, L.stride(0) if packed else npad * npad,
               X.data_ptr(), d, Xs.data_ptr(), d, n, m, d, beta_t.data_ptr(), d,
               s_t.data_ptr(), sp_t.data_ptr(), w_t.data_ptr() if w_t is not None else None, n,
               mean.data_ptr(), var.data_ptr(), mean.stride(0) if batch > 1 else m, batch,
               ws.data_ptr(), ws.numel(), int(m_chunk),
               _capi.LINV_PACKED if packed else _capi.LINV_PADDED,
               z.data_ptr() if z is not None else None,
               z.stride(0) if z is not None else 0, _stream(dev))
    return mean, var


def nll(chol: Cholesky, w) -> torch.Tensor:
    """1/2 ||L^-1 w||^2 + 1/2 log|A| per problem (GPmodule objective, no 2pi)."""
    dev = chol.linv_buf.device
    batch = chol.linv_buf.shape[0]
    npad = chol.linv_buf.shape[1]
    n = chol.n
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    out = torch.empty(batch, dtype=F64, device=dev)
    work = torch.empty((batch, n), dtype=F64, device=dev)
    _capi.call("gp_nll", chol.linv_buf.data_ptr(), npad, npad * npad, n, w_t.data_ptr(), n,
               chol.logdet.data_ptr(), out.data_ptr(), work.data_ptr(), batch, _stream(dev))
    return out


class LoglikWorkspace:
    """Device scratch of :func:`loglik` for fixed (n, batch): allocated once, so a Metropolis
    sweep calls gp_loglik with no allocation and no host synchronisation."""

    def __init__(self, n: int, batch: int, device):
        self.n, self.batch = n, batch
        nbytes = int(_capi.lib().gp_loglik_ws_bytes(n, batch))
        # zero-filled: the library's sticky internal-error word starts clear
        self.buf = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=device)
        self.info = torch.zeros(batch, dtype=torch.int32, device=device)

    def check_status(self, reset: bool = True) -> None:
        """Raise :class:`FactorizationInternalError` if any :func:`loglik` on this workspace
        since the last check had an internal factorisation error (gp_loglik_status; syncs the
        current stream).  A non-positive-definite proposal is not an error (ll = -inf)."""
        rc = _capi.lib().gp_loglik_status(self.buf.data_ptr(), self.n, self.batch,
                                          1 if reset else 0, _stream(self.buf.device))
        if rc == _capi.GPFIT_ERR_INTERNAL:
            raise FactorizationInternalError(
                "gp_loglik: a factorisation gave up (info = -1) since the last check; the "
                "chain's likelihood values are invalid")
        if rc != 0:
            raise _capi.GPFitError("gp_loglik_status", rc)


def loglik(X: torch.Tensor, beta: torch.Tensor, s: torch.Tensor, delta: torch.Tensor,
           w: torch.Tensor, ws: LoglikWorkspace, out: torch.Tensor | None = None) -> torch.Tensor:
    """ll[b] = -(1/2 w_b^T G_b^-1 w_b + 1/2 log|G_b|), G_b = s_b exp(-sum beta_b (dx)^2) + delta_b I;
    -inf where G_b is not positive definite (gp_loglik: Gram -> Cholesky -> quadratic form).

    X (n, d); beta (batch, d); s, delta (batch,); w (batch, n) -- all float64 on the device.
    """
    n, d = X.shape
    batch = ws.batch
    if n != ws.n or beta.shape != (batch, d) or w.shape != (batch, n):
        raise ValueError("loglik: shapes do not match the workspace")
    for t, nm in ((X, "X"), (beta, "beta"), (s, "s"), (delta, "delta"), (w, "w")):
        if t.dtype != F64 or not t.is_contiguous():
            raise TypeError(f"{nm} must be contiguous float64")
    out = torch.empty(batch, dtype=F64, device=X.device) if out is None else out
    _capi.call("gp_loglik", X.data_ptr(), n, d, d, beta.data_ptr(), d, s.data_ptr(),
               delta.data_ptr(), w.data_ptr(), n, batch, ws.buf.data_ptr(), ws.buf.numel(),
               out.data_ptr(), ws.info.data_ptr(), _stream(X.device))
    return out


def trmv(chol: Cholesky, w) -> torch.Tensor:
    """z = L^-1 w per problem -> (batch, n)."""
    dev = chol.linv_buf.device
    batch = chol.linv_buf.shape[0]
    npad = chol.linv_buf.shape[1]
    n = chol.n
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    z = torch.empty((batch, n), dtype=F64, device=dev)
    _capi.call("gp_trmv", chol.linv_buf.data_ptr(), npad, npad * npad, n, w_t.data_ptr(), n,
               z.data_ptr(), n, batch, _stream(dev))
    return z


def xval_max_fold() -> int:
    return int(_capi.lib().gp_xval_max_fold())


def _xval_folds(folds, n: int):
    """Validate ``folds`` (a sequence of index sequences) on the host and return the CSR arrays
    (fold_ptr, fold_idx) as int32 numpy, or (None, None) for leave-one-out over all n."""
    if folds is None:
        return None, None
    fmax = xval_max_fold()
    ptr, idx, seen = [0], [], set()
    for k, fold in enumerate(folds):
        fold = [fold] if np.isscalar(fold) else list(fold)
        if len(fold) > fmax:
            raise ValueError(f"folds: fold {k} holds {len(fold)} indices, more than "
                             f"gp_xval_max_fold() = {fmax}")
        for i in fold:
            if int(i) != i:
                raise ValueError(f"folds: index {i!r} of fold {k} is not an integer")
            i = int(i)
            if not 0 <= i < n:
                raise ValueError(f"folds: index {i} of fold {k} is outside [0, {n})")
            if i in seen:
                raise ValueError(f"folds: index {i} appears twice (again in fold {k})")
            seen.add(i)
            idx.append(i)
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


class XvalNotPositiveDefinite(ValueError):
    """A fold's Q_FF was not positive definite (info = fold + 1)."""


def check_xval_info(info: torch.Tensor) -> None:
    """:func:`check_info` for gp_xval's info: fold + 1 for a fold whose Q_FF is not positive
    definite, -2 for a fold the library refused.  Synchronises with the device."""
    vals = info.cpu()
    bad = torch.nonzero(vals).flatten().tolist()
    if not bad:
        return
    refused = [b for b in bad if int(vals[b]) < 0]
    if refused:
        raise ValueError(f"gp_xval refused a fold (info = -2: too large, or an index out of "
                         f"range) for problems {refused}")
    raise XvalNotPositiveDefinite(
        f"Q_FF not positive definite (info = fold + 1 = {vals[bad].tolist()} for problems {bad})")


def _chol_w(chol, w):
    """Validate the (chol, w) pair of :func:`xval` / :func:`alpha` short of the device checks,
    which come after the caller's own: returns (L, dev, batch, n, npad, w), ``w`` as (batch, n)."""
    if not isinstance(chol, Cholesky):
        raise ValueError("chol: expected a kernels.Cholesky (padded L^-1)")
    L = chol.linv_buf
    dev, batch, n = L.device, L.shape[0], chol.n
    npad = padded_n(n)
    if not torch.is_tensor(w) or w.dtype != F64:
        raise ValueError("w: expected a float64 tensor")
    if w.dim() == 1:
        w = w.reshape(1, -1)
    if tuple(w.shape) != (batch, n):
        raise ValueError(f"w: expected shape ({batch}, {n}), got {tuple(w.shape)}")
    if not w.is_contiguous():
        raise ValueError("w: expected a contiguous tensor")
    if L.dtype != F64 or tuple(L.shape) != (batch, npad, npad) or not L.is_contiguous():
        raise ValueError(f"chol: expected a contiguous float64 ({batch}, {npad}, {npad}) L^-1")
    return L, dev, batch, n, npad, w


def xval(chol: Cholesky, w, folds=None, shift=None, out=None, check: bool = True):
    """Cross-validated mean / variance of the training simulations from L^-1, no refit (gp_xval):
    for every fold F, E[w_F | w outside F] and diag Cov - shift.  Returns (mean, var), each
    (batch, n); entries whose index is in no fold are NaN (left as they are in ``out``).

    ``folds``: a sequence of index sequences (each at most :func:`xval_max_fold` long, no index
    twice), or None for leave-one-out; ``shift`` (batch,) or None for 0 (``s + delta - s_pred``
    gives the variance :func:`predict` reports at a new point placed there); ``w`` a contiguous
    float64 (batch, n) device tensor.  Everything is validated on the host before the call;
    ``check`` synchronises and raises like :meth:`Cholesky.check`."""
    L, dev, batch, n, npad, w = _chol_w(chol, w)
    ptr, idx = _xval_folds(folds, n)
    if shift is not None:
        if not torch.is_tensor(shift) or shift.dtype != F64 or shift.numel() != batch or \
                not shift.is_contiguous():
            raise ValueError(f"shift: expected a contiguous float64 tensor of {batch} values")
    if out is not None:
        if len(out) != 2 or any((not torch.is_tensor(t)) or t.dtype != F64 or
                                tuple(t.shape) != (batch, n) or t.stride(1) != 1 or
                                (batch > 1 and t.stride(0) < n) for t in out) or \
                (batch > 1 and out[0].stride(0) != out[1].stride(0)):
            raise ValueError(f"out: expected two float64 ({batch}, {n}) tensors with unit "
                             "column stride and one row stride")
    for t, nm in ((L, "chol"), (w, "w")) + (((shift, "shift"),) if shift is not None else ()) + \
            (tuple((t, "out") for t in out) if out is not None else ()):
        _check_device(t, nm)
    if out is None:
        mean = torch.full((batch, n), float("nan"), dtype=F64, device=dev)
        var = torch.full((batch, n), float("nan"), dtype=F64, device=dev)
    else:
        mean, var = out
    ptr_t = idx_t = None
    nfolds = nidx = 0
    if ptr is not None:
        nfolds, nidx = len(ptr) - 1, len(idx)
        ptr_t = torch.as_tensor(ptr, device=dev)
        # never an empty allocation: the library wants a pointer when folds are given
        idx_t = torch.zeros(max(nidx, 1), dtype=torch.int32, device=dev)
        if nidx:
            idx_t[:nidx] = torch.as_tensor(idx, device=dev)
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    nbytes = int(_capi.lib().gp_xval_ws_bytes(n, nfolds, nidx, batch))
    ws = _scratch("xval", dev, nbytes)
    _capi.call("gp_xval", L.data_ptr(), npad, npad * npad, n, w.data_ptr(), n,
               ptr_t.data_ptr() if ptr_t is not None else None,
               idx_t.data_ptr() if idx_t is not None else None, nfolds, nidx,
               shift.data_ptr() if shift is not None else None, mean.data_ptr(), var.data_ptr(),
               mean.stride(0) if batch > 1 else n, info.data_ptr(), batch, ws.data_ptr(),
               ws.numel(), _stream(dev))
    if check:
        check_xval_info(info)
    return mean, var


RESP_ORDER = {"cyclic": 0, "ascending": 1}     # GPFIT_RESP_CYCLIC / GPFIT_RESP_ASCENDING
RESP_MAX_EFFECTS = 64                          # GPFIT_RESP_MAX_EFFECTS


def alpha(chol: Cholesky, w, out: torch.Tensor | None = None) -> torch.Tensor:
    """alpha = A^-1 w = L^-T (L^-1 w) per problem -> (batch, n) (gp_alpha): the weights of the
    posterior mean, which :func:`mean_response` contracts.  ``w`` a contiguous float64
    (batch, n) device tensor; ``out`` a float64 (batch, n) tensor with unit column stride."""
    L, dev, batch, n, npad, w = _chol_w(chol, w)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != F64 or tuple(out.shape) != (batch, n) or \
                (n > 1 and out.stride(1) != 1) or (batch > 1 and out.stride(0) < n):
            raise ValueError(f"out: expected a float64 ({batch}, {n}) tensor with unit column "
                             "stride")
    for t, nm in ((L, "chol"), (w, "w")) + (((out, "out"),) if out is not None else ()):
        _check_device(t, nm)
    if out is None:
        out = torch.empty((batch, n), dtype=F64, device=dev)
    if n == 0 or batch == 0:
        return out
    nbytes = int(_capi.lib().gp_alpha_ws_bytes(n, batch))
    ws = _scratch("alpha", dev, nbytes)
    _capi.call("gp_alpha", L.data_ptr(), npad, npad * npad, n, w.data_ptr(), n, out.data_ptr(),
               out.stride(0) if batch > 1 else n, batch, ws.data_ptr(), ws.numel(), _stream(dev))
    return out


_alpha = alpha            # nll_grad's keyword of the same name hides the function


def nll_grad(chol: Cholesky, X, beta, s, w, alpha: torch.Tensor | None = None) -> torch.Tensor:
    """Gradient of :func:`nll` in the kernel's parameters per problem -> (batch, d + 2), in the
    order [d/ds, d/ddelta, d/dbeta_0 .. d/dbeta_{d-1}] (gp_nll_grad), from the L^-1 of
    :func:`cholesky_inverse` with the same X, beta, s.

    ``X`` (n, d), ``beta`` (batch, d), ``s`` (batch,), ``w`` (batch, n): contiguous float64
    device tensors; ``alpha`` (batch, n) from :func:`alpha`, computed here when not given.  A
    problem whose factorisation reported info != 0 has an unspecified gradient."""
    L, dev, batch, n, npad, w = _chol_w(chol, w)
    _f64_tensor(X, "X", f"({n}, d) with 1 <= d", lambda t: t.dim() == 2 and t.shape[0] == n and
                t.shape[1] >= 1)
    d = X.shape[1]
    _f64_tensor(beta, "beta", f"({batch}, {d})", lambda t: tuple(t.shape) == (batch, d))
    _f64_tensor(s, "s", f"({batch},)", lambda t: tuple(t.shape) == (batch,))
    if alpha is not None:
        _f64_tensor(alpha, "alpha", f"({batch}, {n})", lambda t: tuple(t.shape) == (batch, n))
    for t, nm in ((L, "chol"), (w, "w"), (X, "X"), (beta, "beta"), (s, "s")) + \
            (((alpha, "alpha"),) if alpha is not None else ()):
        _check_device(t, nm)
    out = torch.empty((batch, d + 2), dtype=F64, device=dev)
    if n == 0 or batch == 0:
        return out.zero_()
    if alpha is None:
        alpha = _alpha(chol, w)
    nbytes = int(_capi.lib().gp_nll_grad_ws_bytes(n, d, batch))
    ws = _scratch("nll_grad", dev, nbytes)
    _capi.call("gp_nll_grad", L.data_ptr(), npad, npad * npad, X.data_ptr(), d, n, d,
               beta.data_ptr(), d, s.data_ptr(), alpha.data_ptr(), n, out.data_ptr(), d + 2,
               batch, ws.data_ptr(), ws.numel(), _stream(dev))
    return out


def nll_value_grad(X, beta, s, delta, w):
    """Value and gradient of the likelihood of ``batch`` GPs on one design -> (nll, grad, info):
    Gram -> :func:`cholesky_inverse` -> :func:`nll` -> :func:`alpha` -> :func:`nll_grad`, with
    no host synchronisation.  ``nll`` (batch,), ``grad`` (batch, d + 2) as :func:`nll_grad`,
    ``info`` (batch,) int32 the factorisation's; a problem with info != 0 (K not positive
    definite) has NaN in ``nll`` and in its row of ``grad``, set on the device.

    ``X`` (n, d), ``beta`` (batch, d), ``s``, ``delta`` (batch,), ``w`` (batch, n): contiguous
    float64 device tensors."""
    _f64_tensor(X, "X", "(n, d) with 1 <= d", lambda t: t.dim() == 2 and t.shape[1] >= 1)
    n, d = X.shape
    _f64_tensor(beta, "beta", f"(batch, {d})", lambda t: t.dim() == 2 and t.shape[1] == d)
    batch = beta.shape[0]
    _f64_tensor(s, "s", f"({batch},)", lambda t: tuple(t.shape) == (batch,))
    _f64_tensor(delta, "delta", f"({batch},)", lambda t: tuple(t.shape) == (batch,))
    _f64_tensor(w, "w", f"({batch}, {n})", lambda t: tuple(t.shape) == (batch, n))
    for t, nm in ((X, "X"), (beta, "beta"), (s, "s"), (delta, "delta"), (w, "w")):
        _check_device(t, nm)
    ch = cholesky_inverse(gram(X, beta, s, delta, batch=batch))
    val = nll(ch, w)
    grad = nll_grad(ch, X, beta, s, w, alpha(ch, w))
    bad = ch.info != 0
    nan = torch.full((), float("nan"), dtype=F64, device=X.device)
    return torch.where(bad, nan, val), torch.where(bad[:, None], nan, grad), ch.info


def mean_response_max_grid() -> int:
    return int(_capi.lib().gp_mean_response_max_grid())


def mean_response_max_int_elems() -> int:
    return int(_capi.lib().gp_mean_response_max_int_elems())


def _f64_tensor(t, name: str, shape_txt: str, ok) -> None:
    if not torch.is_tensor(t) or t.dtype != F64:
        raise ValueError(f"{name}: expected a float64 tensor")
    if not ok(t):
        raise ValueError(f"{name}: expected shape {shape_txt}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")


def mean_response(X, alpha, beta, s, effects, t1, t2=None, Xint=None, order: str = "ascending",
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Mean-response surfaces of ``batch`` GPs in closed form (gp_mean_response): for every effect
    the posterior mean at x_d1 = t1[a1] (and x_d2 = t2[a2]) averaged over the integration points
    ``Xint`` placed in the other dimensions.  Returns (batch, E, T1) for main effects,
    (batch, E, T2, T1) for pairs.

    ``X`` (n, d), ``alpha`` (batch, n) from :func:`alpha`, ``beta`` (batch, d), ``s`` (batch,),
    ``t1`` (T1,), ``t2`` (T2,), ``Xint`` (I, d - nfree): contiguous float64 device tensors.
    ``effects``: a sequence of dimensions (main effects) or of (d1, d2) pairs, on the host; more
    than 64 are split over several calls.  ``order``: "cyclic" (integration column c takes
    dimension (d1 + 1 + c) mod d; main effects only) or "ascending" (the non-free dimensions in
    ascending order).  ``Xint`` may be None when every dimension is free (d == nfree).  ``out``:
    a contiguous float64 tensor of the result's shape."""
    _f64_tensor(X, "X", "(n, d)", lambda t: t.dim() == 2 and t.shape[1] >= 1)
    n, d = X.shape
    _f64_tensor(alpha, "alpha", f"(batch, {n})", lambda t: t.dim() == 2 and t.shape[1] == n)
    batch = alpha.shape[0]
    _f64_tensor(beta, "beta", f"({batch}, {d})", lambda t: tuple(t.shape) == (batch, d))
    _f64_tensor(s, "s", f"({batch},)", lambda t: tuple(t.shape) == (batch,))
    try:
        eff = np.asarray(effects)
        if eff.size and not np.issubdtype(eff.dtype, np.integer):
            if not np.all(eff == np.floor(eff)):
                raise ValueError
        eff = eff.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError("effects: expected a sequence of dimensions or of (d1, d2) pairs") \
            from None
    if eff.ndim == 0 or eff.ndim > 2 or (eff.ndim == 2 and eff.shape[1] not in (1, 2)):
        raise ValueError("effects: expected a sequence of dimensions or of (d1, d2) pairs")
    nfree = 1 if eff.ndim == 1 else int(eff.shape[1])
    eff = eff.reshape(-1, nfree)
    E = eff.shape[0]
    if ((eff < 0) | (eff >= d)).any():
        raise ValueError(f"effects: a dimension lies outside [0, {d})")
    if nfree == 2 and (eff[:, 0] == eff[:, 1]).any():
        raise ValueError("effects: a pair frees one dimension twice")
    if order not in RESP_ORDER:
        raise ValueError(f"order: expected 'cyclic' or 'ascending', got {order!r}")
    if order == "cyclic" and nfree == 2:
        raise ValueError("order: 'cyclic' is the main effects' rule; pairs take 'ascending'")
    tmax = mean_response_max_grid()
    _f64_tensor(t1, "t1", f"(T1,) with 1 <= T1 <= {tmax}",
                lambda t: t.dim() == 1 and 1 <= t.numel() <= tmax)
    T1, T2 = t1.numel(), 1
    if nfree == 2:
        if t2 is None:
            raise ValueError("t2: pairs need the second dimension's targets")
        _f64_tensor(t2, "t2", f"(T2,) with 1 <= T2 <= {tmax}",
                    lambda t: t.dim() == 1 and 1 <= t.numel() <= tmax)
        T2 = t2.numel()
    elif t2 is not None:
        raise ValueError("t2: main effects take t1 only")
    nc = d - nfree
    if nc < 0:
        raise ValueError(f"effects: pairs need d >= 2, got d = {d}")
    I = 0
    if nc > 0:
        if Xint is None:
            raise ValueError(f"Xint: expected the (I, {nc}) integration points")
        _f64_tensor(Xint, "Xint", f"(I, {nc}) with I >= 1",
                    lambda t: t.dim() == 2 and t.shape[1] == nc and t.shape[0] >= 1)
        I = Xint.shape[0]
        if I * nc > mean_response_max_int_elems():
            raise ValueError(f"Xint: {I} x {nc} values exceed "
                             f"gp_mean_response_max_int_elems() = {mean_response_max_int_elems()}")
    elif Xint is not None:
        raise ValueError("Xint: every dimension is free, there is nothing to integrate")
    shape = (batch, E, T1) if nfree == 1 else (batch, E, T2, T1)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != F64 or tuple(out.shape) != shape or \
                not out.is_contiguous():
            raise ValueError(f"out: expected a contiguous float64 {shape} tensor")
    ops = [(X, "X"), (alpha, "alpha"), (beta, "beta"), (s, "s"), (t1, "t1")]
    ops += [(t, nm) for t, nm in ((t2, "t2"), (Xint, "Xint"), (out, "out")) if t is not None]
    for t, nm in ops:
        _check_device(t, nm)
    dev = X.device
    if out is None:
        out = torch.empty(shape, dtype=F64, device=dev)
    if n == 0:
        return out.zero_()
    if batch == 0 or E == 0:
        return out
    import ctypes
    TT = T1 * T2
    for e0 in range(0, E, RESP_MAX_EFFECTS):
        ne = min(E - e0, RESP_MAX_EFFECTS)
        host = (ctypes.c_int * (ne * nfree))(*[int(v) for v in eff[e0:e0 + ne].reshape(-1)])
        _capi.call("gp_mean_response", X.data_ptr(), n, d, d, alpha.data_ptr(), n,
                   beta.data_ptr(), d, s.data_ptr(), batch, ctypes.addressof(host), nfree, ne,
                   RESP_ORDER[order], t1.data_ptr(), T1,
                   t2.data_ptr() if t2 is not None else None, T2,
                   Xint.data_ptr() if Xint is not None else None, I, max(nc, 1),
                   out.data_ptr() + 8 * e0 * TT, TT, E * TT, _stream(dev))
    return out


def sobol_exact(X, alpha, beta, s, group: int = 1, lo=None, hi=None, out=None):
    """Closed-form Sobol' ingredients of the posterior means of ``U`` GPs under uniform inputs on
    the box ``[lo, hi]`` (gp_sobol_exact).  The units are G = U / ``group`` groups of M = ``group``
    consecutive units.  Returns ``(E, Q)``: ``E`` (U,) the units' means and ``Q`` (G, M, M,
    2 d + 1) per pair of units of one group ``[tot, main_0 .. main_{d-1}, not_0 .. not_{d-1}]`` =
    E[f_a f_b], E[E[f_a|x_i] E[f_b|x_i]], E[E[f_a|x_~i] E[f_b|x_~i]] (include/gpfit.h).

    ``X`` (n, d), ``alpha`` (U, n) from :func:`alpha`, ``beta`` (U, d), ``s`` (U,): contiguous
    float64 device tensors.  ``lo`` / ``hi``: (d,) float64 device tensors with ``hi > lo`` (checked
    here: one host synchronisation), or both None for the unit box.  ``out``: a pair of contiguous
    float64 tensors of the results' shapes."""
    _f64_tensor(X, "X", "(n, d) with 1 <= d", lambda t: t.dim() == 2 and t.shape[1] >= 1)
    n, d = X.shape
    _f64_tensor(alpha, "alpha", f"(U, {n})", lambda t: t.dim() == 2 and t.shape[1] == n)
    U = alpha.shape[0]
    _f64_tensor(beta, "beta", f"({U}, {d})", lambda t: tuple(t.shape) == (U, d))
    _f64_tensor(s, "s", f"({U},)", lambda t: tuple(t.shape) == (U,))
    if d > 32:
        raise ValueError(f"X: d = {d} exceeds GPFIT_MAX_DIM = 32")
    if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or group < 1:
        raise ValueError(f"group: expected an integer >= 1, got {group!r}")
    M = int(group)
    if U % M:
        raise ValueError(f"group: {U} units are no whole number of groups of {M}")
    G = U // M
    if (lo is None) != (hi is None):
        raise ValueError("lo, hi: give both bounds or neither")
    if lo is not None:
        _f64_tensor(lo, "lo", f"({d},)", lambda t: tuple(t.shape) == (d,))
        _f64_tensor(hi, "hi", f"({d},)", lambda t: tuple(t.shape) == (d,))
    shapes = ((U,), (G, M, M, 2 * d + 1))
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or any(
                not torch.is_tensor(o) or o.dtype != F64 or tuple(o.shape) != sh or
                not o.is_contiguous() for o, sh in zip(out, shapes)):
            raise ValueError(f"out: expected contiguous float64 tensors of shapes {shapes}")
    ops = [(X, "X"), (alpha, "alpha"), (beta, "beta"), (s, "s")]
    ops += [(t, nm) for t, nm in ((lo, "lo"), (hi, "hi")) if t is not None]
    ops += [(o, "out") for o in (out or ())]
    for t, nm in ops:
        _check_device(t, nm)
    if lo is not None and not bool((hi > lo).all()):
        raise ValueError("lo, hi: every hi must exceed its lo")
    dev = X.device
    E, Q = out if out is not None else (torch.empty(sh, dtype=F64, device=dev) for sh in shapes)
    if U == 0:
        return E, Q
    nq = 2 * d + 1
    nbytes = int(_capi.lib().gp_sobol_exact_ws_bytes(n, d, G, M))
    ws = _scratch("sobol_exact", dev, nbytes) if nbytes else None
    _capi.call("gp_sobol_exact", X.data_ptr(), n, d, d, G, M, alpha.data_ptr(), n,
               beta.data_ptr(), d, s.data_ptr(), lo.data_ptr() if lo is not None else None,
               hi.data_ptr() if hi is not None else None, E.data_ptr(), 1, Q.data_ptr(), nq,
               M * nq, M * M * nq, ws.data_ptr() if ws is not None else None,
               ws.numel() if ws is not None else 0, _stream(dev))
    return E, Q


@dataclass
class Prepared:
    """Cross-covariance of every test-point chunk, built by :func:`predict_prepare`."""

    n: int
    m: int
    batch: int
    m_chunk: int
    ws: torch.Tensor


def predict_prepare(X: torch.Tensor, Xs: torch.Tensor, beta, s, batch: int = 1,
                    m_chunk: int = 0, workspace: PredictWorkspace | None = None) -> Prepared:
    """Phase 1 of predict (gp_predict_cross): independent of the factorisation, so it can run
    on a side stream while :func:`cholesky_inverse` runs."""
    dev = X.device
    X = _as_f64(X, dev, "X")
    Xs = _as_f64(Xs, dev, "Xs")
    n, d = X.shape
    m = Xs.shape[0]
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    nbytes = _capi.lib().gp_predict_prepared_ws_bytes(n, m, batch, int(m_chunk))
    ws = (workspace or PredictWorkspace()).get(nbytes, dev)
    _capi.call("gp_predict_cross", X.data_ptr(), d, Xs.data_ptr(), d, n, m, d, beta_t.data_ptr(),
               d, s_t.data_ptr(), batch, ws.data_ptr(), ws.numel(), int(m_chunk), _stream(dev))
    return Prepared(n, m, batch, int(m_chunk), ws)


def predict_solve(chol: Cholesky, prep: Prepared, s_pred, w,
                  out: tuple[torch.Tensor, torch.Tensor] | None = None):
    """Phase 2 of predict (gp_predict_solve): mean / variance from a prepared cross-cov."""
    dev = chol.linv_buf.device
    batch, npad = chol.linv_buf.shape[0], chol.linv_buf.shape[1]
    n, m = chol.n, prep.m
    if prep.n != n or prep.batch != batch:
        raise ValueError("prepared cross-covariance does not match the factorisation")
    sp_t = _per_batch(s_pred, batch, dev, "s_pred")
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    if out is None:
        mean = torch.empty((batch, m), dtype=F64, device=dev)
        var = torch.empty((batch, m), dtype=F64, device=dev)
    else:
        mean, var = out
    _capi.call("gp_predict_solve", chol.linv_buf.data_ptr(), npad, npad * npad, n, m,
               sp_t.data_ptr(), w_t.data_ptr(), n, mean.data_ptr(), var.data_ptr(),
               mean.stride(0) if batch > 1 else m, batch, prep.ws.data_ptr(), prep.ws.numel(),
               prep.m_chunk, _stream(dev))
    return mean, var


class FitPredictContext:
    """Caller-owned execution context of :func:`fit_predict` (``gp_ctx_create``): the three
    library streams (factorisation | cross-covariance | prediction) on ``device``.

    Destroy it with :meth:`close` (or use it as a context manager) while the HIP runtime is up:
    the owner decides the teardown order, the library keeps no global state.
    """

    def __init__(self, device=None, cross_start: float = -1.0, aux_free_cus: int = -1,
                 aux_chunks: int = -1):
        import ctypes
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda", torch.cuda.current_device())
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _capi.call("gp_ctx_create", float(cross_start), int(aux_free_cus),
                       ctypes.addressof(self._h))
            if aux_chunks != -1:
                self.set_aux_chunks(aux_chunks)

    def set_aux_chunks(self, nchunks: int) -> None:
        """Chunks whose cross-covariance runs beside the factorisation / earlier TRMMs
        (``gp_ctx_set_aux_chunks``; -1 = all, the default)."""
        _capi.call("gp_ctx_set_aux_chunks", self._h.value, int(nchunks))

    @property
    def handle(self) -> int | None:
        return self._h.value

    def close(self) -> None:
        if self._h.value:
            with torch.cuda.device(self.device):
                _capi.call("gp_ctx_destroy", self._h.value)
            self._h.value = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def fit_predict(X, Xs, beta, s, delta, s_pred, w, m_chunk: int = 0,
                workspace: PredictWorkspace | None = None, out=None,
                ctx: FitPredictContext | None = None, check: bool = True):
    """Gram -> Cholesky/L^-1 -> predict for ``batch`` GPs in one gp_fit_predict call.

    With ``ctx`` the cross-covariance runs on the context's own stream under the
    factorisation's latency-bound tail, then the per-chunk TRMM + mean/var; without it every
    step runs in order on the current stream.  ``check`` synchronises and raises if a Gram was
    not positive definite or its factorisation had an internal error (info = -1): the mean /
    var would be unspecified.  Returns (mean, var, chol).
    """
    dev = X.device
    X = _as_f64(X, dev, "X")
    Xs = _as_f64(Xs, dev, "Xs")
    n, d = X.shape
    m = Xs.shape[0]
    bt = torch.as_tensor(beta)
    batch = bt.shape[0] if bt.dim() == 2 else 1
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    d_t = _per_batch(delta, batch, dev, "delta")
    sp_t = _per_batch(s_pred, batch, dev, "s_pred")
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    npad = padded_n(n)
    G = torch.empty((batch, n, n), dtype=F64, device=dev)
    Linv = torch.empty((batch, npad, npad), dtype=F64, device=dev)
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    logdet = torch.empty(batch, dtype=F64, device=dev)
    if out is None:
        mean = torch.empty((batch, m), dtype=F64, device=dev)
        var = torch.empty((batch, m), dtype=F64, device=dev)
    else:
        mean, var = out
    nbytes = _capi.lib().gp_fit_predict_ws_bytes(n, m, batch, int(m_chunk))
    ws = (workspace or PredictWorkspace()).get(nbytes, dev)
    if ctx is not None and ctx.device != dev:
        raise ValueError(f"context is on {ctx.device}, inputs on {dev}")
    _capi.call("gp_fit_predict", X.data_ptr(), d, Xs.data_ptr(), d, n, m, d, beta_t.data_ptr(),
               d, s_t.data_ptr(), d_t.data_ptr(), sp_t.data_ptr(), w_t.data_ptr(), n,
               G.data_ptr(), n, n * n, Linv.data_ptr(), npad, npad * npad, info.data_ptr(),
               logdet.data_ptr(), mean.data_ptr(), var.data_ptr(),
               mean.stride(0) if batch > 1 else m, batch, ws.data_ptr(), ws.numel(),
               int(m_chunk), ctx.handle if ctx is not None else None, _stream(dev))
    ch = Cholesky(n, G, Linv, info, logdet)
    if check:
        ch.check()
    return mean, var, ch


def cholesky(G: torch.Tensor, overwrite: bool = True):
    """Plain blocked Cholesky (gp_potrf, LAPACK dpotrf('L')): returns (L, info, logdet) with L
    the lower factor as a (batch, n, n) logical tensor."""
    _check_device(G, "G")
    if G.dtype != F64:
        raise TypeError("G must be float64")
    if G.dim() == 2:
        G = G.unsqueeze(0)
    batch, n, n2 = G.shape
    if n != n2:
        raise ValueError("G must be square")
    A = G if (overwrite and G.is_contiguous()) else G.contiguous().clone()
    info = torch.empty(batch, dtype=torch.int32, device=G.device)
    logdet = torch.empty(batch, dtype=F64, device=G.device)
    nbytes = int(_capi.lib().gp_potrf_ws_bytes(n, batch))
    ws = _scratch("potrf", G.device, nbytes)
    _capi.call("gp_potrf_ws", A.data_ptr(), n, n, n * n, batch, info.data_ptr(),
               logdet.data_ptr(), ws.data_ptr(), ws.numel(), _stream(G.device))
    return torch.tril(A.transpose(-1, -2)), info, logdet


def _lapack_buf(L: torch.Tensor) -> torch.Tensor:
    """(batch, n, n) logical lower factor -> contiguous column-major buffer [b, j, i] = L[i, j]."""
    _check_device(L, "L")
    if L.dim() == 2:
        L = L.unsqueeze(0)
    return L.to(F64).transpose(-1, -2).contiguous()


def trtri(L: torch.Tensor) -> Cholesky:
    """L^-1 of a lower factor (gp_trtri, LAPACK dtrtri('L','N')); returns a :class:`Cholesky`
    whose ``info`` flags a zero diagonal, usable with :func:`predict` / :func:`nll`."""
    Lb = _lapack_buf(L)
    batch, n, _ = Lb.shape
    npad = padded_n(n)
    Linv = torch.empty((batch, npad, npad), dtype=F64, device=Lb.device)
    info = torch.empty(batch, dtype=torch.int32, device=Lb.device)
    _capi.call("gp_trtri", Lb.data_ptr(), n, n, n * n, Linv.data_ptr(), npad, npad * npad, batch,
               info.data_ptr(), _stream(Lb.device))
    logdet = 2.0 * torch.log(torch.diagonal(Lb, dim1=-2, dim2=-1)).sum(-1)
    return Cholesky(n, Lb, Linv, info, logdet)


def predict_chol(L: torch.Tensor, X, Xs, beta, s, s_pred, w, m_chunk: int = 0,
                 workspace: PredictWorkspace | None = None):
    """Posterior mean / variance from a Cholesky factor L (gp_predict_chol: gp_trtri into the
    workspace, then gp_predict).  Returns (mean, var, info)."""
    Lb = _lapack_buf(L)
    dev = Lb.device
    batch, n, _ = Lb.shape
    X = _as_f64(X, dev, "X")
    Xs = _as_f64(Xs, dev, "Xs")
    d = X.shape[1]
    m = Xs.shape[0]
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    sp_t = _per_batch(s_pred, batch, dev, "s_pred")
    w_t = _as_f64(w, dev, "w").reshape(batch, n)
    mean = torch.empty((batch, m), dtype=F64, device=dev)
    var = torch.empty((batch, m), dtype=F64, device=dev)
    info = torch.empty(batch, dtype=torch.int32, device=dev)
    nbytes = _capi.lib().gp_predict_chol_ws_bytes(n, m, batch, int(m_chunk))
    ws = (workspace or PredictWorkspace()).get(nbytes, dev)
    _capi.call("gp_predict_chol", Lb.data_ptr(), n, n * n, X.data_ptr(), d, Xs.data_ptr(), d, n,
               m, d, beta_t.data_ptr(), d, s_t.data_ptr(), sp_t.data_ptr(), w_t.data_ptr(), n,
               mean.data_ptr(), var.data_ptr(), m, batch, info.data_ptr(), ws.data_ptr(),
               ws.numel(), int(m_chunk), _stream(dev))
    return mean, var, info


def realize(mean: torch.Tensor, var: torch.Tensor, seed: int, offset: int = 0,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """One marginal draw per entry, mean + sqrt(max(var, 0)) z with z from Philox4x32-10 keyed
    by ``seed`` at counter offset ``offset`` (gp_realize); deterministic per (seed, offset)."""
    _check_device(mean, "mean")
    if mean.dtype != F64 or var.dtype != F64 or mean.shape != var.shape:
        raise TypeError("mean / var must be float64 tensors of one shape")
    mean_c, var_c = mean.contiguous(), var.contiguous()
    out = torch.empty_like(mean_c) if out is None else out
    _capi.call("gp_realize", mean_c.data_ptr(), var_c.data_ptr(), mean_c.numel(),
               int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), out.data_ptr(),
               _stream(mean.device))
    return out


class JointNotPositiveDefinite(ValueError):
    """A joint predictive covariance is not numerically positive definite (gp_potrf info > 0):
    ``units`` lists the failing problems as (index, pivot) pairs."""

    def __init__(self, msg: str, units):
        super().__init__(msg)
        self.units = list(units)


def check_joint_info(info: torch.Tensor, unit0: int = 0, P: int | None = None,
                     jitter=None) -> None:
    """Raise :class:`JointNotPositiveDefinite` for every problem of a joint covariance whose
    factorisation met a non-positive pivot, naming unit ``unit0 + b`` (as (sample, PC) when
    ``P`` is given) and the jitter in force; info = -1 is the factorisation's internal error.
    Synchronises with the device."""
    vals = info.cpu().tolist()
    if any(v < 0 for v in vals):
        check_info(info)
    bad = [(unit0 + b, v) for b, v in enumerate(vals) if v > 0]
    if not bad:
        return
    name = (lambda u: f"(sample {u // P}, PC {u % P})") if P else (lambda u: f"unit {u}")
    txt = ", ".join(f"{name(u)} at pivot {v}" for u, v in bad[:8])
    more = f" and {len(bad) - 8} more" if len(bad) > 8 else ""
    now = "0" if jitter is None else f"{jitter:g}"
    raise JointNotPositiveDefinite(
        f"joint predictive covariance not positive definite for {txt}{more} with "
        f"joint_jitter = {now} (a multiple of s): raise joint_jitter (1e-8 is the default without "
        "the prediction nugget; duplicated test points or a test point on a training point need "
        "one), nothing was retried", bad)


def predict_cov(chol: Cholesky, X: torch.Tensor, Xs: torch.Tensor, beta, s, s_pred, jitter=None,
                out: torch.Tensor | None = None,
                workspace: Workspace | None = None) -> torch.Tensor:
    """Joint predictive covariance of the m test points per problem, (batch, m, m), both
    triangles with the same bits (gp_predict_cov):
    C = K** + (s_pred + jitter - s) I - (L^-1 K*)^T (L^-1 K*).  ``jitter``: one value per problem
    added to the diagonal (None = 0).  ``out``: a (batch, m, m) float64 tensor whose last
    dimension is contiguous (row stride >= m, problem stride >= m rows); only the m x m blocks
    are written."""
    L = chol.linv_buf
    dev = L.device
    X = _as_f64(X, dev, "X")
    Xs = _as_f64(Xs, dev, "Xs")
    n, d = X.shape
    if n != chol.n:
        raise ValueError("X rows do not match the factorisation")
    if Xs.dim() != 2 or Xs.shape[1] != d:
        raise ValueError(f"Xs: expected (m, {d}), got {tuple(Xs.shape)}")
    m = Xs.shape[0]
    batch = L.shape[0]
    npad = padded_n(n)
    beta_t = _beta(beta, batch, d, dev)
    s_t = _per_batch(s, batch, dev, "s")
    sp_t = _per_batch(s_pred, batch, dev, "s_pred")
    j_t = None if jitter is None else _per_batch(jitter, batch, dev, "jitter")
    if out is None:
        out = torch.empty((batch, m, m), dtype=F64, device=dev)
    else:
        _check_device(out, "out")
        if (out.dtype != F64 or tuple(out.shape) != (batch, m, m) or
                (m > 1 and (out.stride(2) != 1 or out.stride(1) < m)) or
                (batch > 1 and m > 0 and out.stride(0) < out.stride(1) * m)):
            raise ValueError(f"out: expected float64 ({batch}, {m}, {m}) with contiguous rows")
    if m == 0 or batch == 0:
        return out
    ldc = out.stride(1) if m > 1 else max(1, m)
    nbytes = int(_capi.lib().gp_predict_cov_ws_bytes(n, m, batch))
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    _capi.call("gp_predict_cov", L.data_ptr(), L.stride(1), L.stride(0), X.data_ptr(), d,
               Xs.data_ptr(), d, n, m, d, beta_t.data_ptr(), d, s_t.data_ptr(), sp_t.data_ptr(),
               j_t.data_ptr() if j_t is not None else None, out.data_ptr(), ldc,
               out.stride(0) if batch > 1 else ldc * m, batch, ws.data_ptr(), ws.numel(),
               _stream(dev))
    return out


def cholesky_inplace(A: torch.Tensor):
    """gp_potrf on a contiguous (batch, n, n) column-major buffer in place: the lower factor in
    ``A[b, j, i]`` for i >= j, the other triangle untouched.  Returns (info, logdet)."""
    _check_device(A, "A")
    if A.dtype != F64 or A.dim() != 3 or A.shape[1] != A.shape[2] or not A.is_contiguous():
        raise TypeError("A must be a contiguous float64 (batch, n, n) tensor")
    batch, n, _ = A.shape
    info = torch.zeros(batch, dtype=torch.int32, device=A.device)
    logdet = torch.empty(batch, dtype=F64, device=A.device)
    nbytes = int(_capi.lib().gp_potrf_ws_bytes(n, batch))
    ws = _scratch("potrf", A.device, nbytes)
    _capi.call("gp_potrf_ws", A.data_ptr(), n, n, n * n, batch, info.data_ptr(),
               logdet.data_ptr(), ws.data_ptr(), ws.numel(), _stream(A.device))
    return info, logdet


def mvn_draw(R: torch.Tensor, mean, seed: int, offset: int = 0, nsamp: int = 1,
             unit0: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """Joint draws mean + tril(R) xi per problem: (batch, nsamp, m) (gp_mvn_draw).

    ``R`` is the column-major buffer gp_potrf leaves (:func:`cholesky_inplace`), (batch, m, m)
    with ``R[b, k, i]`` the factor's element (i, k) for i >= k; the other triangle is never read.
    ``mean`` is (batch, m) or None.  The normals are elements ((unit0 + b) nsamp + r) m + k of
    gp_realize's stream for (seed, offset), so splitting a batch over calls with matching
    ``unit0`` gives the bits of one call."""
    _check_device(R, "R")
    if R.dtype != F64 or R.dim() != 3 or R.shape[1] != R.shape[2] or not R.is_contiguous():
        raise TypeError("R must be a contiguous float64 (batch, m, m) tensor")
    batch, m, _ = R.shape
    dev = R.device
    nsamp = int(nsamp)
    if nsamp < 0 or int(unit0) < 0:
        raise ValueError("nsamp and unit0 must be non-negative")
    mean_t = None
    if mean is not None:
        mean_t = _as_f64(mean, dev, "mean").reshape(batch, m)
    if out is None:
        out = torch.empty((batch, nsamp, m), dtype=F64, device=dev)
    elif out.dtype != F64 or tuple(out.shape) != (batch, nsamp, m) or not out.is_contiguous():
        raise ValueError(f"out: expected contiguous float64 ({batch}, {nsamp}, {m})")
    if m == 0 or nsamp == 0 or batch == 0:
        return out
    _capi.call("gp_mvn_draw", R.data_ptr(), max(1, m), m * m, m,
               mean_t.data_ptr() if mean_t is not None else None, m, nsamp,
               int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(unit0),
               out.data_ptr(), max(1, m), batch, _stream(dev))
    return out
