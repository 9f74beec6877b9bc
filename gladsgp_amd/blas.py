"""Column-major fp64 dense helpers over libgpfit (GEMM, statistics, eigensolver).

A column-major (rows x cols) matrix is a torch tensor ``t`` of shape (cols, ld) with element
(i, j) at ``t[j, i]`` — i.e. the row-major view of its transpose.  :class:`CM` carries the
logical shape and leading dimension so the GEMM call reads like BLAS.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi
from .kernels import F64, _stream


@dataclass
class CM:
    """Column-major view: logical ``rows x cols`` with leading dimension ``ld``."""

    t: torch.Tensor
    rows: int
    cols: int
    ld: int

    @property
    def f32(self) -> bool:
        """Stored as float32 (read by gp_gemm_ex and widened to fp64 on load)."""
        return self.t.dtype == torch.float32

    @staticmethod
    def empty(rows: int, cols: int, device) -> "CM":
        t = torch.empty((max(cols, 1), max(rows, 1)), dtype=F64, device=device)
        return CM(t, rows, cols, max(rows, 1))

    @staticmethod
    def of_rowmajor(a: torch.Tensor) -> "CM":
        """A C-order (r x c) tensor seen column-major is its transpose: (c x r), ld = c -- or,
        for a row-strided view (unit column stride, row stride >= c: the ensemble's padded
        y_std), ld = its row stride, without a copy."""
        if a.dim() == 2 and a.shape[0] > 1 and a.shape[1] > 0 and a.stride(1) == 1 and \
                a.stride(0) >= a.shape[1]:
            return CM(a, a.shape[1], a.shape[0], a.stride(0))
        a = a.contiguous()
        r, c = a.shape
        return CM(a, c, r, c)

    def rowmajor_T(self) -> torch.Tensor:
        """The logical matrix transposed, as a C-order torch tensor (cols x rows) view."""
        return self.t[: self.cols, : self.rows]

    def logical(self) -> torch.Tensor:
        return self.rowmajor_T().transpose(0, 1)

    def ptr(self) -> int:
        return self.t.data_ptr()


_WS: dict = {}


def _ws(nbytes: int, device) -> torch.Tensor | None:
    if nbytes <= 0:
        return None
    key = str(device)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def gemm(transa: bool, transb: bool, A: CM, B: CM, alpha: float = 1.0, beta: float = 0.0,
         C: CM | None = None) -> CM:
    """C = alpha op(A) op(B) + beta C on MFMA (split-K for long inner dimensions).  A or B may
    be float32 (gp_gemm_ex widens them on load: the same fp64 result as on an fp64 copy); C is
    fp64."""
    m = A.cols if transa else A.rows
    k = A.rows if transa else A.cols
    kb = B.cols if transb else B.rows
    n = B.rows if transb else B.cols
    if k != kb:
        raise ValueError(f"gemm: inner dimensions differ ({k} vs {kb})")
    dev = A.t.device
    if C is None:
        C = CM.empty(m, n, dev)
        beta = 0.0
    lib = _capi.lib()
    nbytes = lib.gp_dgemm_ws_bytes(m, n, k)
    ws = _ws(nbytes, dev)
    for nm, M in (("A", A), ("B", B)):
        if M.t.dtype not in (torch.float32, F64):
            raise TypeError(f"gemm: {nm} must be float32 or float64, got {M.t.dtype}")
    if C.t.dtype != F64:
        raise TypeError("gemm: C must be float64")
    _capi.call("gp_gemm_ex", int(transa), int(transb), m, n, k, float(alpha), A.ptr(),
               int(A.f32), A.ld, B.ptr(), int(B.f32), B.ld, float(beta), C.ptr(), C.ld,
               ws.data_ptr() if ws is not None else None, nbytes if ws is not None else 0,
               _stream(dev))
    return C


def sim_stats(Y: torch.Tensor, sd_floor: float = 1e-6):
    """mu, sd(ddof=1, floored) over rows of a C-order (n x ny) ensemble (src/model.py:60-64)."""
    Y = Y.contiguous()
    n, ny = Y.shape
    mu = torch.empty(ny, dtype=F64, device=Y.device)
    sd = torch.empty(ny, dtype=F64, device=Y.device)
    _capi.call("gp_sim_stats", Y.data_ptr(), n, ny, ny, float(sd_floor), mu.data_ptr(),
               sd.data_ptr(), _stream(Y.device))
    return mu, sd


def standardize(Y: torch.Tensor, mu: torch.Tensor, sd: torch.Tensor, inverse: bool = False,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """(Y - mu)/sd, or Y sd + mu when ``inverse`` (C-order rows x ny)."""
    Y = Y.contiguous()
    n, ny = Y.shape
    out = torch.empty_like(Y) if out is None else out
    _capi.call("gp_standardize", Y.data_ptr(), n, ny, ny, mu.data_ptr(), sd.data_ptr(),
               out.data_ptr(), out.stride(0), int(inverse), _stream(Y.device))
    return out


def field_max_pcs() -> int:
    return int(_capi.lib().gp_field_max_pcs())


def field(W: torch.Tensor, K: torch.Tensor, sd: torch.Tensor | None = None,
          mu: torch.Tensor | None = None, err: torch.Tensor | None = None, f32: bool = False,
          out: torch.Tensor | None = None) -> torch.Tensor:
    """Y = (W K + err) sd + mu in one pass (gp_field; SepiaEmulatorPrediction.get_y):
    W (rows x P) and K (P x ncols, row stride free) row-major fp64 on the device, sd / mu
    (ncols) or both None (standardised field), err (rows) or None; Y (rows x ncols) float32 when
    ``f32`` else float64."""
    rows, P = W.shape
    # (a dimension of one element has no stride to check: the reference's scalar models, P = ny = 1)
    if K.shape[0] != P or (K.shape[1] > 1 and K.stride(1) != 1) or (P > 1 and W.stride(1) != 1):
        raise ValueError("field: W (rows x P) and K (P x ncols) must be row-major, K.shape[0] = P")
    ncols = K.shape[1]
    if out is None:
        out = torch.empty((rows, ncols), dtype=torch.float32 if f32 else F64, device=W.device)
    if (sd is None) != (mu is None):
        raise ValueError("field: sd and mu go together")
    for t in (sd, mu, err):
        if t is not None and (t.dtype != F64 or not t.is_contiguous()):
            raise ValueError("field: sd / mu / err must be contiguous float64")
    if err is not None and err.numel() != rows:
        raise ValueError(f"field: err has {err.numel()} values for {rows} rows")
    _capi.call("gp_field", W.data_ptr(), W.stride(0), rows, P, K.data_ptr(), K.stride(0), ncols,
               sd.data_ptr() if sd is not None else None,
               mu.data_ptr() if mu is not None else None,
               err.data_ptr() if err is not None else None, out.data_ptr(), out.stride(0),
               int(f32), _stream(W.device))
    return out


def field_summary_max_tail() -> int:
    return int(_capi.lib().gp_field_summary_max_tail())


def summary_tail_depths(S: int, q_lo: float, q_hi: float):
    """Order statistics gp_field_summary keeps per tail for (S, q_lo, q_hi): the lower one reads
    z_(j), z_(j+1) at j = floor(q_lo (S-1)), the upper one the same two counted from the top."""
    jl = int(np.floor(q_lo * (S - 1)))
    jh = int(np.floor(q_hi * (S - 1)))
    return min(jl + 2, S), S - jh


def _band(q):
    """q -> (q_lo, q_hi): a float is the band [q, 1 - q]."""
    if np.ndim(q) == 0:
        return float(q), 1.0 - float(q)
    q_lo, q_hi = q
    return float(q_lo), float(q_hi)


def _summary_operands(fn, W3, K, sd, mu, err, q):
    """The operand checks field_summary and field_score share -> (S, m, P, ncols, ldw, lds, ldk,
    q_lo, q_hi); every refusal is a ValueError that names ``fn``."""
    for nm, t, nd in (("W3", W3, 3), ("K", K, 2)):
        if not torch.is_tensor(t) or t.dtype != F64 or t.dim() != nd:
            raise ValueError(f"{fn}: {nm} must be a {nd}-d float64 tensor")
    S, m, P = W3.shape
    dev = W3.device
    if K.device != dev:
        raise ValueError(f"{fn}: W3 and K must be on one device")
    if S < 1 or P < 1 or K.shape[0] != P:
        raise ValueError(f"{fn}: W3 {tuple(W3.shape)} needs S >= 1 samples and K "
                         f"{tuple(K.shape)} one row per PC")
    ncols = K.shape[1]
    ldw = W3.stride(1) if m > 1 else max(W3.stride(1), P)
    lds = W3.stride(0) if S > 1 else max(W3.stride(0), (m - 1) * ldw + P)
    if (P > 1 and W3.stride(2) != 1) or ldw < P or lds < (max(m, 1) - 1) * ldw + P:
        raise ValueError(f"{fn}: W3 needs a unit last stride and sample-major strides "
                         f"(lds >= (m - 1) ldw + P, ldw >= P), got {W3.stride()}")
    ldk = K.stride(0) if P > 1 else max(K.stride(0), ncols, 1)
    if (ncols > 1 and K.stride(1) != 1) or ldk < max(ncols, 1):
        raise ValueError(f"{fn}: K must be row-major (strides {K.stride()})")
    if (sd is None) != (mu is None):
        raise ValueError(f"{fn}: sd and mu go together")
    for nm, t, n in (("sd", sd, ncols), ("mu", mu, ncols), ("err", err, S * m)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != F64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{fn}: {nm} must be contiguous float64 on W3's device")
        if t.numel() != n:
            raise ValueError(f"{fn}: {nm} has {t.numel()} values, expected {n}")
    q_lo, q_hi = _band(q)
    if not (0.0 <= q_lo <= q_hi <= 1.0):
        raise ValueError(f"{fn}: need 0 <= q_lo <= q_hi <= 1, got ({q_lo}, {q_hi})")
    return S, m, P, ncols, ldw, lds, ldk, q_lo, q_hi


def _summary_outs(fn, out, m, ncols, dt, dev):
    """The (mean, lo, hi) output checks the two share -> their common row stride ldo."""
    if len(out) != 3:
        raise ValueError(f"{fn}: out is (mean, lo, hi)")
    ldo = max(ncols, 1)
    for t in out:
        if not torch.is_tensor(t) or t.dtype != dt or t.device != dev or \
                tuple(t.shape) != (m, ncols):
            raise ValueError(f"{fn}: out tensors must be {dt} of shape {(m, ncols)} on "
                             "W3's device")
        if ncols > 1 and t.stride(1) != 1:
            raise ValueError(f"{fn}: out tensors need a unit column stride")
        if m > 1:
            ldo = max(ldo, t.stride(0))
    for t in out:
        if m > 1 and t.stride(0) != ldo:
            raise ValueError(f"{fn}: out tensors must share one row stride >= ncols")
    return ldo


def _ptr(t):
    return t.data_ptr() if t is not None else None


def field_summary(W3: torch.Tensor, K: torch.Tensor, sd: torch.Tensor | None = None,
                  mu: torch.Tensor | None = None, err: torch.Tensor | None = None, q=0.025,
                  f32: bool = False, out=None):
    """(mean, lo, hi) over the S samples of the field (W3 K + err) sd + mu in one pass
    (gp_field_summary; np.mean(get_y(), 0) and np.quantile(get_y() + error, [q, 1 - q], 0) without
    the (S, m, ncols) field): W3 (S, m, P) fp64 with unit last stride (its two leading strides are
    passed through), K (P x ncols, row stride free), sd / mu (ncols) or both None, err (S m values,
    sample-major) or None; ``q`` a float (band [q, 1 - q]) or a pair (q_lo, q_hi).  Each result is
    (m, ncols), float32 when ``f32`` else float64; ``out`` = three such tensors (unit column
    stride, one common row stride) to write into."""
    fn = "field_summary"
    S, m, P, ncols, ldw, lds, ldk, q_lo, q_hi = _summary_operands(fn, W3, K, sd, mu, err, q)
    dev = W3.device
    dt = torch.float32 if f32 else F64
    if out is None:
        out = tuple(torch.empty((m, ncols), dtype=dt, device=dev) for _ in range(3))
    ldo = _summary_outs(fn, out, m, ncols, dt, dev)
    mean, lo, hi = out
    if dev.type != "cuda":
        raise ValueError("field_summary: the operands must be on a HIP device")
    if m == 0 or ncols == 0:
        return mean, lo, hi
    _capi.call("gp_field_summary", W3.data_ptr(), ldw, lds, S, m, P, K.data_ptr(), ldk, ncols,
               _ptr(sd), _ptr(mu), _ptr(err), q_lo, q_hi, mean.data_ptr(),
               lo.data_ptr(), hi.data_ptr(), ldo, int(f32), _stream(dev))
    return mean, lo, hi


def field_score_ws_bytes(S: int, m: int, P: int, ncols: int) -> int:
    return int(_capi.lib().gp_field_score_ws_bytes(S, m, P, ncols))


def field_score(W3: torch.Tensor, K: torch.Tensor, sd: torch.Tensor | None = None,
                mu: torch.Tensor | None = None, err: torch.Tensor | None = None,
                Y: torch.Tensor | None = None, q=0.025, mape_floor: float = -np.inf,
                f32: bool = False, out=None, cols: bool = True):
    """Test-error sums of field_summary's (mean, lo, hi) against the truth ``Y`` in the same one
    pass, without the three arrays (gp_field_score): returns ``(rows, cols)``, fp64 device tensors
    (m, 8) and (ncols, 4) in the order of _capi.SCORE_ROW / SCORE_COL (``cols=False``: None), and
    ``(rows, cols, mean, lo, hi)`` when ``out`` = the three tensors field_summary would fill is
    given (they receive the same bits).  W3, K, sd, mu, err, q, f32 as in field_summary; ``Y``
    (m, ncols) float32 or float64 on the device with a unit column stride, NaN where there is no
    truth, or None (no truth at all); absolute percentage errors are counted where
    ``not (y < mape_floor)``."""
    fn = "field_score"
    S, m, P, ncols, ldw, lds, ldk, q_lo, q_hi = _summary_operands(fn, W3, K, sd, mu, err, q)
    dev = W3.device
    ldy = max(ncols, 1)
    if Y is not None:
        if not torch.is_tensor(Y) or Y.dtype not in (torch.float32, F64) or Y.device != dev or \
                tuple(Y.shape) != (m, ncols):
            raise ValueError(f"{fn}: Y must be float32 or float64 of shape {(m, ncols)} on W3's "
                             "device")
        if ncols > 1 and Y.stride(1) != 1:
            raise ValueError(f"{fn}: Y needs a unit column stride")
        if m > 1:
            ldy = Y.stride(0)
        if ldy < max(ncols, 1):
            raise ValueError(f"{fn}: Y needs a row stride >= ncols (strides {Y.stride()})")
    try:
        mape_floor = float(mape_floor)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: mape_floor must be a number") from None
    dt = torch.float32 if f32 else F64
    ldo = max(ncols, 1)
    if out is not None:
        ldo = _summary_outs(fn, out, m, ncols, dt, dev)
    if dev.type != "cuda":
        raise ValueError(f"{fn}: the operands must be on a HIP device")
    rows = torch.empty((m, 8), dtype=F64, device=dev)
    colt = torch.empty((ncols, 4), dtype=F64, device=dev) if cols else None
    res = (rows, colt) if out is None else (rows, colt) + tuple(out)
    if m == 0 or ncols == 0:                       # sums of nothing
        rows.zero_()
        if colt is not None:
            colt.zero_()
        return res
    nbytes = field_score_ws_bytes(S, m, P, ncols)
    ws = _ws(nbytes, dev)
    mean, lo, hi = out if out is not None else (None, None, None)
    _capi.call("gp_field_score", W3.data_ptr(), ldw, lds, S, m, P, K.data_ptr(), ldk, ncols,
               _ptr(sd), _ptr(mu), _ptr(err), q_lo, q_hi, _ptr(Y), ldy,
               int(Y is not None and Y.dtype == torch.float32), mape_floor, _ptr(mean), _ptr(lo),
               _ptr(hi), ldo, int(f32), rows.data_ptr(), _ptr(colt), ws.data_ptr(), nbytes,
               _stream(dev))
    return res


def pca_trunc_limits():
    """(largest rank, most levels per call) of gp_pca_trunc."""
    lib = _capi.lib()
    return int(lib.gp_pca_trunc_max_rank()), int(lib.gp_pca_trunc_max_levels())


def _row_stride(fn, nm, t, rows, cols):
    """Row stride of a 2-d operand with a unit column stride; a single row has none to check."""
    if cols > 1 and t.stride(1) != 1:
        raise ValueError(f"{fn}: {nm} needs a unit column stride (strides {t.stride()})")
    ld = t.stride(0) if rows > 1 else max(t.stride(0), cols, 1)
    if ld < max(cols, 1):
        raise ValueError(f"{fn}: {nm} needs a row stride >= its {cols} columns "
                         f"(strides {t.stride()})")
    return ld


def pca_trunc(Y: torch.Tensor, C: torch.Tensor, V: torch.Tensor, ranks, mu=None, sd=None,
              node: bool = False, out=None):
    """Residual sums of the PCA truncation at every rank of ``ranks`` in one pass over the
    ensemble (gp_pca_trunc): with e_r = (Y - mu) - sd (C[:, :ranks[r]] V[:ranks[r]]),
    ``tot[r] = (sum e_r^2, sum e_r)`` and, when ``node``, ``node[r, j] = sum_i e_r[i, j]^2``.
    Y (n, ncols) float32 or float64, C (n, p) = U diag(S) and V (p, ncols) float64, all on one HIP
    device, row-major with free row strides; mu / sd (ncols) contiguous float64 or both None (0
    and 1); ``ranks`` strictly increasing host integers within [0, min(p, the kernel's largest
    rank)] (lists longer than the kernel's level limit are split over several calls: a level's
    sums do not depend on the other levels).  Returns ``(tot, node_or_None)``, float64 device
    tensors (R, 2) and (R, ncols); ``out`` = such a pair (node None when not requested, unit
    column stride) to write into."""
    fn = "pca_trunc"
    for nm, t, dts in (("Y", Y, (torch.float32, F64)), ("C", C, (F64,)), ("V", V, (F64,))):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype not in dts:
            raise ValueError(f"{fn}: {nm} must be a 2-d " +
                             " or ".join(str(d).replace("torch.", "") for d in dts) + " tensor")
    n, ncols = Y.shape
    p = C.shape[1]
    dev = Y.device
    if C.device != dev or V.device != dev:
        raise ValueError(f"{fn}: Y, C and V must be on one device")
    if p < 1 or C.shape[0] != n or tuple(V.shape) != (p, ncols):
        raise ValueError(f"{fn}: Y {tuple(Y.shape)} needs C (n x p) and V (p x ncols), got "
                         f"C {tuple(C.shape)}, V {tuple(V.shape)}")
    ldy = _row_stride(fn, "Y", Y, n, ncols)
    ldc = _row_stride(fn, "C", C, n, p)
    ldv = _row_stride(fn, "V", V, p, ncols)
    if (mu is None) != (sd is None):
        raise ValueError(f"{fn}: mu and sd go together")
    for nm, t in (("mu", mu), ("sd", sd)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != F64 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{fn}: {nm} must be contiguous float64 on Y's device")
        if t.numel() != ncols:
            raise ValueError(f"{fn}: {nm} has {t.numel()} values, expected {ncols}")
    try:
        rk = [int(r) for r in np.asarray(ranks).reshape(-1)]
        exact = bool(np.all(np.asarray(ranks).reshape(-1) == np.asarray(rk)))
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: ranks must be integers") from None
    max_rank, max_lev = pca_trunc_limits()
    if not exact or not rk or rk[0] < 0 or any(b <= a for a, b in zip(rk, rk[1:])):
        raise ValueError(f"{fn}: ranks must be a non-empty strictly increasing list of "
                         f"integers >= 0, got {list(np.asarray(ranks).reshape(-1))}")
    if rk[-1] > min(p, max_rank):
        raise ValueError(f"{fn}: rank {rk[-1]} is above the {p} columns of C or the kernel's "
                         f"limit {max_rank}")
    R = len(rk)
    if out is None:
        tot = torch.empty((R, 2), dtype=F64, device=dev)
        nod = torch.empty((R, ncols), dtype=F64, device=dev) if node else None
    else:
        if len(out) != 2:
            raise ValueError(f"{fn}: out is (tot, node)")
        tot, nod = out
        if not torch.is_tensor(tot) or tot.dtype != F64 or tot.device != dev or \
                tuple(tot.shape) != (R, 2) or not tot.is_contiguous():
            raise ValueError(f"{fn}: out[0] (tot) must be contiguous float64 of shape {(R, 2)} on "
                             "Y's device")
        if node != (nod is not None):
            raise ValueError(f"{fn}: out[1] (node) is given exactly when node=True")
        if nod is not None and (not torch.is_tensor(nod) or nod.dtype != F64 or
                                nod.device != dev or tuple(nod.shape) != (R, ncols)):
            raise ValueError(f"{fn}: out[1] (node) must be float64 of shape {(R, ncols)} on Y's "
                             "device")
    ldn = _row_stride(fn, "node", nod, R, ncols) if nod is not None else max(ncols, 1)
    if dev.type != "cuda":
        raise ValueError(f"{fn}: the operands must be on a HIP device")
    if n == 0 or ncols == 0:                       # sums of nothing
        tot.zero_()
        if nod is not None:
            nod.zero_()
        return tot, nod
    lib = _capi.lib()
    for lo in range(0, R, max_lev):
        part = rk[lo:lo + max_lev]
        arr = (ctypes.c_int * len(part))(*part)
        nbytes = int(lib.gp_pca_trunc_ws_bytes(n, ncols, len(part)))
        ws = _ws(nbytes, dev)
        _capi.call("gp_pca_trunc", Y.data_ptr(), ldy, int(Y.dtype == torch.float32), n, ncols,
                   _ptr(mu), _ptr(sd), C.data_ptr(), ldc, V.data_ptr(), ldv,
                   ctypes.addressof(arr), len(part), tot[lo:].data_ptr(),
                   nod[lo:].data_ptr() if nod is not None else None, ldn, ws.data_ptr(), nbytes,
                   _stream(dev))
    return tot, nod


def mean_var(x: torch.Tensor, ddof: int = 0):
    """(mean, var) of all elements of ``x`` (device scalars tensor of 2)."""
    x = x.contiguous()
    out = torch.empty(2, dtype=F64, device=x.device)
    work = torch.empty(1024, dtype=F64, device=x.device)
    _capi.call("gp_mean_var", x.data_ptr(), x.numel(), int(ddof), out.data_ptr(),
               work.data_ptr(), _stream(x.device))
    return out


def shift_diag(G: CM, factor: float) -> None:
    _capi.call("gp_shift_diag", G.ptr(), G.rows, G.ld, float(factor), _stream(G.t.device))


def rowscale(M: CM, f: torch.Tensor, inverse: bool = False) -> None:
    _capi.call("gp_rowscale", M.ptr(), M.rows, M.cols, M.ld, f.data_ptr(), int(inverse),
               _stream(M.t.device))


def syevj(A: CM, max_sweeps: int = 30, tol: float = 1e-15, want_sqrt: bool = False):
    """Eigen-decomposition of a symmetric r x r matrix (destroyed): (W desc, V, sweeps)."""
    r = A.rows
    dev = A.t.device
    W = torch.empty(r, dtype=F64, device=dev)
    V = CM.empty(r, r, dev)
    sweeps = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.call("gp_syevj", A.ptr(), r, A.ld, W.data_ptr(), V.ptr(), V.ld, int(max_sweeps),
               float(tol), sweeps.data_ptr(), int(want_sqrt), _stream(dev))
    return W, V, sweeps
