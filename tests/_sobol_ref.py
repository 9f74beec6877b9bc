"""numpy restatement of gp_sobol_replicates (include/gpfit.h) for the tests, written from the
header's formulas, with the per-element rounding bound the GPU tests compare under.

Operands are output-major like the kernel's: fA / fB (p, N), fAB (d, p, N); ``rows`` (R, M) are
the design rows of every replicate.  Not a fixture module: imported by name.
"""
import numpy as np

from oracle import rng_ref

EPS = np.finfo(np.float64).eps


def philox_rows(N, n_draw, R, seed, offset=0):
    """Rows GPFIT_SOBOL_PHILOX selects: key seed, counter (k >> 2, r, offset_lo, offset_hi),
    word k & 3 -> x, row (x N) >> 32."""
    Q = (n_draw + 3) // 4
    q = np.tile(np.arange(Q, dtype=np.uint32), R)
    r = np.repeat(np.arange(R, dtype=np.uint32), Q)
    ctr = np.stack([q, r, np.full(R * Q, offset & 0xFFFFFFFF, dtype=np.uint32),
                    np.full(R * Q, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint32)], axis=1)
    x = rng_ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    x = x.reshape(R, Q * 4)[:, :n_draw].astype(np.uint64)
    return ((x * np.uint64(N)) >> np.uint64(32)).astype(np.int32)


def jackknife_rows(N):
    k = np.arange(N - 1)[None, :]
    r = np.arange(N)[:, None]
    return (k + (k >= r)).astype(np.int32)


def replicates(fA, fB, fAB, rows, pcvar=None, clamp=False):
    """dict: first / total (R, p, d), gfirst / gtotal (R, d) or None, and the bounds b_first,
    b_total, b_gfirst, b_gtotal on |kernel - this| from the plain summation bound
    |fl(sum t) - sum t| <= (M + 8) eps sum |t| (factor 4: this restatement's own rounding, the
    variance and the division)."""
    fA, fB, fAB = (np.asarray(x, dtype=np.float64) for x in (fA, fB, fAB))
    rows = np.clip(np.asarray(rows), 0, fA.shape[1] - 1)
    R, M = rows.shape
    a = fA[:, rows]                                   # (p, R, M)
    b = fB[:, rows]
    c = fAB[:, :, rows]                               # (d, p, R, M)
    mu = (a.sum(-1) + b.sum(-1)) / (2 * M)
    var = (((a - mu[..., None]) ** 2).sum(-1) + ((b - mu[..., None]) ** 2).sum(-1)) / (2 * M)
    terms = a[None] * (c - b[None])
    V = terms.sum(-1) / M                             # (d, p, R)
    absV = np.abs(terms).sum(-1) / M
    E = ((b[None] - c) ** 2).sum(-1) / (2 * M)
    if clamp:
        V = np.where(V < 0, 0.0, V)
    first = np.transpose(V / var[None], (2, 1, 0))    # (R, p, d)
    total = np.transpose(E / var[None], (2, 1, 0))
    f = 4 * (M + 8) * EPS
    out = {"first": first, "total": total,
           "b_first": f * (np.transpose(absV / var[None], (2, 1, 0)) + np.abs(first)),
           "b_total": f * np.abs(total),
           "gfirst": None, "gtotal": None, "b_gfirst": None, "b_gtotal": None}
    if pcvar is not None:
        w = np.asarray(pcvar, dtype=np.float64)[None, :, None]
        gf = np.zeros((R, first.shape[2]))
        gt = np.zeros_like(gf)
        for j in range(first.shape[1]):               # increasing j
            gf += w[:, j] * first[:, j]
            gt += w[:, j] * total[:, j]
        out.update(gfirst=gf, gtotal=gt, b_gfirst=(np.abs(w) * out["b_first"]).sum(1),
                   b_gtotal=(np.abs(w) * out["b_total"]).sum(1))
    return out


def to_output_major(fA, fB, fAB):
    """The reference's (N, p), (N, p), (d, N, p) -> the kernel's (p, N), (p, N), (d, p, N)."""
    return (np.ascontiguousarray(np.asarray(fA).T), np.ascontiguousarray(np.asarray(fB).T),
            np.ascontiguousarray(np.transpose(np.asarray(fAB), (0, 2, 1))))
