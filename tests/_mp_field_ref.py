"""The field back end at 50 digits (mpmath), its regimes, and the fp64 noise level per regime.

TEST INFRASTRUCTURE ONLY: plain Python / numpy / mpmath, no GPU.  The companion of
tests/_mp_ref.py (the GP chain) and tests/_mp_pca_ref.py (the PCA front end) for everything
downstream of the PC weights: gp_field, gp_field_summary, gp_field_score and gp_pca_trunc, as
include/gpfit.h defines them.

* Truth (``mp.dps = 50``, the inputs taken as the exact binary values of the fp64 / float32
  arrays): ``field_truth`` (a = sum_k W K by mp.fdot, which adds the exact products and rounds
  once; y = a sd + mu, z = (a + err) sd + mu), ``round_f32`` (one rounding to float32, to nearest
  even, +-inf beyond FLT_MAX, subnormals included), ``summary_truth`` (the mean of y_s; lo / hi
  from the sorted z_s with the position (j, t) of ``position`` -- pos = fl(q (S - 1)) in fp64,
  part of the definition -- and the interpolation itself in mpmath), ``score_truth`` (the eight
  row sums and four column sums from the truth's mean / lo / hi rounded to the output dtype and
  widened again) and ``trunc_truth`` (one pass over k, a snapshot at every rank).  Results are
  ``_mp_ref.DD`` pairs.
* Regimes: ``FIELD_REGIMES`` for field / summary / score, ``TRUNC_REGIMES`` for gp_pca_trunc;
  ``FIELD_CASES``, ``SUMMARY_CASES``, ``SCORE_CASES`` and ``TRUNC_CASES`` are the shapes, the
  smallest that cross every structural edge of the kernels.
* Noise: the largest error against the truth over fp64 restatements built from numpy alone
  (W @ K, the strictly k-ordered chain, NPERM seeded permutations of the PC order; for means and
  sums NPERM permutations of the summed index; for gp_pca_trunc the same over k and over rows),
  never below 4 eps of the quantity's scale.  Order statistics are 1-Lipschitz in the sup norm,
  so a quantile's noise is the noise of z plus 3 eps |z| for the three roundings of the
  interpolation: no near-tie makes it discontinuous and nothing is excluded.  A test asks
  ``error <= MARGIN * noise``.
* ``FINDINGS``: the (quantity, regime) pairs at which the device was measured above that and the
  cause is the library's documented arithmetic; they carry ``one_pass_var_term``, derived there.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from mpmath import mp, mpf

import _pca_ref
import _score_ref
from _mp_ref import DD, EPS, MARGIN

DPS = 50
NPERM = 8
U = EPS / 2.0                                   # the unit roundoff 2^-53
FLT_MAX = float(np.finfo(np.float32).max)
F32_MIN_EXP = -126                              # exponent of the smallest normal float32

FIELD_REGIMES = ("mid", "graded", "cancel", "offset", "f32edge", "ties")
TRUNC_REGIMES = ("mid", "exact", "graded", "offset32", "biased")
CANCEL = 1e10                                   # the cancel regime's sum|w K| / |a|
BIAS = 1e4                                      # the biased regime's delta / residual spread
TRUNC_NOISE = 1e-3                              # _pca_ref.ensemble's residual spread


# ---------------------------------------------------------------------------- mpmath helpers
def _mat(a):
    return [[mpf(v) for v in row] for row in np.asarray(a, dtype=np.float64).tolist()]


def _vec(a):
    return [mpf(v) for v in np.asarray(a, dtype=np.float64).reshape(-1).tolist()]


def _tr(A):
    return [list(c) for c in zip(*A)]


def _dd(rows):
    rows = [list(r) for r in rows]
    return DD((v for r in rows for v in r), (len(rows), len(rows[0]) if rows else 0))


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def round_f32(v) -> float:
    """The mpf ``v`` rounded once to float32, to nearest even, as a Python float: +-inf from
    FLT_MAX + half an ulp on, subnormals on the 2^-149 grid."""
    if v == 0:
        return 0.0
    x = abs(v)
    e = mp.frexp(x)[1] - 1                       # x = f 2^e, 1 <= f < 2
    q = max(int(e), F32_MIN_EXP) - 23            # exponent of the ulp
    n = int(mp.nint(mp.ldexp(x, -q)))            # half to even
    r = math.ldexp(n, q)                         # exact: n <= 2^24
    if r > FLT_MAX:
        r = math.inf
    return -r if v < 0 else r


def ulp_f32(x):
    """The float32 ulp at the magnitude of the fp64 array ``x`` (of its own binade; 2^-149 below
    the normal range)."""
    e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))[1] - 1
    return np.ldexp(1.0, np.maximum(e, F32_MIN_EXP) - 23)


def all_normal(*arrays) -> bool:
    """Every non-zero value of every array is finite and in fp64's normal range."""
    for a in arrays:
        x = np.abs(np.asarray(a, dtype=np.float64))
        x = x[x != 0]
        if x.size and not (np.all(np.isfinite(x)) and x.min() >= 2.0 ** -1022):
            return False
    return True


# ------------------------------------------------------------------------------------- truth
class FieldTruth:
    """y and z as rows of mpf (``ym``, ``zm``: rows x ncols) and as DD (``y``, ``z``)."""


def products(W, K):
    """a = W K as rows of mpf: mp.fdot adds the exact products and rounds once to 50 digits."""
    W, K = np.asarray(W, dtype=np.float64), np.asarray(K, dtype=np.float64)
    with mp.workdps(DPS):
        Kt = _tr(_mat(K)) if K.shape[1] else []
        return [[mp.fdot(w, k) for k in Kt] for w in _mat(W)]


def field_truth(W, K, sd=None, mu=None, err=None, a=None) -> FieldTruth:
    """``a``: products(W, K) when the caller has them already."""
    with mp.workdps(DPS):
        a = products(W, K) if a is None else a
        s = _vec(sd) if sd is not None else None
        m = _vec(mu) if mu is not None else None
        e = _vec(err) if err is not None else None
        t = FieldTruth()
        if s is None:
            t.ym = a
            t.zm = a if e is None else [[v + e[r] for v in row] for r, row in enumerate(a)]
        else:
            t.ym = [[v * s[c] + m[c] for c, v in enumerate(row)] for row in a]
            t.zm = t.ym if e is None else \
                [[(v + e[r]) * s[c] + m[c] for c, v in enumerate(row)] for r, row in enumerate(a)]
        t.y = _dd(t.ym)
        t.z = t.y if t.zm is t.ym else _dd(t.zm)
        return t


def f32_of(rows):
    """Rows of mpf -> the float32 expectation, as an fp64 array holding float32 values."""
    with mp.workdps(DPS):
        return np.array([[round_f32(v) for v in r] for r in rows], dtype=np.float64).reshape(
            len(rows), len(rows[0]) if rows else 0)


def position(q: float, S: int):
    """(j, t) of the header's rule, in fp64: pos = fl(q (S - 1)), j = floor(pos), t = pos - j."""
    pos = float(q) * float(S - 1)
    j = math.floor(pos)
    return int(j), pos - j


def band(q):
    return (float(q), 1.0 - float(q)) if np.ndim(q) == 0 else (float(q[0]), float(q[1]))


def tail_depths(S, q):
    """Order statistics gp_field_summary keeps per tail (include/gpfit.h)."""
    q_lo, q_hi = band(q)
    return min(position(q_lo, S)[0] + 2, S), S - position(q_hi, S)[0]


def list_depth(S, q):
    """The instantiated list depth 2 / 4 / 8 that holds the request (None: refused)."""
    d = max(tail_depths(S, q))
    return next((k for k in (2, 4, 8) if d <= k), None)


class SummaryTruth:
    """mean, lo, hi as DD (m, ncols) and as rows of mpf (``mean_m`` ...); ``src_lo`` / ``src_hi``
    (m, ncols) the sample whose z is z_(j); ``tied_lo`` / ``tied_hi`` where z_(j) = z_(j+1)
    exactly (or j = S - 1), so the quantile is that sample's value itself."""


def _quantile(zs, q):
    """(value, sample of z_(j), tied) from [(z_s, s)] sorted."""
    S = len(zs)
    j, t = position(q, S)
    if j >= S - 1:
        return zs[S - 1][0], zs[S - 1][1], True
    a, b = zs[j][0], zs[j + 1][0]
    return a + (b - a) * mpf(t), zs[j][1], a == b


def summary_truth(ft: FieldTruth, S, m, q) -> SummaryTruth:
    q_lo, q_hi = band(q)
    ncols = len(ft.ym[0])
    with mp.workdps(DPS):
        t = SummaryTruth()
        t.mean_m = [[mp.fsum(ft.ym[s * m + i][c] for s in range(S)) / S for c in range(ncols)]
                    for i in range(m)]
        t.lo_m, t.hi_m = [], []
        src = np.zeros((2, m, ncols), dtype=np.int64)
        tied = np.zeros((2, m, ncols), dtype=bool)
        for i in range(m):
            lo_r, hi_r = [], []
            for c in range(ncols):
                zs = sorted(((ft.zm[s * m + i][c], s) for s in range(S)), key=lambda p: p[0])
                for k, (qq, out) in enumerate(((q_lo, lo_r), (q_hi, hi_r))):
                    v, src[k, i, c], tied[k, i, c] = _quantile(zs, qq)
                    out.append(v)
            t.lo_m.append(lo_r)
            t.hi_m.append(hi_r)
        t.mean, t.lo, t.hi = _dd(t.mean_m), _dd(t.lo_m), _dd(t.hi_m)
        t.src_lo, t.src_hi = src
        t.tied_lo, t.tied_hi = tied
        return t


def _stored(rows, f32):
    """The truth rounded to the output dtype and widened again (rows of mpf)."""
    return [[mpf(round_f32(v) if f32 else float(v)) for v in r] for r in rows]


def score_truth(st: SummaryTruth, f32, Y, floor):
    """(rows (m, 8) DD, cols (ncols, 4) DD, rabs, cabs): gp_field_score's sums in mpmath on the
    stored truth; ``rabs`` / ``cabs`` the sums of the terms' magnitudes (fp64, zero in the count
    columns).  Y: (m, ncols) float32 / float64 with NaN = no truth, or None."""
    R, C = _score_ref.ROW, _score_ref.COL
    with mp.workdps(DPS):
        mu, lo, hi = (_stored(a, f32) for a in (st.mean_m, st.lo_m, st.hi_m))
        m, n = len(mu), len(mu[0])
        rows = [[mpf(0)] * 8 for _ in range(m)]
        cols = [[mpf(0)] * 4 for _ in range(n)]
        rabs, cabs = np.zeros((m, 8)), np.zeros((n, 4))
        y = None if Y is None else np.asarray(Y).astype(np.float64)
        for i in range(m):
            for c in range(n):
                for k, v in ((R["lo"], lo[i][c]), (R["hi"], hi[i][c]), (R["mean"], mu[i][c])):
                    rows[i][k] += v
                    rabs[i, k] += abs(float(v))
                w = hi[i][c] - lo[i][c]
                cols[c][C["width"]] += w
                cabs[c, C["width"]] += abs(float(w))
                if y is None or np.isnan(y[i, c]):
                    continue
                yv = mpf(float(y[i, c]))
                sq = (mu[i][c] - yv) ** 2
                rows[i][R["sqerr"]] += sq
                cols[c][C["sqerr"]] += sq
                rabs[i, R["sqerr"]] += float(sq)
                cabs[c, C["sqerr"]] += float(sq)
                rows[i][R["valid"]] += 1
                cols[c][C["valid"]] += 1
                if not (y[i, c] < floor):
                    ape = abs((mu[i][c] - yv) / yv)
                    rows[i][R["ape"]] += ape
                    rabs[i, R["ape"]] += float(ape)
                    rows[i][R["ape_n"]] += 1
                if lo[i][c] <= yv <= hi[i][c]:
                    rows[i][R["covered"]] += 1
                    cols[c][C["covered"]] += 1
        return _dd(rows), _dd(cols), rabs, cabs


class TruncTruth:
    """tot (R, 2), node (R, ncols), rmse (R,), var (R,) as DD; ``A`` = mean(e^2), ``B`` = mean(e)
    and ``abs1`` = sum |e| per level in fp64 (scales)."""


def trunc_truth(Y, C, V, ranks, mu=None, sd=None) -> TruncTruth:
    """One pass over k, snapshotting at each rank.  Y float32 or float64 (widened exactly)."""
    Y = np.asarray(Y).astype(np.float64)
    n, ncols = Y.shape
    ranks = [int(r) for r in ranks]
    with mp.workdps(DPS):
        Ym, Cm, Vt = _mat(Y), _mat(C), _tr(_mat(V))
        m = _vec(mu) if mu is not None else [mpf(0)] * ncols
        s = _vec(sd) if sd is not None else [mpf(1)] * ncols
        R = len(ranks)
        sq = [[[None] * ncols for _ in range(n)] for _ in range(R)]
        tot1, ab = [mpf(0)] * R, [mpf(0)] * R
        for i in range(n):
            for j in range(ncols):
                e0, d, k0 = Ym[i][j] - m[j], mpf(0), 0
                for r, p in enumerate(ranks):
                    if p > k0:
                        d += mp.fdot(Cm[i][k0:p], Vt[j][k0:p])
                        k0 = p
                    e = e0 - s[j] * d
                    sq[r][i][j] = e * e
                    tot1[r] += e
                    ab[r] += abs(e)
        node = [[mp.fsum(sq[r][i][j] for i in range(n)) for j in range(ncols)] for r in range(R)]
        tot0 = [mp.fsum(node[r]) for r in range(R)]
        N = mpf(n) * ncols
        t = TruncTruth()
        t.tot = _dd([[tot0[r], tot1[r]] for r in range(R)])
        t.node = _dd(node)
        t.rmse = DD([mp.sqrt(tot0[r] / N) for r in range(R)])
        t.var = DD([tot0[r] / N - (tot1[r] / N) ** 2 for r in range(R)])
        t.A = np.array([float(tot0[r] / N) for r in range(R)])
        t.B = np.array([float(tot1[r] / N) for r in range(R)])
        t.abs1 = np.array([float(v) for v in ab])
        t.N = float(n) * float(ncols)
        return t


# ----------------------------------------------------------------------------------- regimes
def _seed(*key):
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key))


@functools.lru_cache(maxsize=None)
def field_operands(regime, rows, P, ncols):
    """(W (rows, P), K (P, ncols), sd, mu (ncols), err (rows)), read-only fp64.  A case passes sd /
    mu and err or leaves them out.

    mid      the existing tests' operands: N(0,1) W and K, sd in [0.5, 2], mu ~ 3 N, err ~ 0.3 N
    graded   row k of K scaled by 10^(-16 k / P)
    cancel   K = g c^T + 1e-10 N with W's rows orthogonal to g: sum|w_k K_k| / |a| ~ 1e10 per
             element (P >= 2; with one PC nothing can cancel and the operands are mid's)
    offset   mu ~ 1e6, sd = 1e-3: the samples' band is 1e-9 of its level
    f32edge  sd per column 1e38, 1e-38, 1e-42, 1e-45 and 1 in turn with mu = 0: values either side
             of FLT_MAX, of the smallest normal float32 and of the smallest subnormal
    ties     mid's operands; ``summary_operands`` repeats the samples in groups
    """
    rng = np.random.default_rng(_seed(regime, rows, P, ncols))
    W = rng.standard_normal((rows, P))
    K = rng.standard_normal((P, ncols))
    sd = rng.uniform(0.5, 2.0, ncols)
    mu = rng.standard_normal(ncols) * 3.0
    err = rng.standard_normal(rows) * 0.3
    if regime == "graded":
        K = K * (10.0 ** (-16.0 * np.arange(P) / P))[:, None]
    elif regime == "cancel" and P >= 2:
        g = rng.standard_normal(P)
        g /= np.linalg.norm(g)
        K = np.outer(g, rng.uniform(0.5, 2.0, ncols) * rng.choice([-1.0, 1.0], ncols)) + \
            K / CANCEL
        W = W - np.outer(W @ g, g)
        W = W - np.outer(W @ g, g)
        err = err / CANCEL
    elif regime == "offset":
        sd = np.full(ncols, 1e-3)
        mu = 1e6 + 1e3 * rng.standard_normal(ncols)
    elif regime == "f32edge":
        sd = np.array([1e38, 1e-38, 1e-42, 1e-45, 1.0])[np.arange(ncols) % 5]
        mu = np.zeros(ncols)
    elif regime not in FIELD_REGIMES:
        raise ValueError(regime)
    return _ro(W, K, sd, mu, err)


def tie_groups(S, kt):
    """[(first sample, size)]: sizes 1, 2, 3 and kt + 1 in turn until S samples are placed."""
    out, s, i = [], 0, 0
    sizes = (1, 2, 3, kt + 1)
    while s < S:
        g = min(sizes[i % 4], S - s)
        out.append((s, g))
        s, i = s + g, i + 1
    return out


@functools.lru_cache(maxsize=None)
def summary_operands(regime, S, m, P, ncols, q):
    """(W3 (S, m, P), K, sd, mu, err (S m, sample-major)).  ``ties``: whole samples repeated in
    groups of 1, 2, 3 and KT + 1 (KT the list depth of (S, q)) with equal error terms, so exact
    duplicates sit next to each other in the sample order -- in different rows of an MFMA tile,
    hence in the lanes that merge 16 and 32 apart -- and, in many columns, at the selected
    positions; the last group of two or more is all-zero rows of both signs."""
    W, K, sd, mu, err = field_operands(regime, S * m, P, ncols)
    W3 = W.reshape(S, m, P)
    if regime == "ties":
        W3, err2 = W3.copy(), err.reshape(S, m).copy()
        groups = tie_groups(S, list_depth(S, q) or 8)
        for s0, g in groups:
            W3[s0:s0 + g] = W3[s0]
            err2[s0:s0 + g] = err2[s0]
        zero = [gr for gr in groups if gr[1] >= 2]
        if zero:
            s0, g = zero[-1]
            sign = np.where(np.arange(g * m * P).reshape(g, m, P) % 2 == 0, 0.0, -0.0)
            W3[s0:s0 + g] = sign
            err2[s0:s0 + g] = np.where(np.arange(g * m).reshape(g, m) % 2 == 0, -0.0, 0.0)
        err = err2.reshape(-1)
        _ro(W3, err)
    return W3, K, sd, mu, err


# field: every k-step instantiation (P -> dispatch_ks 2 / 4 / 8 / 12 / 16), rows 1 and 37,
# ncols 1 and 130 (one past a 128-column panel), every regime; all four sd / err combinations
# and both output dtypes are run on every case
FIELD_CASES = (
    ("mid", 1, 1, 1), ("mid", 37, 5, 130), ("mid", 37, 64, 130), ("mid", 1, 25, 130),
    ("graded", 37, 12, 130), ("graded", 37, 64, 1), ("graded", 1, 40, 130),
    ("cancel", 37, 5, 130), ("cancel", 37, 40, 130), ("cancel", 1, 64, 130),
    ("offset", 37, 25, 130), ("offset", 37, 1, 130),
    ("f32edge", 37, 12, 130), ("f32edge", 1, 64, 130), ("f32edge", 37, 5, 1),
    ("ties", 37, 40, 130),
)
COMBOS = ((False, False), (True, False), (False, True), (True, True))      # (sd and mu, err)
# the exact power-of-two scalings (a = +-300) run on one 37-row case per regime
SCALED_FIELD_CASES = tuple(next(c for c in FIELD_CASES if c[0] == r and c[1] == 37 and c[3] == 130)
                           for r in FIELD_REGIMES)
SCALE_EXPONENTS = (-300, 300)

# summary / score: (regime, S, P, m, ncols, q, sd and mu, err).  S = 1, 2, 17, 33, 64 with
# q = 0, 0.025, 0.1, (0, 1): list depths 2, 4 and 8, partial 16- and 32-sample tiles; P = 8 / 40
# (32- and 16-row tiles); m = 1 / 3; ncols = 31 / 130
SUMMARY_CASES = (
    ("mid", 1, 8, 1, 31, 0.025, False, False),
    ("mid", 2, 40, 3, 130, 0, True, True),
    ("mid", 17, 8, 3, 31, 0.1, True, True),
    ("mid", 64, 40, 1, 130, 0.1, True, False),
    ("graded", 33, 40, 3, 31, 0.025, True, True),
    ("graded", 64, 8, 1, 130, (0, 1), False, True),
    ("cancel", 33, 8, 1, 130, 0.1, True, True),
    ("cancel", 17, 40, 3, 31, 0.025, False, True),
    ("offset", 64, 8, 3, 31, 0.025, True, True),
    ("offset", 33, 40, 1, 130, 0.1, True, True),
    ("offset", 17, 8, 1, 130, (0, 1), True, True),
    ("f32edge", 33, 8, 3, 31, 0.1, True, True),
    ("f32edge", 17, 40, 1, 130, 0.025, True, False),
    ("ties", 64, 8, 1, 130, 0.1, True, True),
    ("ties", 33, 40, 3, 31, 0.1, True, True),
    ("ties", 64, 40, 1, 130, 0.025, True, True),
    ("ties", 17, 8, 3, 31, 0.025, False, True),
    ("ties", 2, 8, 1, 31, (0, 1), True, True),
    ("ties", 33, 8, 1, 130, 0, False, False),
)
# the listed S and q stop at depth 8 (S = 64, q = 0.1); one order statistic more is refused
REFUSED = ((64, (0.12, 1.0), -13), (64, (0.0, 0.88), -14))


@functools.lru_cache(maxsize=None)
def _field_products(regime, rows, P, ncols):
    W, K = field_operands(regime, rows, P, ncols)[:2]
    return products(W, K)


@functools.lru_cache(maxsize=None)
def field_case_truth(regime, rows, P, ncols, sdmu, err):
    W, K, sd, mu, e = field_operands(regime, rows, P, ncols)
    return field_truth(W, K, sd if sdmu else None, mu if sdmu else None, e if err else None,
                       a=_field_products(regime, rows, P, ncols))


@functools.lru_cache(maxsize=None)
def summary_case_truth(case):
    regime, S, P, m, ncols, q, sdmu, err = case
    W3, K, sd, mu, e = summary_operands(regime, S, m, P, ncols, q)
    ft = field_truth(W3.reshape(S * m, P), K, sd if sdmu else None, mu if sdmu else None,
                     e if err else None)
    return ft, summary_truth(ft, S, m, q)


# ------------------------------------------------------------------------------------- noise
def _perms(n, base):
    return [np.random.default_rng(base + s).permutation(n) for s in range(NPERM)]


def _chain(W, K, order):
    acc = np.zeros((W.shape[0], K.shape[1]))
    for k in order:
        acc = acc + W[:, k, None] * K[k][None, :]
    return acc


def field_members(W, K, sd, mu, err):
    """(y, z) of every fp64 restatement: W @ K, the k-ordered chain, NPERM PC orders."""
    P = W.shape[1]
    for a in [W @ K, _chain(W, K, range(P))] + [_chain(W, K, p) for p in _perms(P, 100)]:
        y = a if sd is None else a * sd + mu
        if err is None:
            z = y
        else:
            z = a + err[:, None]
            z = z if sd is None else z * sd + mu
        yield y, z


def _col_err(x, t: DD):
    return np.max(np.abs((x - t.hi) - t.lo), axis=0)


def _field_noise(W, K, sd, mu, err, ft: FieldTruth):
    """Per-column noise of y and of z, and the members."""
    fl_y = 4.0 * EPS * np.max(np.abs(ft.y.hi), axis=0)
    fl_z = 4.0 * EPS * np.max(np.abs(ft.z.hi), axis=0)
    members = list(field_members(W, K, sd, mu, err))
    for y, z in members:
        fl_y = np.maximum(fl_y, _col_err(y, ft.y))
        fl_z = np.maximum(fl_z, _col_err(z, ft.z))
    return fl_y, fl_z, members


@functools.lru_cache(maxsize=None)
def field_noise(regime, rows, P, ncols, sdmu, err):
    """(noise of y, noise of z) per column of a field case."""
    W, K, sd, mu, e = field_operands(regime, rows, P, ncols)
    ft = field_case_truth(regime, rows, P, ncols, sdmu, err)
    return _field_noise(W, K, sd if sdmu else None, mu if sdmu else None, e if err else None,
                        ft)[:2]


def _cast(a, f32):
    return a.astype(np.float32).astype(np.float64) if f32 else a


@functools.lru_cache(maxsize=None)
def _summary_members(case):
    regime, S, P, m, ncols, q, sdmu, err = case
    W3, K, sd, mu, e = summary_operands(regime, S, m, P, ncols, q)
    ft, st = summary_case_truth(case)
    nz_y, nz_z, members = _field_noise(W3.reshape(S * m, P), K, sd if sdmu else None,
                                       mu if sdmu else None, e if err else None, ft)
    q_lo, q_hi = band(q)
    zmax = np.max(np.abs(ft.z.hi), axis=0)
    out = {"z": nz_z, "y": nz_y,
           "mean": np.broadcast_to(4.0 * EPS * np.max(np.abs(ft.y.hi), axis=0), (m, ncols)).copy()}
    maps = []
    for y, z in members:
        y3, z3 = y.reshape(S, m, ncols), z.reshape(S, m, ncols)
        means = [np.mean(y3, axis=0)] + [np.add.reduce(y3[p], axis=0) / S for p in _perms(S, 200)]
        for mm in means:
            out["mean"] = np.maximum(out["mean"], np.abs((mm - st.mean.hi) - st.mean.lo))
        maps.append((means[0], np.quantile(z3, q_lo, axis=0), np.quantile(z3, q_hi, axis=0)))
    out["lo"] = out["hi"] = np.broadcast_to(nz_z + 3.0 * EPS * zmax, (m, ncols))
    return out, maps


def summary_noise(case):
    """{"y", "z": per column; "mean", "lo", "hi": (m, ncols)}.  The mean: every field member's
    np.mean and NPERM orders of the samples; a quantile: the noise of z plus 3 eps max|z|."""
    return _summary_members(case)[0]


def trunc_members(Y, C, V, ranks, mu, sd):
    """e (R, n, ncols) of every fp64 restatement: C[:, :p] @ V[:p], the k-ordered chain, NPERM
    orders of k (the PCs below a rank in the permutation's order)."""
    Y = np.asarray(Y).astype(np.float64)
    e0 = Y if mu is None else Y - mu[None, :]
    s = 1.0 if sd is None else sd[None, :]
    pmax = max(ranks) if len(ranks) else 0
    yield np.stack([e0 - s * (C[:, :p] @ V[:p]) for p in ranks])
    for order in [np.arange(pmax)] + _perms(pmax, 300):
        yield np.stack([e0 - s * _chain(C, V, order[order < p]) for p in ranks])


def _trunc_stats(e, rp=None, cp=None):
    """tot, node, rmse, var of one residual stack (optionally with the rows / columns permuted
    before they are summed)."""
    if rp is not None:
        e = e[:, rp][:, :, cp]
    sq = e * e
    node = np.add.reduce(sq, axis=1)
    if cp is not None:
        node = node[:, np.argsort(cp)]
    tot = np.stack([np.sum(sq, axis=(1, 2)), np.sum(e, axis=(1, 2))], axis=1)
    N = float(e.shape[1] * e.shape[2])
    return tot, node, np.sqrt(tot[:, 0] / N), np.var(e, axis=(1, 2))


def trunc_noise(Y, C, V, ranks, mu, sd, t: TruncTruth):
    """{"sse", "sum", "rmse", "var": (R,); "node": (R, ncols)}; floors 4 eps of sum e^2, sum |e|,
    the RMSE, the variance itself and the node's own sum."""
    n, ncols = np.asarray(Y).shape
    out = {"sse": 4.0 * EPS * t.tot.hi[:, 0], "sum": 4.0 * EPS * t.abs1,
           "rmse": 4.0 * EPS * t.rmse.hi, "var": 4.0 * EPS * np.abs(t.var.hi),
           "node": 4.0 * EPS * t.node.hi}
    first = True
    for e in trunc_members(Y, C, V, ranks, mu, sd):
        views = [(None, None)]
        if first:
            views += list(zip(_perms(n, 400), _perms(ncols, 500)))
            first = False
        for rp, cp in views:
            tot, node, rmse, var = _trunc_stats(e, rp, cp)
            for nm, got, ref in (("sse", tot[:, 0], t.tot.take((slice(None), 0))),
                                 ("sum", tot[:, 1], t.tot.take((slice(None), 1))),
                                 ("rmse", rmse, t.rmse), ("var", var, t.var),
                                 ("node", node, t.node)):
                out[nm] = np.maximum(out[nm], np.abs((got - ref.hi) - ref.lo))
    return out


# ---------------------------------------------------------------------- gp_pca_trunc regimes
def even_spread(p, levels=32):
    return sorted(set(int(v) for v in np.linspace(0, p, levels).round()))


def reference_ranks(p):
    return sorted(set(int(min(r, p)) for r in _pca_ref.REFERENCE_RANKS))


# (regime, n, ncols, p, rank list, float32 Y, mu and sd): n = 1, 16, 17, 33 (one row tile, its
# edge, two sub-tiles, a ragged third tile); ncols = 1, 65, 130 (panels of 64); the rank lists
# of the issue: [0]; the reference's 26 ranks clipped to p; list(range(31)) + [128] at n = 33
# (padded inner dimension 224: the one-row-tile kernel although n > 16); an even spread of 32
TRUNC_CASES = (
    ("mid", 1, 1, 4, (0,), False, True),
    ("mid", 16, 65, 100, tuple(reference_ranks(100)), False, True),
    ("mid", 17, 130, 100, tuple(reference_ranks(100)), True, False),
    ("mid", 33, 130, 128, tuple(range(31)) + (128,), False, True),
    ("exact", 16, 130, 31, tuple(even_spread(31)), False, True),
    ("exact", 33, 65, 100, tuple(reference_ranks(100)), False, False),
    ("exact", 17, 1, 8, tuple(reference_ranks(8)), False, True),
    ("graded", 33, 130, 128, tuple(range(31)) + (128,), False, True),
    ("graded", 17, 65, 100, tuple(reference_ranks(100)), False, True),
    ("offset32", 33, 130, 40, tuple(reference_ranks(40)), True, True),
    ("offset32", 16, 65, 31, tuple(even_spread(31)), True, True),
    ("biased", 33, 130, 100, tuple(reference_ranks(100)), False, True),
    ("biased", 17, 65, 40, tuple(reference_ranks(40)), True, False),
    ("biased", 1, 130, 4, (0,), False, True),
)


SCALED_TRUNC_CASES = tuple(TRUNC_CASES[i] for i in (1, 4, 5, 8, 11))       # fp64 Y


@functools.lru_cache(maxsize=None)
def trunc_operands(regime, n, ncols, p, f32, stats):
    """(Y, C, V, mu, sd), read-only; mu = sd = None when not ``stats``.

    mid       _pca_ref.ensemble: signal + 1e-3 noise
    exact     Y = fl(mu + sd (C V)) at the full rank p: the last level's residual is Y's rounding
    graded    S_k = 10^(-12 k / p), Y = mu + sd (C V) + 1e-13 N
    offset32  float32 Y with column means about 1e4 over a unit spread
    biased    mid with mu off by delta = 1e4 x the residual's spread (Y itself without mu), so
              sum e dominates sum e^2 / N - (sum e / N)^2
    """
    seed = _seed(regime, n, ncols, p)
    dt = np.float32 if f32 else np.float64
    if regime in ("mid", "biased"):
        Y, C, V, mu, sd = _pca_ref.ensemble(n, ncols, p, seed, noise=TRUNC_NOISE, dtype=np.float64,
                                            stats=stats)
        if regime == "biased":
            Y = Y + BIAS * TRUNC_NOISE
        return _ro(Y.astype(dt), C, V, mu, sd)
    g = np.random.default_rng(seed)
    S = 10.0 ** (-12.0 * np.arange(p) / p) if regime == "graded" else 2.0 ** (-np.arange(p) / 4.0)
    C = g.standard_normal((n, p)) * S[None, :]
    V = g.standard_normal((p, ncols)) / np.sqrt(p)
    mu = sd = None
    if stats:
        mu = g.standard_normal(ncols) * 3.0
        sd = g.uniform(0.5, 2.0, ncols)
        if regime == "offset32":
            mu = 1e4 * (1.0 + 0.1 * g.standard_normal(ncols))
    Y = C @ V
    if stats:
        Y = mu[None, :] + sd[None, :] * Y
    if regime == "graded":
        Y = Y + 1e-13 * g.standard_normal((n, ncols))
    elif regime == "offset32":
        Y = Y + TRUNC_NOISE * g.standard_normal((n, ncols))
    elif regime != "exact":
        raise ValueError(regime)
    return _ro(Y.astype(dt), C, V, mu, sd)


@functools.lru_cache(maxsize=None)
def trunc_case(case):
    """(operands, truth, noise) of a TRUNC_CASES entry."""
    regime, n, ncols, p, ranks, f32, stats = case
    ops = trunc_operands(regime, n, ncols, p, f32, stats)
    t = trunc_truth(*ops[:3], ranks, ops[3], ops[4])
    return ops, t, trunc_noise(*ops[:3], list(ranks), ops[3], ops[4], t)


# ------------------------------------------- the library's own arithmetic (pca.TruncationCurve)
# TruncationCurve.var = sse / N - (sum / N)^2 is the one-pass form of the header (np.var =
# tot[2r] / N - (tot[2r+1] / N)^2): the kernel returns the two sums and nothing else.  With
# A = sse / N, B = sum / N and u = 2^-53 the fp64 evaluation is
#     fl(fl(sse' / N) - fl(fl(sum' / N)^2)) = (A (1 + a)(1 + d1) - B^2 (1 + b)^2 (1 + d2)^2 (1 + d3))
#                                             (1 + d4),   |d_i| <= u,
# sse' = sse (1 + a) and sum' = sum (1 + b) the kernel's sums.  To first order its error is
#     A (a + d1) - B^2 (2 b + 2 d2 + d3) + (A - B^2) d4,
# bounded by   |dsse| / N + 2 |B| |dsum| / N + u (A + 3 B^2 + |A - B^2|)
# with dsse, dsum the errors of the two sums (their own noise).  Relative to var = A - B^2 that is
# u (A + 3 B^2) / (A - B^2) + 1 and more: (B / spread)^2 = 1e8 units in the last place in the
# biased regime, where a two-pass np.var (the noise ensemble) stays at a few.  The information is
# lost in sse itself (its own rounding is u A), so no arithmetic on the two sums can restore it;
# a shifted sum would need a kernel change.
FINDINGS = frozenset([("var", "biased")])


def one_pass_var_term(t: TruncTruth, nz):
    """The bound derived above, per level, from the truth's A and B and the noise of the sums."""
    return (nz["sse"] + 2.0 * np.abs(t.B) * nz["sum"]) / t.N + \
        U * (t.A + 3.0 * t.B * t.B + np.abs(t.var.hi))


def trunc_limit(quantity, case):
    """The tests' bound: MARGIN x noise, plus MARGIN x the one-pass term at the findings."""
    _, t, nz = trunc_case(case)
    lim = MARGIN * nz[quantity]
    if (quantity, case[0]) in FINDINGS:
        lim = lim + MARGIN * one_pass_var_term(t, nz)
    return lim


# --------------------------------------------------------------------------- the score's truth
SCORE_FLOORS = (-np.inf, np.inf, float("nan"), 0.5)
# (summary case index, float32 outputs, float32 Y, mape_floor, tiny y): every regime, both
# output dtypes, both Y dtypes, the three special floors and a finite one; y of magnitude 1e-300
# among the APE terms where |mean / y| stays finite (fp64 Y)
SCORE_CASES = (
    (2, False, False, -np.inf, True),
    (3, True, True, 0.5, False),
    (4, False, True, np.inf, False),
    (6, False, False, float("nan"), True),
    (8, True, False, -np.inf, True),
    (9, False, False, 0.5, False),
    (11, False, False, -np.inf, False),
    (13, False, True, 0.5, False),
    (14, True, True, float("nan"), False),
)


SCALED_SCORE_CASES = (2, 9)                     # summary cases whose score is rescaled by 2^+-300


@functools.lru_cache(maxsize=None)
def score_Y(idx, f32, y_f32, tiny):
    """The score's truth field Y (m, ncols) for SUMMARY_CASES[idx]: around the truth's band --
    lo + u (hi - lo) with u in [-1, 2], so about a third is covered -- with every fifth element
    NaN and, when ``tiny``, every seventh +-1e-300; on a band of no width (float32 lo = hi) the
    offsets are taken from the level instead."""
    case = SUMMARY_CASES[idx]
    _, st = summary_case_truth(case)
    rng = np.random.default_rng(7000 + idx)
    lo, hi = st.lo.hi, st.hi.hi
    w = hi - lo
    w = np.where(w > 1e-11 * np.abs(hi), w, 1e-3 * np.maximum(np.abs(hi), 1e-3))
    u = rng.uniform(-1.0, 2.0, lo.shape)
    u = np.where(np.abs(u) < 0.05, u + 0.1, u)               # clear of the two edges by w / 20
    u = np.where(np.abs(u - 1.0) < 0.05, u + 0.1, u)
    Y = lo + u * w
    flat = Y.reshape(-1)
    if tiny and not y_f32:
        flat[3::7] = 1e-300 * rng.choice([-1.0, 1.0], flat[3::7].size)
    flat[1::5] = np.nan
    Y = Y.astype(np.float32) if y_f32 else Y
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def score_case(scase):
    """(Y, rows DD, cols DD, noise of rows (m, 8), noise of cols (ncols, 4), undecided): the
    truth's sums, their noise -- _score_ref.score_sums (numpy) on every field member's maps and on
    NPERM orders of the summed index, floored at 4 eps sum|terms| and at the maps' own noise
    carried through the terms -- and the number of elements of
    Y within MARGIN x noise of a band edge or of the floor (the tests need 0)."""
    idx, f32, y_f32, floor, tiny = scase
    case = SUMMARY_CASES[idx]
    m, ncols = case[3], case[4]
    _, st = summary_case_truth(case)
    nz, maps = _summary_members(case)
    Y = score_Y(idx, f32, y_f32, tiny)
    rows, cols, rabs, cabs = score_truth(st, f32, Y, floor)
    e_r, e_c = 4.0 * EPS * rabs, 4.0 * EPS * cabs
    # the sums are functions of the stored maps, which are themselves held to MARGIN x their
    # noise: a sum's noise is at least that noise carried through its terms to first order
    # (d (mu - y)^2 = 2 |mu - y| d + d^2, d |(mu - y) / y| = d / |y|, d (h - l) = dh + dl)
    R, C = _score_ref.ROW, _score_ref.COL
    y = np.asarray(Y).astype(np.float64)
    valid = ~np.isnan(y)
    y0 = np.where(valid, y, 1.0)
    dm, dl, dh = nz["mean"], nz["lo"], nz["hi"]
    dsq = np.where(valid, 2.0 * np.abs(_cast(st.mean.hi, f32) - y0) * dm + dm * dm, 0.0)
    with np.errstate(invalid="ignore"):
        dape = np.where(valid & ~(y < floor), dm / np.abs(y0), 0.0)
    p_r, p_c = np.zeros((m, 8)), np.zeros((ncols, 4))
    p_r[:, R["sqerr"]], p_r[:, R["ape"]] = dsq.sum(1), dape.sum(1)
    p_r[:, R["lo"]], p_r[:, R["hi"]], p_r[:, R["mean"]] = dl.sum(1), dh.sum(1), dm.sum(1)
    p_c[:, C["sqerr"]], p_c[:, C["width"]] = dsq.sum(0), (dl + dh).sum(0)
    e_r, e_c = np.maximum(e_r, p_r), np.maximum(e_c, p_c)
    first = True
    for mean, lo, hi in maps:
        maps_c = [_cast(a, f32) for a in (mean, lo, hi)]
        views = [(np.arange(m), np.arange(ncols))]
        if first:
            views += list(zip(_perms(m, 600), _perms(ncols, 700)))
            first = False
        for rp, cp in views:
            r, c = _score_ref.score_sums(*(a[rp][:, cp] for a in maps_c), Y[rp][:, cp], floor)[:2]
            e_r = np.maximum(e_r, np.abs((r[np.argsort(rp)] - rows.hi) - rows.lo))
            e_c = np.maximum(e_c, np.abs((c[np.argsort(cp)] - cols.hi) - cols.lo))
    y = np.asarray(Y).astype(np.float64)
    lo_s = _cast(st.lo.hi, f32)
    hi_s = _cast(st.hi.hi, f32)
    with np.errstate(invalid="ignore"):
        near = (np.abs(y - lo_s) <= MARGIN * nz["lo"]) | (np.abs(y - hi_s) <= MARGIN * nz["hi"])
        if np.isfinite(floor):
            near |= np.abs(y - floor) <= MARGIN * np.maximum(nz["lo"], nz["hi"])
    return Y, rows, cols, e_r, e_c, int(np.count_nonzero(near & ~np.isnan(y)))
