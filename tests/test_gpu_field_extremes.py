"""The field back end on the device against a 50-digit truth, at scaling extremes
(tests/_mp_field_ref.py: truth, regimes, noise level).

(a) gp_field (blas.field) through every k-step instantiation, rows 1 / 37, ncols 1 / 130, all four
    sd / err combinations, fp64 and float32 (half a float32 ulp of the truth on top; +-inf exactly
    where the truth rounds to it, subnormal results included);
(b) gp_field_summary: mean, lo, hi against the truth; lo / hi bit for bit against
    np.quantile of the device's own fp64 field (summary.hip's claim about numpy's _lerp, here an
    assertion); exact duplicates at the selected positions and across the merge partners; the
    refusal one order statistic past the deepest list;
(c) gp_field_score: every count exactly (tests/test_mp_field_ref_cpu.py shows that no element of
    Y is within 16 x noise of an edge), every sum against the truth's;
(d) gp_pca_trunc: the sums, the node map, TruncationCurve.rmse and .var per level; a level's bits
    do not depend on the other levels where the residual is pure rounding;
(e) exact power-of-two scaling of all of it (field, summary, score, gp_pca_trunc), bit for bit,
    at 2^+-300.

Every assertion is error <= MARGIN x noise (MARGIN = 16), plus the derived one-pass term only at
the entries of _mp_field_ref.FINDINGS (TruncationCurve.var in the biased regime, the one-pass
form's cancellation).  Nothing is skipped.
tools/extremes_ratios.py prints the measured error / noise as DESIGN.md section 7's fourth table.
"""
import numpy as np
import pytest
import torch

import _mp_field_ref as F
from _score_ref import COL, COL_COUNTS, ROW, ROW_COUNTS

pytestmark = pytest.mark.gpu

EPS = F.EPS
MARGIN = F.MARGIN


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


def _t(x, dev):
    return None if x is None else torch.as_tensor(np.array(x, order="C"), device=dev)


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = np.int64 if a.dtype == np.float64 else np.int32
    assert np.array_equal(a.view(view), b.view(view)), \
        (what, int(np.count_nonzero(a.view(view) != b.view(view))))


def _worst(e, nz):
    """max error / noise; 0 / 0 counts as 0."""
    e, nz = np.broadcast_arrays(np.asarray(e, dtype=float), np.asarray(nz, dtype=float))
    with np.errstate(all="ignore"):
        ratio = np.where(nz > 0, e / nz, np.where(e > 0, np.inf, 0.0))
    return float(np.max(ratio)) if ratio.size else 0.0


def _err(x, t):
    """|x - truth| per element (DD)."""
    return np.abs((np.asarray(x, dtype=np.float64) - t.hi) - t.lo)


def _f32_excess(got32, rows_m, t):
    """A float32 result against the truth rounded once: +-inf exactly where the truth rounds to
    it; elsewhere what |got - truth| exceeds half a float32 ulp of the truth by (>= 0).  Also
    returns the number of subnormal expectations."""
    want = F.f32_of(rows_m)
    got = np.asarray(got32).astype(np.float64)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    assert not np.isnan(got).any()
    fin = ~inf
    exc = np.zeros(got.shape)
    exc[fin] = np.maximum(0.0, np.abs((got[fin] - t.hi[fin]) - t.lo[fin]) - 0.5 * F.ulp_f32(t.hi[fin]))
    sub = fin & (want != 0) & (np.abs(want) < 2.0 ** F.F32_MIN_EXP)
    return exc, int(np.count_nonzero(sub)), int(np.count_nonzero(inf))


# ================================================================================= (a) field
def field_run(dev, case, sdmu, err, f32=False, wexp=0, kexp=0, oexp=0):
    """blas.field on a case's operands; W 2^wexp, K 2^kexp, (sd, mu) 2^oexp."""
    from gladsgp_amd import blas
    W, K, sd, mu, e = F.field_operands(*case)
    out = blas.field(_t(np.ldexp(W, wexp), dev), _t(np.ldexp(K, kexp), dev),
                     _t(np.ldexp(sd, oexp), dev) if sdmu else None,
                     _t(np.ldexp(mu, oexp), dev) if sdmu else None,
                     _t(e, dev) if err else None, f32=f32)
    return out.cpu().numpy()


def field_errors(dev, case):
    """[(sdmu, err, fp64 error (rows, ncols), noise (ncols), float32 excess, subnormals, infs)]."""
    out = []
    for sdmu, err in F.COMBOS:
        t = F.field_case_truth(*case, sdmu, err)
        nz = F.field_noise(*case, sdmu, err)[1 if err else 0]
        tz, rows_m = (t.z, t.zm) if err else (t.y, t.ym)
        got = field_run(dev, case, sdmu, err)
        assert got.dtype == np.float64 and np.all(np.isfinite(got))
        got32 = field_run(dev, case, sdmu, err, f32=True)
        assert got32.dtype == np.float32
        exc, nsub, ninf = _f32_excess(got32, rows_m, tz)
        out.append((sdmu, err, _err(got, tz), nz, exc, nsub, ninf))
    return out


@pytest.mark.parametrize("case", F.FIELD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_field_against_truth(dev, case):
    """fp64: every element within MARGIN x noise.  float32: within half a float32 ulp of the
    truth + MARGIN x noise, +-inf exactly where the truth rounds to it, subnormals included."""
    nsub = ninf = 0
    for sdmu, err, e64, nz, exc, s, i in field_errors(dev, case):
        print(f"{case} sdmu={sdmu} err={err}: fp64 error / noise {_worst(e64, nz):.3g}, "
              f"float32 excess / noise {_worst(exc, nz):.3g} ({s} subnormal, {i} infinite)")
        assert np.all(e64 <= MARGIN * nz), (case, sdmu, err, _worst(e64, nz))
        assert np.all(exc <= MARGIN * nz), (case, sdmu, err, _worst(exc, nz))
        nsub, ninf = nsub + s, ninf + i
    if case[0] == "f32edge" and case[3] > 1:
        assert nsub > 0 and ninf > 0, (nsub, ninf)


@pytest.mark.parametrize("a", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("case", F.SCALED_FIELD_CASES, ids=lambda c: c[0])
def test_field_exact_scaling(dev, case, a):
    """W 2^a with K 2^-a: identical bits.  (sd, mu) 2^a: every output 2^a.  W 2^a without sd, mu
    and err: every output 2^a.  Everything stays in the normal range (asserted)."""
    W, K, sd, mu, e = F.field_operands(*case)
    assert F.all_normal(np.ldexp(W, a), np.ldexp(K, -a), np.ldexp(sd, a), np.ldexp(mu, a))
    for sdmu, err in F.COMBOS:
        base = field_run(dev, case, sdmu, err)
        _bits_equal(field_run(dev, case, sdmu, err, wexp=a, kexp=-a), base, ("W K", case, sdmu, err))
        if sdmu:
            got = field_run(dev, case, sdmu, err, oexp=a)
            assert F.all_normal(base, got)
            _bits_equal(got, np.ldexp(base, a), ("sd mu", case, err, a))
    base = field_run(dev, case, False, False)
    got = field_run(dev, case, False, False, wexp=a)
    assert F.all_normal(base, got)
    _bits_equal(got, np.ldexp(base, a), ("W", case, a))


# =============================================================================== (b) summary
def summary_run(dev, case, f32=False, wexp=0, kexp=0, oexp=0):
    """(mean, lo, hi) of blas.field_summary and the device's own fp64 field z (S, m, ncols)."""
    from gladsgp_amd import blas
    regime, S, P, m, ncols, q, sdmu, err = case
    W3, K, sd, mu, e = F.summary_operands(regime, S, m, P, ncols, q)
    Wd, Kd = _t(np.ldexp(W3, wexp), dev), _t(np.ldexp(K, kexp), dev)
    sdd = _t(np.ldexp(sd, oexp), dev) if sdmu else None
    mud = _t(np.ldexp(mu, oexp), dev) if sdmu else None
    ed = _t(e, dev) if err else None
    got = blas.field_summary(Wd, Kd, sdd, mud, ed, q=q, f32=f32)
    z = blas.field(Wd.reshape(S * m, P), Kd, sdd, mud, ed)
    return tuple(g.cpu().numpy() for g in got), z.cpu().numpy().reshape(S, m, ncols)


def summary_errors(dev, case):
    """{"mean" | "lo" | "hi": (error, noise, float32 excess)}, the fp64 maps and z_dev."""
    ft, st = F.summary_case_truth(case)
    nz = F.summary_noise(case)
    (mean, lo, hi), z = summary_run(dev, case)
    got32, _ = summary_run(dev, case, f32=True)
    out = {}
    for nm, g, g32, t, tm in (("mean", mean, got32[0], st.mean, st.mean_m),
                              ("lo", lo, got32[1], st.lo, st.lo_m), ("hi", hi, got32[2], st.hi, st.hi_m)):
        assert g.dtype == np.float64 and g32.dtype == np.float32
        with np.errstate(over="ignore", under="ignore"):
            _bits_equal(g32, g.astype(np.float32), (nm, "float32 = the fp64 result rounded", case))
        out[nm] = (_err(g, t), nz[nm], _f32_excess(g32, tm, t)[0])
    return out, (mean, lo, hi), got32, z


@pytest.mark.parametrize("case", F.SUMMARY_CASES, ids=lambda c: "-".join(map(str, c[:6])))
def test_summary_against_truth(dev, case):
    regime, S, P, m, ncols, q, sdmu, err = case
    errs, (mean, lo, hi), (mean32, lo32, hi32), z = summary_errors(dev, case)
    ft, st = F.summary_case_truth(case)
    for nm, (e, nz, exc) in errs.items():
        print(f"{nm} {case}: error / noise {_worst(e, nz):.3g}, float32 excess / noise "
              f"{_worst(exc, nz):.3g}")
    # the field the summary never stores is the field blas.field stores: held to the truth here
    zn = F.summary_noise(case)["z"]
    assert np.all(_err(z.reshape(S * m, ncols), ft.z) <= MARGIN * zn)
    for nm, (e, nz, exc) in errs.items():
        assert np.all(e <= MARGIN * nz), (nm, case, _worst(e, nz))
        assert np.all(exc <= MARGIN * nz), (nm, "float32", case, _worst(exc, nz))
    assert np.all(hi >= lo) and np.all(hi32 >= lo32)
    # numpy's rule on the device's own samples, bit for bit (position, selection and _lerp)
    q_lo, q_hi = F.band(q)
    _bits_equal(lo, np.quantile(z, q_lo, axis=0), ("lo", case))
    _bits_equal(hi, np.quantile(z, q_hi, axis=0), ("hi", case))
    if regime == "ties":
        # where z_(j) = z_(j+1) exactly the quantile is that sample's value itself
        ii, cc = np.indices((m, ncols))
        for nm, g, tied, src in (("lo", lo, st.tied_lo, st.src_lo), ("hi", hi, st.tied_hi, st.src_hi)):
            _bits_equal(g[tied], z[src, ii, cc][tied], ("tied " + nm, case))
        assert np.count_nonzero(st.tied_lo) + np.count_nonzero(st.tied_hi) > 0
    if regime == "offset":
        # a band of 1e-9 of its level: float32 lo == hi wherever the truth rounds so
        same = F.f32_of(st.lo_m) == F.f32_of(st.hi_m)
        assert same.any() and np.array_equal(lo32[same], hi32[same])


@pytest.mark.parametrize("S,q,rc", F.REFUSED)
def test_summary_refuses_depth_nine(dev, S, q, rc):
    from gladsgp_amd import _capi, blas
    assert max(F.tail_depths(S, q)) == blas.field_summary_max_tail() + 1
    W3, K, sd, mu, e = F.summary_operands("mid", S, 1, 8, 31, 0.1)
    with pytest.raises(_capi.GPFitError) as ei:
        blas.field_summary(_t(W3, dev), _t(K, dev), q=q)
    assert ei.value.rc == rc
    with pytest.raises(_capi.GPFitError) as ei:
        blas.field_score(_t(W3, dev), _t(K, dev), q=q)
    assert ei.value.rc == rc


@pytest.mark.parametrize("a", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("idx", [2, 4, 9, 13])
def test_summary_exact_scaling(dev, idx, a):
    """W 2^a with K 2^-a: identical bits; (sd, mu) 2^a: mean, lo, hi 2^a to the bit."""
    case = F.SUMMARY_CASES[idx]
    assert case[6]
    base, _ = summary_run(dev, case)
    same, _ = summary_run(dev, case, wexp=a, kexp=-a)
    scaled, _ = summary_run(dev, case, oexp=a)
    assert F.all_normal(*base, *scaled)
    for nm, b, s, c in zip(("mean", "lo", "hi"), base, same, scaled):
        _bits_equal(s, b, (nm, "W K", case, a))
        _bits_equal(c, np.ldexp(b, a), (nm, "sd mu", case, a))


# ================================================================================= (c) score
def score_run(dev, scase, cols=True):
    from gladsgp_amd import blas
    idx, f32, y_f32, floor, tiny = scase
    regime, S, P, m, ncols, q, sdmu, err = F.SUMMARY_CASES[idx]
    W3, K, sd, mu, e = F.summary_operands(regime, S, m, P, ncols, q)
    Y = F.score_Y(idx, f32, y_f32, tiny)
    got = blas.field_score(_t(W3, dev), _t(K, dev), _t(sd, dev) if sdmu else None,
                           _t(mu, dev) if sdmu else None, _t(e, dev) if err else None,
                           Y=_t(np.array(Y), dev), q=q, mape_floor=floor, f32=f32, cols=cols)
    return got[0].cpu().numpy(), None if got[1] is None else got[1].cpu().numpy()


def score_errors(dev, scase):
    """(rows error, rows noise, cols error, cols noise, rows, cols) -- counts included."""
    Y, rows_t, cols_t, e_r, e_c, undecided = F.score_case(scase)
    assert undecided == 0
    rows, cols = score_run(dev, scase)
    return _err(rows, rows_t), e_r, _err(cols, cols_t), e_c, rows, cols


@pytest.mark.parametrize("scase", F.SCORE_CASES,
                         ids=lambda s: f"{F.SUMMARY_CASES[s[0]][0]}-{s[0]}-{s[1]}-{s[2]}-{s[3]}")
def test_score_against_truth(dev, scase):
    Y, rows_t, cols_t = F.score_case(scase)[:3]
    er, nr, ec, nc, rows, cols = score_errors(dev, scase)
    sums_r = [k for k in range(8) if k not in ROW_COUNTS]
    sums_c = [k for k in range(4) if k not in COL_COUNTS]
    print(f"{scase}: row sums error / noise {_worst(er[:, sums_r], nr[:, sums_r]):.3g}, "
          f"column sums {_worst(ec[:, sums_c], nc[:, sums_c]):.3g}")
    for k in ROW_COUNTS:
        assert np.array_equal(rows[:, k], rows_t.hi[:, k]), ("row count", k, scase)
    for k in COL_COUNTS:
        assert np.array_equal(cols[:, k], cols_t.hi[:, k]), ("column count", k, scase)
    assert np.all(er[:, sums_r] <= MARGIN * nr[:, sums_r]), (scase, _worst(er[:, sums_r], nr[:, sums_r]))
    assert np.all(ec[:, sums_c] <= MARGIN * nc[:, sums_c]), (scase, _worst(ec[:, sums_c], nc[:, sums_c]))
    if scase[4]:
        assert np.all(rows_t.hi[:, ROW["ape"]] > 1e290)          # the 1e-300 truths are counted
    rows_only, none = score_run(dev, scase, cols=False)
    assert none is None
    _bits_equal(rows_only, rows, ("cols=False", scase))
    assert cols[:, COL["width"]].min() >= 0.0


@pytest.mark.parametrize("a", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("idx", F.SCALED_SCORE_CASES)
def test_score_exact_scaling(dev, idx, a):
    """sd, mu, Y and the floor 2^a: the sums of l, h, mu and of the widths 2^a, the squared errors
    2^2a, the percentage errors and every count unchanged, bit for bit."""
    from gladsgp_amd import blas
    regime, S, P, m, ncols, q, sdmu, err = F.SUMMARY_CASES[idx]
    assert sdmu
    W3, K, sd, mu, e = F.summary_operands(regime, S, m, P, ncols, q)
    Y = np.array(F.score_Y(idx, False, False, False))

    def run(k):
        rows, cols = blas.field_score(_t(W3, dev), _t(K, dev), _t(np.ldexp(sd, k), dev),
                                      _t(np.ldexp(mu, k), dev), _t(e, dev) if err else None,
                                      Y=_t(np.ldexp(Y, k), dev), q=q, mape_floor=np.ldexp(0.5, k))
        return rows.cpu().numpy(), cols.cpu().numpy()

    rows, cols = run(0)
    rows_a, cols_a = run(a)
    assert F.all_normal(rows, cols, rows_a, cols_a)
    power_r = np.zeros(8, dtype=np.int64)
    power_r[[ROW["lo"], ROW["hi"], ROW["mean"]]] = a
    power_r[ROW["sqerr"]] = 2 * a
    power_c = np.zeros(4, dtype=np.int64)
    power_c[COL["width"]], power_c[COL["sqerr"]] = a, 2 * a
    _bits_equal(rows_a, np.ldexp(rows, power_r[None, :]), ("rows", idx, a))
    _bits_equal(cols_a, np.ldexp(cols, power_c[None, :]), ("cols", idx, a))
    assert rows[:, ROW["ape_n"]].sum() > 0 and rows[:, ROW["covered"]].sum() > 0


# ============================================================================= (d) pca_trunc
def trunc_run(dev, case, node=True, ranks=None, yexp=0, cexp=0, vexp=0):
    """(tot (R, 2), node (R, ncols) or None) of blas.pca_trunc; Y, mu, sd 2^yexp, C 2^cexp,
    V 2^vexp."""
    from gladsgp_amd import blas
    regime, n, ncols, p, rk, f32, stats = case
    Y, C, V, mu, sd = F.trunc_operands(regime, n, ncols, p, f32, stats)
    Yd = _t(np.ldexp(Y, yexp) if yexp else np.array(Y), dev)
    tot, nod = blas.pca_trunc(Yd, _t(np.ldexp(C, cexp), dev), _t(np.ldexp(V, vexp), dev),
                              list(rk if ranks is None else ranks),
                              mu=_t(np.ldexp(mu, yexp), dev) if stats else None,
                              sd=_t(np.ldexp(sd, yexp), dev) if stats else None, node=node)
    return tot.cpu().numpy(), None if nod is None else nod.cpu().numpy()


def trunc_curve(dev, case):
    """TruncationCurve of pca.truncation_error on the case (S = 1: C is U diag(S) already)."""
    from gladsgp_amd import pca
    regime, n, ncols, p, rk, f32, stats = case
    Y, C, V, mu, sd = F.trunc_operands(regime, n, ncols, p, f32, stats)
    return pca.truncation_error((np.array(C), np.ones(p), np.array(V)),
                                np.array(mu) if stats else 0.0, np.array(sd) if stats else 1.0,
                                np.array(Y), ranks=list(rk), node=True,
                                device=dev)


def trunc_errors(dev, case):
    """{"sse" | "sum" | "node" | "rmse" | "var": (error, noise, bound)} per level."""
    _, t, nz = F.trunc_case(case)
    tot, node = trunc_run(dev, case)
    tot_only, none = trunc_run(dev, case, node=False)
    assert none is None
    _bits_equal(tot_only, tot, ("tot with and without node", case))
    cv = trunc_curve(dev, case)
    if case[6]:
        _bits_equal(np.asarray(cv.sse), tot[:, 0], ("TruncationCurve.sse", case))
        _bits_equal(np.asarray(cv.sum), tot[:, 1], ("TruncationCurve.sum", case))
    got = {"sse": (tot[:, 0], t.tot.take((slice(None), 0))), "sum": (tot[:, 1], t.tot.take((slice(None), 1))),
           "node": (node, t.node), "rmse": (np.asarray(cv.rmse), t.rmse),
           "var": (np.asarray(cv.var), t.var)}
    return {nm: (_err(g, tt), nz[nm], F.trunc_limit(nm, case)) for nm, (g, tt) in got.items()}


@pytest.mark.parametrize("case", F.TRUNC_CASES,
                         ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{len(c[4])}-{c[5]}-{c[6]}")
def test_pca_trunc_against_truth(dev, case):
    errs = trunc_errors(dev, case)
    for nm, (e, nz, lim) in errs.items():
        print(f"{nm} {case[:4]}: worst error / noise {_worst(e, nz):.3g}, "
              f"{MARGIN * _worst(e, lim):.3g} against the bound's 16")
    for nm, (e, nz, lim) in errs.items():
        assert np.all(np.isfinite(e)) and np.all(e <= lim), (nm, case, _worst(e, nz), _worst(e, lim))


@pytest.mark.parametrize("case", [c for c in F.TRUNC_CASES if c[0] in ("exact", "graded")],
                         ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{len(c[4])}")
def test_pca_trunc_levels_are_independent(dev, case):
    """Every level asked for alone, and the list in two halves: the bits of the one call, where
    the deep levels' residual is nothing but rounding."""
    tot, node = trunc_run(dev, case)
    rk = list(case[4])
    for r, p in enumerate(rk):
        t1, n1 = trunc_run(dev, case, ranks=[p])
        _bits_equal(t1[0], tot[r], ("tot", case, p))
        _bits_equal(n1[0], node[r], ("node", case, p))
    h = len(rk) // 2
    if h:
        for part, sl in ((rk[:h], slice(0, h)), (rk[h:], slice(h, None))):
            t2, n2 = trunc_run(dev, case, ranks=part)
            _bits_equal(t2, tot[sl], ("tot", case, part))
            _bits_equal(n2, node[sl], ("node", case, part))


@pytest.mark.parametrize("a", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("case", F.SCALED_TRUNC_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_pca_trunc_exact_scaling(dev, case, a):
    """Y, mu, sd 2^a: sum e^2 and node 2^2a, sum e 2^a.  C 2^a with V 2^-a: identical bits."""
    tot, node = trunc_run(dev, case)
    same_t, same_n = trunc_run(dev, case, cexp=a, vexp=-a)
    _bits_equal(same_t, tot, ("tot, C V", case, a))
    _bits_equal(same_n, node, ("node, C V", case, a))
    sc_t, sc_n = trunc_run(dev, case, yexp=a, cexp=a if not case[6] else 0)
    want = np.stack([np.ldexp(tot[:, 0], 2 * a), np.ldexp(tot[:, 1], a)], axis=1)
    assert F.all_normal(tot, node, want, sc_t, sc_n)
    _bits_equal(sc_t, want, ("tot, Y mu sd", case, a))
    _bits_equal(sc_n, np.ldexp(node, 2 * a), ("node, Y mu sd", case, a))
