"""gp_predict_cov, gp_potrf on its output and gp_mvn_draw on the device against a 50-digit truth
(tests/_mp_joint_ref.py), in the regimes of tests/_mp_ref.py and at test points that sit on, next
to and twice on training points and each other: where C = K** + (s_pred + jitter - s) I - V^T V
is the small difference of two numbers of size s.

(a) C within limit_cov = MARGIN x the regime's own fp64 noise of the truth (plus the
    explicit-inverse term at _mp_joint_ref.FINDINGS_COV only), the diagonal held separately, both
    triangles and batch / alone equal to the bit, under every factorisation path, and d = 9, 17
    (the first of each rolled epilogue template) by zero-beta padding;
(b) the jitter touches the diagonal only; exact power-of-four scaling; the prior's whole argument
    range through the epilogue's exp_neg_scaled (n = 0) in all three D templates and both tiles;
(c) gp_potrf on the unpadded ld = m buffer against the 50-digit factor of the same fp64 matrix;
(d) positive definiteness at derived jitters: must factorise above, must fail below;
(e) gp_mvn_draw against 50-digit draws across its LDS rounds, row blocks and groups of 8.

Every problem asserts info == 0; nothing is skipped.  tools/extremes_ratios.py joint prints the
measured error / noise as DESIGN.md §7's table.
"""
import numpy as np
import pytest
import torch

import _mp_joint_ref as J
import _mp_ref as M
import test_gpu_extremes as TX

pytestmark = pytest.mark.gpu

EPS = M.EPS
MARGIN = M.MARGIN
_t, _info_ok, _bits_equal = TX._t, TX._info_ok, TX._bits_equal
COV_CASES = [(r, n, pts) for r in M.REGIMES for n, pts in J.CASES]
GROUP_CASES = [(g, n, pts) for g in M.GROUPS for n, pts in J.CASES]
WIDE_CASES = [(n, w) for n in J.WIDE_N for w in J.WIDE]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------ device set-up
_FACTORS, _COV = {}, {}


def _inputs(group, n, c=1.0):
    ps = [M.problem(r, n) for r in M.GROUPS[group]]
    return ps, dict(X=ps[0].X, beta=np.stack([p.beta for p in ps]),
                    s=np.array([p.s for p in ps]) * c, delta=np.array([p.delta for p in ps]) * c,
                    s_pred=np.array([p.s_pred for p in ps]) * c)


def _factorise(inp, dev):
    """kernels.gram + kernels.cholesky_inverse of a group under the path in force; info == 0."""
    from gladsgp_amd import kernels
    B = inp["beta"].shape[0]
    G = kernels.gram(_t(inp["X"], dev), _t(inp["beta"], dev), _t(inp["s"], dev),
                     _t(inp["delta"], dev), batch=B)
    ch = kernels.cholesky_inverse(G)
    _info_ok(ch.info, "gp_potrf_inv")
    return ch


def _chain(group, n, dev):
    """(problems, inputs, factorisation) of a regime group at one size, once per module."""
    key = (group, n)
    if key not in _FACTORS:
        ps, inp = _inputs(group, n)
        _FACTORS[key] = (ps, inp, _factorise(inp, dev))
    return _FACTORS[key]


def _predict_cov(ch, inp, Xs, dev, jitter=None, nugget=True, rows=slice(None)):
    from gladsgp_amd import kernels
    sp = inp["s_pred"] if nugget else inp["s"]
    jit = None if jitter is None else _t(np.asarray(jitter, dtype=np.float64)[rows], dev)
    C = kernels.predict_cov(ch, _t(inp["X"], dev), _t(Xs, dev), _t(inp["beta"][rows], dev),
                            _t(inp["s"][rows], dev), _t(sp[rows], dev), jitter=jit)
    return C


def _cov(group, n, pts, dev):
    """The group's C (batch, m, m) with the nugget and no jitter argument, once per module."""
    key = (group, n, pts)
    if key not in _COV:
        ps, inp, ch = _chain(group, n, dev)
        C = _predict_cov(ch, inp, J.points(ps[0].regime, n, pts), dev)
        _COV[key] = C.cpu().numpy()
    return _COV[key]


def _sub(ch, b):
    from gladsgp_amd import kernels
    return kernels.Cholesky(ch.n, ch.a_buf[b:b + 1], ch.linv_buf[b:b + 1].contiguous(),
                            ch.info[b:b + 1], ch.logdet[b:b + 1])


def _diag_err(t, C):
    idx = np.diag_indices(C.shape[0])
    return t.take(idx).err(C[idx])


# =========================================================== (a) the covariance against the truth
def cov_errors(dev, regime, n, pts):
    """(max-abs error of C, of its diagonal) against the truth (tools/extremes_ratios.py)."""
    group = M.group_of(regime)
    C = _cov(group, n, pts, dev)[M.GROUPS[group].index(regime)]
    t = J.truth_cov(regime, n, pts)
    return t.err(C), _diag_err(t, C)


@pytest.mark.parametrize("regime,n,pts", COV_CASES)
def test_cov_against_truth(dev, regime, n, pts):
    """max |C - truth| <= limit_cov, the diagonal against the same bound on its own, the two
    triangles bitwise equal."""
    group = M.group_of(regime)
    C = _cov(group, n, pts, dev)[M.GROUPS[group].index(regime)]
    nz, lim = J.noise_cov(regime, n, pts), J.limit_cov(regime, n, pts)
    err, derr = cov_errors(dev, regime, n, pts)
    print(f"C {regime} n={n} {pts}: err {err:.3e} diag {derr:.3e} noise {nz:.3e} ratio "
          f"{err / nz:.3g}, {MARGIN * err / lim:.3g} against the bound's 16")
    assert np.isfinite(C).all()
    assert err <= lim, (regime, n, pts, err / nz, MARGIN * err / lim)
    assert derr <= lim, (regime, n, pts, derr / nz)
    _bits_equal(C, np.ascontiguousarray(C.T), ("triangles", regime, n, pts))


@pytest.mark.parametrize("n,pts", J.CASES)
def test_batch_and_alone_have_the_same_bits(dev, n, pts):
    """The four d = 8 regimes as one batch against each problem alone."""
    ps, inp, ch = _chain("d8", n, dev)
    C = _cov("d8", n, pts, dev)
    Xs = J.points("mid", n, pts)
    for b in range(len(ps)):
        one = _predict_cov(_sub(ch, b), inp, Xs, dev, rows=slice(b, b + 1)).cpu().numpy()
        _bits_equal(one[0], C[b], ("alone", ps[b].regime, n, pts))


def test_cov_under_every_factorisation_path(dev):
    """L^-1 is the input: the d = 8 batch at (n, m) = (130, 130) under each path of gp_potrf_inv."""
    n, pts = 130, "wide130"
    ps, inp = _inputs("d8", n)
    Xs = J.points("mid", n, pts)
    paths = TX._potrf_paths(n, len(ps), dev)
    for path in paths:
        with TX._potrf_path(path):
            ch = _factorise(inp, dev)
        C = _predict_cov(ch, inp, Xs, dev).cpu().numpy()
        for b, p in enumerate(ps):
            t = J.truth_cov(p.regime, n, pts)
            err, lim = t.err(C[b]), J.limit_cov(p.regime, n, pts)
            print(f"C {p.regime} potrf path {path}: {MARGIN * err / lim:.3g} against 16")
            assert err <= lim and _diag_err(t, C[b]) <= lim, (p.regime, path, err / lim)


@pytest.mark.parametrize("n,pts", [(65, "wide65"), (130, "std")])
@pytest.mark.parametrize("d", [9, 17])
def test_padded_dimensions_reach_the_rolled_templates(dev, d, n, pts):
    """"mid" padded to d = 9 (jc_syrk_kernel<NT, 16>) and d = 17 (<NT, 32>) with zero-beta
    coordinates that hold random values.  Every added term is exact: the Gram and K* scale the
    coordinates by sqrt(0) = 0 and add a square of 0, the epilogue adds fma(0 t, t, dist) = dist,
    and its rolled loop accumulates in ard_dist's order (k ascending, fma(beta_k t_k, t_k, .)).
    No step differs, so C has the unpadded call's bits."""
    p = M.problem("mid", n)
    rng = np.random.default_rng([d, n])
    Xs = J.points("mid", n, pts)
    pad = d - p.d
    inp = dict(X=np.concatenate([p.X, rng.random((n, pad))], axis=1),
               beta=np.concatenate([p.beta, np.zeros(pad)])[None], s=np.array([p.s]),
               delta=np.array([p.delta]), s_pred=np.array([p.s_pred]))
    ch = _factorise(inp, dev)
    C = _predict_cov(ch, inp, np.concatenate([Xs, rng.random((Xs.shape[0], pad))], axis=1),
                     dev).cpu().numpy()[0]
    want = _cov("d8", n, pts, dev)[0]
    t, lim = J.truth_cov("mid", n, pts), J.limit_cov("mid", n, pts)
    print(f"d={d} n={n} {pts}: err {MARGIN * t.err(C) / lim:.3g} against 16")
    assert t.err(C) <= lim and _diag_err(t, C) <= lim
    _bits_equal(C, np.ascontiguousarray(C.T), ("triangles", d, n, pts))
    _bits_equal(C, want, ("padded against unpadded", d, n, pts))


# ================================================================== (b) jitter, scale, the prior
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_jitter_touches_the_diagonal_only(dev, group):
    """jitter = 0, 2^-30 s, s at (n, m) = (65, 65): the off-diagonal bits of the call without a
    jitter argument, the diagonal against truth_cov(jitter=...)."""
    n, pts = 65, "wide65"
    ps, inp, ch = _chain(group, n, dev)
    base = _cov(group, n, pts, dev)
    Xs = J.points(ps[0].regime, n, pts)
    off = ~np.eye(Xs.shape[0], dtype=bool)
    for mul in (0.0, 2.0 ** -30, 1.0):
        jit = mul * inp["s"]
        C = _predict_cov(ch, inp, Xs, dev, jitter=jit).cpu().numpy()
        for b, p in enumerate(ps):
            _bits_equal(C[b][off], base[b][off], ("off-diagonal", p.regime, mul))
            t = J.truth_cov(p.regime, n, pts, float(jit[b]))
            lim = J.limit_cov(p.regime, n, pts, float(jit[b]))
            derr = _diag_err(t, C[b])
            print(f"{p.regime} jitter {mul:g} s: diag {MARGIN * derr / lim:.3g} against 16")
            assert derr <= lim and t.err(C[b]) <= lim, (p.regime, mul, derr / lim)
        if mul == 0.0:
            _bits_equal(C, base, ("jitter 0 against no jitter", group))


@pytest.mark.parametrize("k", [-10, 10])
@pytest.mark.parametrize("group,n,pts", [(g, n, pts) for g in ("d8", "grid")
                                         for n, pts in ((65, "wide65"), (130, "wide130"))])
def test_exact_scaling(dev, group, n, pts, k):
    """s, delta, s_pred and the jitter times c = 4^k scale C by c to the bit: G scales by c and
    L^-1 by 2^-k (test_gpu_extremes.py (c)), K* and the prior by c (exp_neg(_tab)_scaled
    multiplies the polynomial's value by s before the ldexp), V = L^-1 K* by 2^k, V^T V by c, and
    fl(s_pred + jitter) by c; nothing leaves the normal range at these magnitudes, so no step is
    inexact."""
    c = 4.0 ** k
    ps, inp, ch = _chain(group, n, dev)
    Xs = J.points(ps[0].regime, n, pts)
    jit = 2.0 ** -30 * inp["s"]
    base = _predict_cov(ch, inp, Xs, dev, jitter=jit).cpu().numpy()
    _, inp_c = _inputs(group, n, c)
    ch_c = _factorise(inp_c, dev)
    got = _predict_cov(ch_c, inp_c, Xs, dev, jitter=jit * c).cpu().numpy()
    _bits_equal(got, base * c, ("scaled", group, n, pts, k))


def _prior_device(Xs, beta, s, diag_sp, jit, dev):
    """gp_predict_cov with n = 0 (no factor, no workspace): the epilogue alone."""
    from gladsgp_amd import _capi, kernels
    B, (m, d) = beta.shape[0], Xs.shape
    Xs_t, beta_t, s_t = _t(Xs, dev), _t(beta, dev), _t(s, dev)
    sp_t, jit_t = _t(diag_sp, dev), _t(jit, dev)
    any16 = torch.zeros(2, dtype=torch.float64, device=dev)
    C = torch.full((B, m, m), -7.25, dtype=torch.float64, device=dev)
    assert _capi.lib().gp_predict_cov_ws_bytes(0, m, B) == 0
    _capi.call("gp_predict_cov", any16.data_ptr(), 0, 0, any16.data_ptr(), d, Xs_t.data_ptr(), d,
               0, m, d, beta_t.data_ptr(), d, s_t.data_ptr(), sp_t.data_ptr(), jit_t.data_ptr(),
               C.data_ptr(), m, m * m, B, None, 0, kernels._stream(dev))
    torch.cuda.synchronize()
    return C.cpu().numpy()


@pytest.mark.parametrize("regime", M.REGIMES)
def test_no_training_points_gives_the_prior(dev, regime):
    """n = 0 in every regime (the 12 random points of problem(regime, 0)): truth_cov's prior
    within limit_cov, fl(s_pred + jitter) itself on the diagonal."""
    p = M.problem(regime, 0)
    assert p.X.shape[0] == 0
    jit = 2.0 ** -30 * p.s
    C = _prior_device(p.Xs, p.beta[None], np.array([p.s]), np.array([p.s_pred]),
                      np.array([jit]), dev)[0]
    t, lim = J.truth_cov(regime, 0, "std", jit), J.limit_cov(regime, 0, "std", jit)
    print(f"prior {regime}: {MARGIN * t.err(C) / lim:.3g} against 16")
    assert t.err(C) <= lim
    np.testing.assert_array_equal(np.diag(C), np.full(p.m, p.s_pred + jit))
    np.testing.assert_array_equal(C, C.T)


@pytest.mark.parametrize("m", [60, 70])
@pytest.mark.parametrize("d", [1, 8, 9, 16, 17, 32])
def test_prior_whole_range(dev, d, m):
    """n = 0: every entry of the prior against the 50-digit kernel value over acc = 0 ... 1200
    (test_gpu_extremes._spread in the first coordinate), at s = 2^-20, 1, 2^20, with
    _check_values' rule 2 bound_rel t + 2^-1074 and exactly +0 below 2^-1075, bound_rel being
    the epilogue's own (_mp_joint_ref.bound_rel_epilogue); d = 1, 8 / 9, 16 / 17, 32 are both ends
    of jc_syrk_kernel's three D templates, m = 60 / 70 its 64- and 128-tiles.  The diagonal is
    fl(s_pred + jitter) to the bit."""
    rng = np.random.default_rng([600, d, m])
    Xs = 0.25 * rng.random((m, d))
    Xs[:, 0] = TX._spread(m, rng)
    Xs[1, 1:] = Xs[0, 1:]                      # a repeated point: acc exactly 0 off the diagonal
    rows = np.ones((2, d))
    rows[0, 1:] = rng.uniform(0.5, 5.0, d - 1)
    rows[1, 1:] = rng.uniform(0.5, 5.0, d - 1) * (np.arange(1, d) % 2)      # zeros among them
    beta = np.repeat(rows, 3, axis=0)
    s = np.tile(TX.S_A, 2)
    sp, jit = s * 1.01, s * 2.0 ** -30
    C = _prior_device(Xs, beta, s, sp, jit, dev)
    total = np.zeros(3, dtype=int)
    for r in range(2):
        truth = M.kernel_values(Xs, Xs, rows[r])
        bound = J.bound_rel_epilogue(Xs, Xs, rows[r])
        for b in (3 * r, 3 * r + 1, 3 * r + 2):
            np.testing.assert_array_equal(C[b], C[b].T)
            np.testing.assert_array_equal(np.diag(C[b]), np.full(m, sp[b] + jit[b]))
            offd = C[b].copy()
            offd[np.diag_indices(m)] = s[b]      # the truth's diagonal is s exp(0)
            total += TX._check_values(offd, truth, bound, s[b], ("prior", d, m, b))
    assert np.all(total > 0), total              # the sweep reached all three classes


@pytest.mark.parametrize("m", [60, 70])
@pytest.mark.parametrize("d", [8, 9, 17])
def test_prior_exact_arguments(dev, d, m):
    """Integer coordinates with beta in {0, 1, 4}: the differences, beta t, and every fma of the
    distance are exact (integers far below 2^53), so bound_rel_epilogue is left with its last
    term and a prior value owes the truth 2 eps (exp_neg's ulp and the scale) + 2^-1074 at every
    argument 0 ... 1225: where an error of the exp's range reduction, which grows with the
    argument as the bound itself does, has nowhere to hide (test_gpu_extremes.py does the same
    for the Gram's exp)."""
    rng = np.random.default_rng([700, d, m])
    Xs = np.zeros((m, d))
    Xs[:, 0] = (np.arange(m) * 7) % 36
    Xs[:, 1:] = rng.integers(0, 3, (m, d - 1))
    rows = np.ones((2, d))
    rows[0, 1:] = rng.choice([0.0, 1.0, 4.0], d - 1)
    rows[1, 1:] = 0.0
    beta = np.repeat(rows, 3, axis=0)
    s = np.tile(TX.S_A, 2)
    C = _prior_device(Xs, beta, s, s * 1.01, 0.0 * s, dev)
    total = np.zeros(3, dtype=int)
    for r in range(2):
        truth = M.kernel_values(Xs, Xs, rows[r])
        for b in (3 * r, 3 * r + 1, 3 * r + 2):
            offd = C[b].copy()
            offd[np.diag_indices(m)] = s[b]
            total += TX._check_values(offd, truth, np.full((m, m), EPS), s[b],
                                      ("prior, exact arguments", d, m, b))
    assert np.all(total > 0), total


# ================================================================================ (c) the factor
FACTOR_CASES = [(130, "one"), (65, "std"), (65, "wide65"), (130, "wide130")]
_FACTOR_RUNS = {}


def _factor_run(dev, n, pts, nugget):
    """gp_potrf (ld = m, in place) on the fp64-rounded truth C of all seven regimes as one batch;
    without the nugget with the derived jitter of (d).  Returns (C, logical buffer, logdet)."""
    from gladsgp_amd import kernels
    key = (n, pts, nugget)
    if key not in _FACTOR_RUNS:
        Cn = np.stack([J.truth_cov(r, n, pts, 0.0 if nugget else J.sufficient_jitter(r, n, pts),
                                   nugget).hi for r in M.REGIMES])
        buf = _t(Cn, dev)
        info, logdet = kernels.cholesky_inplace(buf)
        _info_ok(info, ("gp_potrf", n, pts, nugget))
        _FACTOR_RUNS[key] = (Cn, np.swapaxes(buf.cpu().numpy(), 1, 2), logdet.cpu().numpy())
    return _FACTOR_RUNS[key]


def factor_errors(dev, regime, n, pts, nugget):
    """((error, noise) of R, (error, noise) of logdet) (tools/extremes_ratios.py)."""
    Cn, Rl, logdet = _factor_run(dev, n, pts, nugget)
    b = M.REGIMES.index(regime)
    Rt, ldt = J.truth_factor(Cn[b])
    nR, nld = J.noise_factor(Cn[b])
    return (Rt.err(np.tril(Rl[b])), nR), (ldt.err(logdet[b]), nld)


@pytest.mark.parametrize("nugget", [True, False])
@pytest.mark.parametrize("n,pts", FACTOR_CASES)
def test_factor_against_truth(dev, n, pts, nugget):
    """cholesky_inplace on exact input at m = 1, 24, 65, 130: the factor and the log-determinant
    within MARGIN x what LAPACK delivers on the same matrix, the other triangle untouched."""
    Cn, Rl, _ = _factor_run(dev, n, pts, nugget)
    m = Cn.shape[1]
    iu = np.triu_indices(m, 1)
    for b, regime in enumerate(M.REGIMES):
        (eR, nR), (eld, nld) = factor_errors(dev, regime, n, pts, nugget)
        print(f"R {regime} m={m} nugget={nugget}: err {eR:.3e} noise {nR:.3e} ratio "
              f"{eR / nR:.3g}; logdet ratio {eld / nld:.3g}")
        assert eR <= MARGIN * nR, (regime, m, nugget, eR / nR)
        assert eld <= MARGIN * nld, (regime, m, nugget, eld / nld)
        assert np.array_equal(Rl[b][iu], Cn[b][iu])


# ===================================================================== (d) positive definiteness
@pytest.mark.parametrize("group,n,pts", [(g, n, w) for g in M.GROUPS for n, w in WIDE_CASES])
def test_positive_definite_at_the_derived_jitter(dev, group, n, pts):
    """Without the nugget the exact repeats make the true C singular.  With jitter J = 2 (m E + F)
    (_mp_joint_ref.sufficient_jitter: E = limit_cov, F the Cholesky's backward error) the device
    must factorise and draw finite values; with -(lambda_min(truth) + J) the device's C has an
    eigenvalue <= -(m E + 2 F) and the factorisation must report it."""
    from gladsgp_amd import kernels
    ps, inp, ch = _chain(group, n, dev)
    Xs = J.points(ps[0].regime, n, pts)
    jit = np.array([J.sufficient_jitter(p.regime, n, pts) for p in ps])
    lam = np.array([J.lambda_min(p.regime, n, pts) for p in ps])
    for p, jv, lv in zip(ps, jit, lam):
        print(f"{p.regime} n={n} {pts}: derived jitter {jv / p.s:.3e} s, lambda_min(truth) "
              f"{lv / p.s:.2e} s")
    C = _predict_cov(ch, inp, Xs, dev, jitter=jit, nugget=False)
    info, _ = kernels.cholesky_inplace(C)
    _info_ok(info, ("gp_potrf at the derived jitter", group, n, pts))
    kernels.check_joint_info(info, 3)
    assert torch.isfinite(kernels.mvn_draw(C, None, 1, 0, 3)).all()
    C = _predict_cov(ch, inp, Xs, dev, jitter=-(lam + jit), nugget=False)
    info, _ = kernels.cholesky_inplace(C)
    assert (info.cpu().numpy() > 0).all(), info.cpu().tolist()
    with pytest.raises(kernels.JointNotPositiveDefinite, match=r"unit 3 at pivot") as exc:
        kernels.check_joint_info(info, 3)
    assert [u for u, _ in exc.value.units] == list(range(3, 3 + len(ps)))


def _default_jitter():
    """EmulatorPrediction's joint_jitter without the nugget, a multiple of s."""
    from gladsgp_amd.emulator import EmulatorPrediction
    return EmulatorPrediction.joint_jitter_default


def default_jitter_run(dev, group, n=130, pts="wide130"):
    """[(regime, derived J / s, info, draws finite)] at the emulator's default jitter, no
    nugget."""
    from gladsgp_amd import kernels
    DEFAULT_JITTER = _default_jitter()
    ps, inp, ch = _chain(group, n, dev)
    C = _predict_cov(ch, inp, J.points(ps[0].regime, n, pts), dev,
                     jitter=DEFAULT_JITTER * inp["s"], nugget=False)
    info, _ = kernels.cholesky_inplace(C)
    draws = kernels.mvn_draw(C, None, 1, 0, 3)
    return [(p.regime, J.sufficient_jitter(p.regime, n, pts) / p.s, int(v),
             bool(torch.isfinite(draws[b]).all()))
            for b, (p, v) in enumerate(zip(ps, info.cpu().tolist()))]


@pytest.mark.parametrize("group", list(M.GROUPS))
def test_default_jitter_at_130_points(dev, group):
    """The emulator's default 1e-8 s against the derived sufficient jitter at m = 130.  Where the
    default is at or above it the factorisation must succeed; where it is below, the derived
    value is a sufficient condition only and both are recorded."""
    DEFAULT_JITTER = _default_jitter()
    for regime, derived, info, finite in default_jitter_run(dev, group):
        print(f"{regime}: default {DEFAULT_JITTER:g} s, derived sufficient {derived:.3e} s, "
              f"info {info}, draws finite {finite}")
        if DEFAULT_JITTER >= derived:
            assert info == 0 and finite, (regime, derived, info)


# ================================================================================= (e) the draws
DRAW_SEED, DRAW_OFFSET, DRAW_UNIT0 = 2024, 5, 3
_DRAW_R = {}


def _draw_factor(dev, m):
    """The device's own factor of "mid" and "flat" at n = 65 and m seeded random test points
    (with the nugget): (buffer on the device, logical R [b, i, k], mean)."""
    from gladsgp_amd import kernels
    if m not in _DRAW_R:
        ps, inp, ch = _chain("d8", 65, dev)
        rng = np.random.default_rng([m, 77])
        C = _predict_cov(ch, inp, rng.random((m, 8)), dev)[:2].contiguous()
        info, _ = kernels.cholesky_inplace(C)
        _info_ok(info, ("gp_potrf for the draws", m))
        _DRAW_R[m] = (C, np.swapaxes(C.cpu().numpy(), 1, 2), rng.standard_normal((2, m)))
    return _DRAW_R[m]


def draw_errors(dev, m, nsamp):
    """(elementwise error, elementwise bound, its noise part without the margin, the per-element
    bound that weighs every normal by its own fp64 error)."""
    from gladsgp_amd import kernels
    buf, Rl, mean = _draw_factor(dev, m)
    got = kernels.mvn_draw(buf, _t(mean, dev), DRAW_SEED, DRAW_OFFSET, nsamp,
                           unit0=DRAW_UNIT0).cpu().numpy()
    assert got.shape == (2, nsamp, m)
    t, mag, magerr = J.truth_draws(Rl, mean, DRAW_SEED, DRAW_OFFSET, nsamp, unit0=DRAW_UNIT0)
    lo, hi = DRAW_UNIT0 * nsamp * m, (DRAW_UNIT0 + 2) * nsamp * m
    rel = max(J.normals_rel_error(hi, DRAW_SEED, DRAW_OFFSET, lo), 4.0 * EPS)
    acc = (m + 2) * EPS / 2.0 * (np.abs(mean)[:, None, :] + mag)
    noise = rel * mag + acc
    bound = MARGIN * rel * mag + acc
    tight = MARGIN * magerr + acc
    assert np.all(tight <= bound * (1 + 8 * EPS))
    return np.abs((got - t.hi) - t.lo), bound, noise, tight


@pytest.mark.parametrize("nsamp", [1, 8, 9])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_draws_against_truth(dev, m, nsamp):
    """mean + tril(R) xi with unit0 = 3 across the 64-column LDS round (m = 63, 64, 65), the
    256-row block (257) and the group of 8 draws (8, 9).  Per element: MARGIN x (the worst
    relative error of the fp64 stream oracle.rng_ref.normals against the 50-digit one, at least
    4 eps) x sum_k |R_ik xi_k| for the normals, plus (m + 2) eps / 2 of |mean_i| + sum_k |R_ik
    xi_k| for the m-term fma accumulation and the final add.

    That worst relative error is set by the few normals whose cos / sin(2 pi u2) sits next to a
    zero (numpy rounds 2 pi u2 first: up to 1.3e-11), and would let an error of 1e-12 in every
    normal pass.  So the same form is also asserted with every normal weighed by its own fp64
    error: MARGIN x sum_k |R_ik| max(e_k, 4 eps |xi_k|) in the first term, never above the bound
    before and up to 26 times below it (measured)."""
    err, bound, _, tight = draw_errors(dev, m, nsamp)
    print(f"draws m={m} nsamp={nsamp}: worst error / bound {float(np.max(err / bound)):.3g}, "
          f"/ per-element bound {float(np.max(err / tight)):.3g}")
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.all(err <= tight), float(np.max(err / tight))


@pytest.mark.parametrize("m", [65, 257])
def test_draws_scale_with_the_factor(dev, m):
    """R times 2^k rescales the mean-free draws to the bit."""
    from gladsgp_amd import kernels
    buf, _, _ = _draw_factor(dev, m)
    base = kernels.mvn_draw(buf, None, DRAW_SEED, DRAW_OFFSET, 9, unit0=DRAW_UNIT0).cpu().numpy()
    assert np.isfinite(base).all() and np.abs(base).max() > 0
    for k in (-7, 9):
        got = kernels.mvn_draw((buf * 2.0 ** k).contiguous(), None, DRAW_SEED, DRAW_OFFSET, 9,
                               unit0=DRAW_UNIT0).cpu().numpy()
        _bits_equal(got, base * 2.0 ** k, ("draws", m, k))
