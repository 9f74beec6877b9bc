"""The GP chain on the device against a 50-digit truth, at the hyperparameter extremes the
sampler can reach (tests/_mp_ref.py: truth, regimes, noise level).

(a) kernel values of gp_gram_ardse / gp_cross_ardse / the prediction's K* over the whole
    argument range of the two hand-written exps (0 ... past the 1100 clamp), every entry within
    2 bound_rel (+ 2^-1074) of the mpmath value;
(b) every quantity of the chain, from every entry point that produces it, within MARGIN = 16
    times the regime's own fp64 noise of the truth under every factorisation path; only at the
    documented findings (_mp_ref.FINDINGS: the 1-D grid from n = 64 on) plus the term the
    library's explicit-inverse arithmetic adds (_mp_ref.explicit_inverse_term);
(c) exact power-of-two scaling of s, delta, s_pred and of w: no absolute threshold anywhere.

Every problem asserts info == 0; nothing is skipped.  tools/extremes_ratios.py prints the
measured error / noise of (b) as DESIGN.md §7's table.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
from mpmath import mp, mpf

import _mp_ref as M

pytestmark = pytest.mark.gpu

EPS = M.EPS
MARGIN = M.MARGIN
CASES = [(r, n) for r in M.REGIMES for n in M.SIZES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=dev)


def _lib():
    from gladsgp_amd import _capi
    return _capi.lib()


@contextlib.contextmanager
def _potrf_path(path):
    prev = _lib().gp_set_potrf_path(path)
    try:
        yield
    finally:
        _lib().gp_set_potrf_path(prev)


@contextlib.contextmanager
def _predict_path(path):
    prev = _lib().gp_set_predict_path(path)
    try:
        yield
    finally:
        _lib().gp_set_predict_path(prev)


def _info_ok(info, what):
    assert info.cpu().tolist() == [0] * info.numel(), (what, info.cpu().tolist())


# =============================================================== (a) kernel values, whole range
N_A, M_A = 65, 70
S_A = (2.0 ** -20, 1.0, 2.0 ** 20)


def _spread(count, rng):
    """First-coordinate values whose pairwise squared gaps (beta_0 = 1) sweep the exps' whole
    argument range: exactly 0 (a repeated point), 1e-20, the usual range, 100 - 700, the
    subnormal window (708.4, 745.1), just past underflow, and past the 1100 clamp."""
    acc = np.concatenate([
        [0.0, 0.0, 1e-20], rng.uniform(0.01, 40.0, 8), rng.uniform(100.0, 700.0, 10),
        np.linspace(708.5, 745.0, 14), [745.14, 745.2, 745.5, 746.0, 750.0, 760.0, 800.0],
        [1000.0, 1099.9, 1100.0, 1100.1, 1150.0, 1200.0]])
    acc = np.concatenate([acc, rng.uniform(0.0, 1200.0, count - acc.size)])
    return np.sqrt(acc[:count])


@pytest.fixture(scope="module", params=[1, 8, 9, 16, 17, 32])
def kv(request, dev):
    """Device Gram and cross-covariance of one d (a batch of 3 beta rows x 3 scales) and the
    50-digit exp(-acc) of every pair, computed once."""
    from gladsgp_amd import kernels
    d = request.param
    rng = np.random.default_rng(500 + d)
    X, Xs = 0.25 * rng.random((N_A, d)), 0.25 * rng.random((M_A, d))
    X[:, 0], Xs[:, 0] = _spread(N_A, rng), _spread(M_A, rng)
    X[1, 1:] = X[0, 1:]                        # a repeated point: acc exactly 0 off the diagonal
    X[2, 1:] = X[0, 1:]                        # and one 1e-10 away in one coordinate
    Xs[0], Xs[2] = X[0], X[2]
    rows = np.ones((3, d))
    rows[0, 1:] = rng.uniform(0.5, 5.0, d - 1)
    rows[1, 1:] = rng.uniform(0.5, 5.0, d - 1) * (np.arange(1, d) % 2)      # zeros among them
    rows[2, 0], rows[2, 1:] = 0.25, 0.0                                     # one live dimension
    beta = np.repeat(rows, 3, axis=0)
    s = np.tile(S_A, 3)
    delta = 1e-6 * s
    G = kernels.gram(_t(X, dev), _t(beta, dev), _t(s, dev), _t(delta, dev)).cpu().numpy()
    Kt = kernels.cross(_t(X, dev), _t(Xs, dev), _t(beta, dev), _t(s, dev)).cpu().numpy()
    truth_g = [M.kernel_values(X, X, rows[r]) for r in range(3)]
    truth_k = [M.kernel_values(Xs, X, rows[r]) for r in range(3)]
    return dict(d=d, X=X, Xs=Xs, rows=rows, s=s, delta=delta, G=G, Kt=Kt, truth_g=truth_g,
                truth_k=truth_k)


def _check_values(got, truth, bound, s, what):
    """Every entry within 2 bound_rel t + 2^-1074 of t = s truth; +0 exactly where t < 2^-1075.
    Returns how many truths fell in (normal, subnormal, zero)."""
    counts = [0, 0, 0]
    with mp.workdps(M.DPS):
        sm, tiny, half_tiny = mpf(s), mpf(2) ** -1074, mpf(2) ** -1075
        for i, row in enumerate(truth):
            for j, e in enumerate(row):
                t, g = sm * e, float(got[i][j])
                assert g == g and g >= 0.0 and not np.signbit(g), (what, i, j, g)
                if t < half_tiny:
                    assert g == 0.0, (what, i, j, g, float(t))
                    counts[2] += 1
                    continue
                counts[0 if t >= mpf(2) ** -1022 else 1] += 1
                err, lim = abs(mpf(g) - t), 2 * mpf(float(bound[i][j])) * t + tiny
                assert err <= lim, (what, i, j, g, float(t), float(err / lim))
    return counts


def test_gram_values_whole_range(kv):
    """gp_gram_ardse against the 50-digit kernel value over acc = 0 ... 1200 (ardse_kernel<D> at
    both ends of its d range, zero betas, s = 2^-20, 1, 2^20); G_ii = fl(s + delta) to the bit;
    G bitwise symmetric."""
    total = np.zeros(3, dtype=int)
    for b in range(9):
        G, s, delta = kv["G"][b], kv["s"][b], kv["delta"][b]
        np.testing.assert_array_equal(G, G.T)
        np.testing.assert_array_equal(np.diag(G), np.full(N_A, s + delta))
        off = G.copy()
        off[np.diag_indices(N_A)] = s            # the truth's diagonal is s exp(0)
        bound = M.bound_rel(kv["X"], kv["X"], kv["rows"][b // 3])
        total += _check_values(off, kv["truth_g"][b // 3], bound, s, ("gram", kv["d"], b))
    assert np.all(total > 0), total              # the sweep reached all three classes


def test_cross_values_whole_range(kv):
    """gp_cross_ardse (m = 70 test points against n = 65) the same way."""
    total = np.zeros(3, dtype=int)
    for b in range(9):
        bound = M.bound_rel(kv["Xs"], kv["X"], kv["rows"][b // 3])
        total += _check_values(kv["Kt"][b], kv["truth_k"][b // 3], bound, kv["s"][b],
                               ("cross", kv["d"], b))
    assert np.all(total > 0), total


@pytest.mark.parametrize("d", [1, 8, 9, 16, 17, 32])
def test_values_exact_arguments(dev, d):
    """Integer coordinates with beta in {0, 1, 4}: sqrt(beta), the scaled coordinates, their
    differences, squares and sums are all exact (integers far below 2^53), so every term of
    bound_rel but the last is a rounding that does not happen and the kernel value owes the
    truth 2 eps (exp's ulp and the scale) + 2^-1074, at every argument 0 ... 1225.  This is
    where an error of the exp's range reduction, which grows with the argument like bound_rel
    itself does, has nowhere to hide."""
    from gladsgp_amd import kernels
    rng = np.random.default_rng(700 + d)
    n, m = 65, 70
    X, Xs = np.zeros((n, d)), np.zeros((m, d))
    X[:, 0], Xs[:, 0] = np.arange(n) % 36, (np.arange(m) * 7) % 36
    X[:, 1:] = rng.integers(0, 3, (n, d - 1))
    Xs[:, 1:] = rng.integers(0, 3, (m, d - 1))
    rows = np.ones((2, d))
    rows[0, 1:] = rng.choice([0.0, 1.0, 4.0], d - 1)
    rows[1, 1:] = 0.0
    beta = np.repeat(rows, 3, axis=0)
    s = np.tile(S_A, 2)
    G = kernels.gram(_t(X, dev), _t(beta, dev), _t(s, dev), _t(0.0 * s, dev)).cpu().numpy()
    Kt = kernels.cross(_t(X, dev), _t(Xs, dev), _t(beta, dev), _t(s, dev)).cpu().numpy()
    total = np.zeros(3, dtype=int)
    for r in range(2):
        tg, tk = M.kernel_values(X, X, rows[r]), M.kernel_values(Xs, X, rows[r])
        for b in (3 * r, 3 * r + 1, 3 * r + 2):
            total += _check_values(G[b], tg, np.full((n, n), EPS), s[b], ("gram", d, b))
            total += _check_values(Kt[b], tk, np.full((m, n), EPS), s[b], ("cross", d, b))
    assert np.all(total > 0), total


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("pad_d", [1, 12])
@pytest.mark.parametrize("ppath", [0, 1, 2])
def test_kstar_through_diagonal_system(dev, ppath, pad_d, exact):
    """The prediction's K* has no output of its own: training points at the integers 0 .. n-1
    with beta = 800 make every off-diagonal Gram entry underflow to +0, so A = (s + delta) I
    exactly and, with w one-hot at i, mean_j = k(x_i, xs_j) / (s + delta) to three more
    roundings (L^-1_ii, z_i, the product).  Test points at x_i +- t, 800 t^2 = 0 ... 700; on
    prediction paths 0 / 1 / 2, and padded to d = 12 (the chunked cross-covariance).

    ``exact``: beta = 900 and t = k / 32, k = 0 ... 28, with s + delta = 1 + 2^-13 exact:
    sqrt(beta) = 30, the scaled coordinates 30 (i + k / 32), their differences and the argument
    900 k^2 / 1024 = 0 ... 689 are all exact, so bound_rel is left with its last term, 2 eps (the
    table exp's ulp and the scale), at every argument and every x_i: 2 (2 eps) + 4 eps."""
    from gladsgp_amd import kernels
    n, hot = 65, [0, 17, 63, 64]
    b0 = 900.0 if exact else 800.0
    s, delta = (1.0, 2.0 ** -13) if exact else (1.0, 1e-4)
    acc = np.array([0.0, 1e-20, 1e-6, 0.03, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 40.0, 80.0, 150.0,
                    300.0, 450.0, 600.0, 690.0, 700.0])
    tt = np.arange(29) / 32.0 if exact else np.sqrt(acc / b0)
    pts = np.concatenate([v for i in hot for v in (i + tt, i - tt[1:])])
    X = np.zeros((n, pad_d))
    Xs = np.zeros((pts.size, pad_d))
    X[:, 0], Xs[:, 0] = np.arange(n), pts
    beta = np.ones((len(hot), pad_d))
    beta[:, 0] = b0
    W = np.zeros((len(hot), n))
    W[np.arange(len(hot)), hot] = 1.0
    B = len(hot)
    Xd, Xsd, bd = _t(X, dev), _t(Xs, dev), _t(beta, dev)
    G = kernels.gram(Xd, bd, s, delta, batch=B)
    expect = np.zeros((n, n))
    expect[np.diag_indices(n)] = s + delta
    for b in range(B):
        Gb = G[b].cpu().numpy()
        np.testing.assert_array_equal(Gb, expect)
        assert not np.signbit(Gb).any()
    ch = kernels.cholesky_inverse(G)
    _info_ok(ch.info, "diagonal system")
    with _predict_path(ppath):
        mean, var = kernels.predict(ch, Xd, Xsd, bd, s, s + 0.01, _t(W, dev))
    mean = mean.cpu().numpy()
    assert np.all(np.isfinite(var.cpu().numpy()))
    for b, i in enumerate(hot):
        kt = M.kernel_values(Xs, X[i:i + 1], beta[b], s)
        bound = M.bound_rel(Xs, X[i:i + 1], beta[b])[:, 0]
        if exact:
            bound = np.full(pts.size, 2.0 * EPS)
        with mp.workdps(M.DPS):
            for j in range(pts.size):
                t = kt[j][0] / (mpf(s) + mpf(delta))
                err = abs(mpf(float(mean[b, j])) - t)
                lim = (2 * mpf(float(bound[j])) + 4 * mpf(EPS)) * t + mpf(2) ** -1074
                assert err <= lim, (ppath, pad_d, i, j, float(mean[b, j]), float(t),
                                    float(err / lim))


# ====================================================== (b) the chain against the truth per regime
def _group_inputs(group, n):
    ps = [M.problem(r, n) for r in M.GROUPS[group]]
    return ps, dict(
        X=ps[0].X, Xs=ps[0].Xs, beta=np.stack([p.beta for p in ps]),
        s=np.array([p.s for p in ps]), delta=np.array([p.delta for p in ps]),
        s_pred=np.array([p.s_pred for p in ps]), W=np.stack([p.w for p in ps]))


def _potrf_paths(n, batch, dev):
    """1 (the blocked sweep) always; 0 and 2 where gp_pp_plan reports the persistent kernel
    eligible for either the factorisation with L^-1 or the plain one."""
    from gladsgp_amd import _capi
    lib = _lib()
    eligible = False
    with _potrf_path(0):
        for inv in (0, 1):
            out = (ctypes.c_longlong * len(_capi.PP_PLAN))()
            stream = torch.cuda.current_stream(dev).cuda_stream
            assert lib.gp_pp_plan_stream(n, batch, inv, -1, out, stream) == 0
            eligible = eligible or bool(dict(zip(_capi.PP_PLAN, out))["eligible"])
    return (0, 1, 2) if eligible else (1,)


def _run_chain(inp, n, dev, scale_w=1.0):
    """Every entry point of the chain once, under the factorisation path now in force: a dict
    source -> numpy array with the batch in front (matrices logical [b][i][j])."""
    from gladsgp_amd import kernels
    X, Xs, beta = _t(inp["X"], dev), _t(inp["Xs"], dev), _t(inp["beta"], dev)
    s, delta, sp = _t(inp["s"], dev), _t(inp["delta"], dev), _t(inp["s_pred"], dev)
    W = _t(inp["W"] * scale_w, dev)
    B = W.shape[0]
    out = {}
    G = kernels.gram(X, beta, s, delta, batch=B)
    out["G"] = G
    ch = kernels.cholesky_inverse(G.clone())
    _info_ok(ch.info, "gp_potrf_inv")
    out["L/potrf_inv"], out["Linv/potrf_inv"], out["logdet/potrf_inv"] = ch.L, ch.Linv, ch.logdet
    Lp, info, logdet = kernels.cholesky(G.clone())
    _info_ok(info, "gp_potrf")
    out["L/potrf"], out["logdet/potrf"] = Lp, logdet
    tr = kernels.trtri(ch.L)
    _info_ok(tr.info, "gp_trtri")
    out["Linv/trtri"] = tr.Linv
    out["z/trmv"] = kernels.trmv(ch, W)
    out["z/predict_z"] = kernels.predict_z(ch, W)[:, :n]
    out["nll/nll"] = kernels.nll(ch, W)
    lws = kernels.LoglikWorkspace(n, B, dev)
    out["loglik/loglik"] = kernels.loglik(X, beta.contiguous(), s, delta, W, lws)
    _info_ok(lws.info, "gp_loglik")
    lws.check_status()
    out["alpha/alpha"] = kernels.alpha(ch, W)
    for pp in (0, 1, 2):
        with _predict_path(pp):
            out[f"mean/predict{pp}"], out[f"var/predict{pp}"] = kernels.predict(
                ch, X, Xs, beta, s, sp, W)
    mean, var, info = kernels.predict_chol(ch.L, X, Xs, beta, s, sp, W)
    _info_ok(info, "gp_predict_chol")
    out["mean/predict_chol"], out["var/predict_chol"] = mean, var
    mean, var, chf = kernels.fit_predict(X, Xs, beta, s, delta, sp, W, check=False)
    _info_ok(chf.info, "gp_fit_predict")
    out["mean/fit_predict"], out["var/fit_predict"], out["L/fit_predict"] = mean, var, chf.L
    with kernels.FitPredictContext(dev) as ctx:
        mean, var, chf = kernels.fit_predict(X, Xs, beta, s, delta, sp, W, ctx=ctx, check=False)
        torch.cuda.synchronize()
    _info_ok(chf.info, "gp_fit_predict (context)")
    out["mean/fit_predict_ctx"], out["var/fit_predict_ctx"] = mean, var
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_CHAIN = {}


def _chain(group, n, dev):
    """{potrf path: outputs} of one regime group at one size, computed once per module."""
    key = (group, n)
    if key not in _CHAIN:
        ps, inp = _group_inputs(group, n)
        res = {}
        for path in _potrf_paths(n, len(ps), dev):
            with _potrf_path(path):
                res[path] = _run_chain(inp, n, dev)
        _CHAIN[key] = res
    return _CHAIN[key]


SOURCES = {
    "L": ["L/potrf_inv", "L/potrf", "L/fit_predict"],
    "Linv": ["Linv/potrf_inv", "Linv/trtri"],
    "logdet": ["logdet/potrf_inv", "logdet/potrf"],
    "z": ["z/trmv", "z/predict_z"],
    "nll": ["nll/nll", "loglik/loglik"],
    "alpha": ["alpha/alpha"],
}


def chain_errors(dev, source, regime, n):
    """{factorisation path: max-abs error against the truth} of one source (tools/
    extremes_ratios.py makes DESIGN.md's table from this)."""
    quantity = source.split("/")[0]
    group = M.group_of(regime)
    b = M.GROUPS[group].index(regime)
    tq = getattr(M.truth_of(regime, n), "nll" if quantity == "loglik" else quantity)
    errs = {}
    for path, out in _chain(group, n, dev).items():
        x = out[source][b]
        x = -x if quantity == "loglik" else (np.tril(x) if quantity == "L" else x)
        errs[path] = tq.err(x)
    return errs


def _assert_quantity(dev, source, regime, n):
    """error <= MARGIN x noise under every factorisation path (plus MARGIN x the explicit-inverse
    term at the documented findings, _mp_ref.FINDINGS); var >= -that."""
    quantity = source.split("/")[0]
    ref = "nll" if quantity == "loglik" else quantity
    group = M.group_of(regime)
    b = M.GROUPS[group].index(regime)
    nz, lim = M.noise(ref, regime, n), M.limit(ref, regime, n)
    errs = chain_errors(dev, source, regime, n)
    for path, err in errs.items():
        print(f"{source} {regime} n={n} potrf path {path}: err {err:.3e} noise {nz:.3e} "
              f"ratio {err / nz:.3g}, {MARGIN * err / lim:.3g} against the bound's 16")
    for path, err in errs.items():
        assert err <= lim, (source, regime, n, path, err / nz, MARGIN * err / lim)
        if quantity == "var":
            low = float(np.min(_chain(group, n, dev)[path][source][b]))
            assert low >= -lim, (source, regime, n, path, low / lim)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", SOURCES["L"])
def test_chain_L(dev, source, regime, n):
    _assert_quantity(dev, source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", SOURCES["Linv"])
def test_chain_Linv(dev, source, regime, n):
    _assert_quantity(dev, source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", SOURCES["logdet"])
def test_chain_logdet(dev, source, regime, n):
    _assert_quantity(dev, source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", SOURCES["z"])
def test_chain_z(dev, source, regime, n):
    _assert_quantity(dev, source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", SOURCES["nll"])
def test_chain_nll_loglik(dev, source, regime, n):
    _assert_quantity(dev, source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
def test_chain_alpha(dev, regime, n):
    _assert_quantity(dev, "alpha/alpha", regime, n)


PRED_SOURCES = ["predict0", "predict1", "predict2", "predict_chol", "fit_predict",
                "fit_predict_ctx"]


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", PRED_SOURCES)
def test_chain_mean(dev, source, regime, n):
    _assert_quantity(dev, "mean/" + source, regime, n)


@pytest.mark.parametrize("regime,n", CASES)
@pytest.mark.parametrize("source", PRED_SOURCES)
def test_chain_var(dev, source, regime, n):
    _assert_quantity(dev, "var/" + source, regime, n)


# ========================================================================= (c) exact scaling
SCALED = ["G", "L/potrf_inv", "L/potrf", "L/fit_predict", "Linv/potrf_inv", "Linv/trtri",
          "z/trmv", "z/predict_z", "alpha/alpha"] + \
    [f"{q}/{s}" for q in ("mean", "var") for s in PRED_SOURCES]


def _bits_equal(a, b, what):
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), \
        (what, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("k", [-10, 10])
@pytest.mark.parametrize("regime,n", [(r, n) for r in ("mid", "grid") for n in (65, 130)])
def test_exact_scaling(dev, regime, n, k):
    """s, delta, s_pred times c = 4^k: G and var scale by c, L by 2^k, L^-1 by 2^-k, mean keeps
    its bits, z and alpha scale by 2^-k and c^-1.  w times 2^k: z, alpha and mean scale by 2^k,
    var keeps its bits.  Bitwise after the power-of-two rescale (nothing under- or overflows at
    these magnitudes), under every factorisation path."""
    group = M.group_of(regime)
    _, inp = _group_inputs(group, n)
    b = M.GROUPS[group].index(regime)
    c, r = 4.0 ** k, 2.0 ** k
    inp_c = dict(inp, s=inp["s"] * c, delta=inp["delta"] * c, s_pred=inp["s_pred"] * c)
    base = _chain(group, n, dev)
    for path in base:
        with _potrf_path(path):
            hyp = _run_chain(inp_c, n, dev)
            wsc = _run_chain(inp, n, dev, scale_w=r)
        for src in SCALED:
            q = src.split("/")[0]
            f_hyp = {"G": c, "var": c, "L": r, "Linv": 1 / r, "mean": 1.0, "z": 1 / r,
                     "alpha": 1 / c}[q]
            f_w = {"G": 1.0, "var": 1.0, "L": 1.0, "Linv": 1.0, "mean": r, "z": r, "alpha": r}[q]
            ref = base[path][src][b]
            _bits_equal(hyp[src][b], ref * f_hyp, ("hyper", src, regime, n, k, path))
            _bits_equal(wsc[src][b], ref * f_w, ("w", src, regime, n, k, path))
