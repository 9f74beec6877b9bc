"""The PCA front end on the device against an 80-digit truth, at spectral extremes
(tests/_mp_pca_ref.py: truth, regimes, noise level).

(a) gp_sim_stats / gp_standardize through both kernels (the row-quartered one below ny = 65536
    and the thread-per-location one from there on), n = 1 ... 37, columns with a large mean over
    a tiny spread, constant columns, deviations one ulp either side of the floor; exact
    power-of-two scaling;
(b) gp_syevj at r = 1, 2, 25, 64, 65 on graded, clustered, indefinite, diagonal and zero inputs,
    and exact power-of-two scaling up to 2^+-600 (the stop rule has no absolute threshold);
(c) randomized_svd on every regime: S, identifiable vectors, cluster projectors, both
    orthonormalities and the truncation residual;
(d) the basis and the PC weights on the device's own K.

Every assertion is error <= MARGIN x noise (MARGIN = 16), plus the build's own term only at the entries
of _mp_pca_ref.FINDINGS.  Nothing is skipped.  tools/extremes_ratios.py prints the measured
error / noise as DESIGN.md section 7's second table.
"""
import numpy as np
import pytest
import torch

from oracle import gp_ref

import _mp_pca_ref as P

pytestmark = pytest.mark.gpu

EPS = P.EPS
MARGIN = P.MARGIN
FLOOR = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=dev)


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), \
        (what, float(np.max(np.abs(a - b))) if a.size else 0.0)


def _worst(e, nz):
    """max error / noise; 0 / 0 (an exact result where the truth is exactly representable and
    the noise ensemble never errs) counts as 0."""
    e, nz = np.asarray(e, dtype=float), np.asarray(nz, dtype=float)
    with np.errstate(all="ignore"):
        ratio = np.where(nz > 0, e / nz, np.where(e > 0, np.inf, 0.0))
    return float(np.max(ratio)) if ratio.size else 0.0


# ============================================================================= (a) statistics
SPLIT_NY = 1 << 16                     # blas.hip kSimStatsSplitNy
STAT_SHAPES = [(37, 1), (37, 63), (37, 1000), (1, 63), (2, 63), (3, 63), (5, 63),
               (3, SPLIT_NY + 3)]


def _device_stats(Y, floor, dev):
    from gladsgp_amd import blas
    Yd = _t(Y, dev)
    mu, sd = blas.sim_stats(Yd, floor)
    ys = blas.standardize(Yd, mu, sd)
    back = blas.standardize(ys, mu, sd, inverse=True)
    return tuple(a.cpu().numpy() for a in (mu, sd, ys, back))


def _stats_case(n, ny):
    """(Y, columns the truth is computed for): the whole ensemble when small, a spread of
    columns that reaches every block edge and all six kinds when ny is past the split."""
    Y = P.stats_ensemble(n, ny, FLOOR)
    if ny <= 1000:
        return Y, np.arange(ny)
    cols = np.unique(np.concatenate([np.arange(12), np.arange(250, 262), np.arange(ny - 12, ny),
                                     np.arange(SPLIT_NY - 6, SPLIT_NY + 3)]))
    return Y, cols


def stats_errors(dev, n, ny):
    """{quantity: (per-column error, per-column noise)} and the raw device arrays."""
    Y, cols = _stats_case(n, ny)
    mu, sd, ys, back = _device_stats(Y, FLOOR, dev)
    truth = P.stats(Y[:, cols], FLOOR)
    e_mu, e_sd, e_ys = P.stats_noise(Y[:, cols], FLOOR, truth)
    mu_t, sd_t, ys_t = truth
    err = {"mu": (np.abs((mu[cols] - mu_t.hi) - mu_t.lo), e_mu),
           "sd": (np.abs((sd[cols] - sd_t.hi) - sd_t.lo), e_sd),
           "y_std": (np.max(np.abs((ys[:, cols] - ys_t.hi) - ys_t.lo), axis=0), e_ys)}
    return err, dict(Y=Y, cols=cols, mu=mu, sd=sd, ys=ys, back=back, truth=truth)


@pytest.mark.parametrize("n,ny", STAT_SHAPES)
def test_stats_against_truth(dev, n, ny):
    """mu, sd and y_std within MARGIN x noise per column; a constant column's sd is the floor to
    the bit (and for n = 1 every column's); the inverse transform returns Y within the three
    roundings between them."""
    err, out = stats_errors(dev, n, ny)
    for q, (e, nz) in err.items():
        print(f"{q} n={n} ny={ny}: worst error / noise {_worst(e, nz):.3g}")
    for q, (e, nz) in err.items():
        bad = np.nonzero(~(e <= MARGIN * nz))[0]
        assert bad.size == 0, (q, n, ny, out["cols"][bad[:5]], e[bad[:5]], nz[bad[:5]])
    assert np.all(np.isfinite(out["mu"])) and np.all(np.isfinite(out["sd"]))
    assert np.all(np.isfinite(out["ys"]))
    kinds = np.arange(ny) % 6
    const = np.nonzero(kinds == P.STAT_KINDS.index("constant"))[0] if n > 1 else np.arange(ny)
    _bits_equal(out["sd"][const], np.full(const.size, FLOOR), ("floor", n, ny))
    assert np.all(out["sd"] >= FLOOR)
    # y_std = (y - mu)(1 + d1)(1 + d2) / sd and back = fma(y_std, sd, mu) = (y + (y - mu)(d1 + d2))
    # (1 + d3) with the device's own mu and sd, whatever their errors: eps |y - mu| + eps / 2 |y|
    Y = out["Y"]
    lim = EPS * (np.abs(Y - out["mu"]) + np.abs(Y))
    assert np.all(np.abs(out["back"] - Y) <= lim), (n, ny)


def test_stats_kernels_agree(dev):
    """The same columns (n = 3) through simstats_split_kernel (ny = 63) and simstats_kernel
    (ny = 65539, the columns tiled): both within MARGIN x noise of one truth, so of each other
    within twice that."""
    from gladsgp_amd import blas
    Y = P.stats_ensemble(3, 63, FLOOR)
    reps = -(-(SPLIT_NY + 3) // 63)
    wide = np.tile(Y, (1, reps))[:, : SPLIT_NY + 3]
    mu_s, sd_s = (a.cpu().numpy() for a in blas.sim_stats(_t(Y, dev), FLOOR))
    mu_w, sd_w = (a.cpu().numpy() for a in blas.sim_stats(_t(wide, dev), FLOOR))
    truth = P.stats(Y, FLOOR)
    e_mu, e_sd, _ = P.stats_noise(Y, FLOOR, truth)
    idx = np.arange(SPLIT_NY + 3) % 63
    for got, t, nz in ((mu_s, truth[0], e_mu), (sd_s, truth[1], e_sd)):
        assert np.all(np.abs((got - t.hi) - t.lo) <= MARGIN * nz)
    for got, t, nz in ((mu_w, truth[0], e_mu), (sd_w, truth[1], e_sd)):
        assert np.all(np.abs((got - t.hi[idx]) - t.lo[idx]) <= MARGIN * nz[idx])
    assert np.all(np.abs(mu_w - mu_s[idx]) <= 2 * MARGIN * e_mu[idx])
    assert np.all(np.abs(sd_w - sd_s[idx]) <= 2 * MARGIN * e_sd[idx])


@pytest.mark.parametrize("k", [-200, 200])
@pytest.mark.parametrize("n,ny", [(37, 63), (5, 63), (3, SPLIT_NY + 3)])
def test_stats_exact_scaling(dev, n, ny, k):
    """Y 2^k with the floor 2^k: mu 2^k and sd 2^k to the bit, y_std identical."""
    Y = P.stats_ensemble(n, ny, FLOOR)
    c = 2.0 ** k
    mu, sd, ys, _ = _device_stats(Y, FLOOR, dev)
    mu_c, sd_c, ys_c, _ = _device_stats(Y * c, FLOOR * c, dev)
    _bits_equal(mu_c, mu * c, ("mu", n, ny, k))
    _bits_equal(sd_c, sd * c, ("sd", n, ny, k))
    _bits_equal(ys_c, ys, ("y_std", n, ny, k))


def test_stats_single_row(dev):
    """n = 1: no sample deviation (numpy's ddof = 1 gives NaN); the build returns the floor, mu
    the row itself and y_std = 0 exactly (include/gpfit.h)."""
    Y = P.stats_ensemble(1, 63, FLOOR)
    mu, sd, ys, back = _device_stats(Y, FLOOR, dev)
    _bits_equal(mu, Y[0], "mu")
    _bits_equal(sd, np.full(63, FLOOR), "sd")
    assert np.all(ys == 0.0)
    _bits_equal(back, Y, "inverse")


# ============================================================================= (b) eigensolver
EIG_SIZES = (1, 2, 25, 64, 65)         # both kernels (LDS up to 64), odd and even r
MAX_SWEEPS = 30


def _syevj(A, dev, want_sqrt=False):
    from gladsgp_amd.blas import CM, syevj
    r = A.shape[0]
    W, V, sw = syevj(CM(_t(A, dev).contiguous(), r, r, r), max_sweeps=MAX_SWEEPS,
                     want_sqrt=want_sqrt)
    return W.cpu().numpy(), V.logical().cpu().numpy().copy(), int(sw[0])


_EIG = {}


def eig_run(dev, kind, r):
    if (kind, r) not in _EIG:
        _EIG[(kind, r)] = _syevj(P.eig_input(kind, r), dev)
    return _EIG[(kind, r)]


def eig_errors(dev, kind, r):
    """{measure: (device value, noise)} for eigenvalues, |V^T V - I| and |A V - V W|."""
    A = P.eig_input(kind, r)
    W, V, _ = eig_run(dev, kind, r)
    nz_w, nz_o, nz_r = P.eig_noise(kind, r)
    return {"W": (P.eig_truth(kind, r).err(W), nz_w),
            "VtV": (float(np.max(np.abs(V.T @ V - np.eye(r)))), nz_o),
            "AV": (P.eig_residual(A, W, V), nz_r)}


@pytest.mark.parametrize("r", EIG_SIZES)
@pytest.mark.parametrize("kind", P.EIG_KINDS)
def test_syevj_against_truth(dev, kind, r):
    W, V, sweeps = eig_run(dev, kind, r)
    errs = eig_errors(dev, kind, r)
    for q, (e, nz) in errs.items():
        print(f"{q} {kind} r={r}: {e:.3e} noise {nz:.3e} ratio {e / nz if nz else 0.0:.3g}")
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(V))
    for q, (e, nz) in errs.items():
        assert e <= MARGIN * nz, (q, kind, r, e, nz)
    assert np.all(W[:-1] >= W[1:]), (kind, r)
    assert sweeps < MAX_SWEEPS, (kind, r, sweeps)
    if kind in ("diagonal", "zero"):
        # nothing to rotate: the sorted diagonal to the bit, V a permutation, no sweep
        _bits_equal(W, np.sort(np.diag(P.eig_input(kind, r)))[::-1] + 0.0, (kind, r))
        assert sweeps == 0 and np.array_equal(np.sort(V, axis=0)[-1], np.ones(r))
        assert np.count_nonzero(V) == r
    if kind == "diagonal_tiny":
        # (1e-200)^2 is 0 at any normaliser: converged as given, the diagonal untouched
        _bits_equal(W, np.sort(np.diag(P.eig_input(kind, r)))[::-1] + 0.0, (kind, r))
        assert np.count_nonzero(V) == r
    if kind == "diagonal_tiny_live" and r >= 4:
        # a live pivot elsewhere keeps the sweeps going, so the (0, r-1) pivot is rotated:
        # theta^2 overflows, t = 0, c = 1, s = 0 -- rows 0 and r-1 of V stay unit vectors and
        # the two diagonal entries keep their bits
        assert sweeps > 0
        for i in (0, r - 1):
            assert np.count_nonzero(V[i]) == 1 and np.max(V[i]) == 1.0, (r, i)
            j = int(np.argmax(V[i]))
            assert W[j] == P.eig_input(kind, r)[i, i], (r, i)
    Ws, Vs, sw_s = _syevj(P.eig_input(kind, r), dev, want_sqrt=True)
    _bits_equal(Ws, np.sqrt(np.maximum(W, 0.0)), ("want_sqrt", kind, r))
    _bits_equal(Vs, V, ("want_sqrt V", kind, r))
    assert sw_s == sweeps


@pytest.mark.parametrize("k", [-100, 100, -600, 600])
@pytest.mark.parametrize("r", [25, 64, 65])
@pytest.mark.parametrize("kind", ["graded", "cluster", "indefinite"])
def test_syevj_exact_scaling(dev, kind, r, k):
    """A 2^k gives W 2^k, the same V and the same sweep count, bit for bit.  At k = +-600 every
    square of an entry is 0 or inf: the stop rule's sums are taken on entries normalised by a
    power of two from max|a| (eig.hip), so nothing is decided differently there -- without the
    normaliser the solve stopped at sweep 0 with diag(A) and V = I."""
    A = P.eig_input(kind, r)
    W, V, sweeps = eig_run(dev, kind, r)
    c = 2.0 ** k
    Wc, Vc, sw_c = _syevj(A * c, dev)
    assert sweeps > 0
    assert sw_c == sweeps, (kind, r, k, sw_c, sweeps)
    _bits_equal(Wc, W * c, ("W", kind, r, k))
    _bits_equal(Vc, V, ("V", kind, r, k))


# ========================================================================= (c) randomized SVD
_SVD = {}


def svd_run(dev, case):
    from gladsgp_amd.svd import randomized_svd
    if case not in _SVD:
        X, om, p, k, q = P.case_inputs(case)
        _SVD[case] = randomized_svd(np.array(X), p, k=k, q=q, omega=np.array(om), device=dev)
    return _SVD[case]


def svd_errors(dev, case):
    """{quantity: (error, noise, bound)} of one case: S at every entry; U, Vh over the
    identifiable triplets; the cluster projectors; U^T U - I; Vh Vh^T - I over the identifiable
    rows; the truncation residual against the truth's own."""
    X = P.case_inputs(case)[0]
    U, S, Vh = svd_run(dev, case)
    t = P.svd_truth(case)
    ident, clusters = P.classify(case)
    p = S.shape[0]
    eu, ev = P.vector_errors(U, Vh, t)
    out = {"S": (np.abs((S - t.S.hi) - t.S.lo), P.noise("S", case), P.limit("S", case)),
           "U": (eu[ident], P.noise("U", case)[ident], P.limit("U", case)[ident]),
           "Vh": (ev[ident], P.noise("Vh", case)[ident], P.limit("Vh", case)[ident])}
    for c, idx in enumerate(clusters):
        for nm, Z, T, rows in ((f"PU{c}", U, t.U, False), (f"PV{c}", Vh, t.Vh, True)):
            out[nm] = (P.projector_error(Z, T, idx, rows), P.noise(nm, case),
                       MARGIN * P.noise(nm, case))
    V = Vh[ident]
    scal = {"UtU": float(np.max(np.abs(U.T @ U - np.eye(p)))),
            "VVt": float(np.max(np.abs(V @ V.T - np.eye(len(ident))))),
            "resid": abs(P.residual(X, U, S, Vh) - t.resid)}
    for nm, e in scal.items():
        lim = P.limit(nm, case) if nm == "resid" else MARGIN * P.noise(nm, case)
        out[nm] = (e, P.noise(nm, case), lim)
    return out


@pytest.mark.parametrize("case", P.SVD_CASES)
def test_randomized_svd_against_truth(dev, case):
    U, S, Vh = svd_run(dev, case)
    X, om, p, k, q = P.case_inputs(case)
    assert U.shape == (X.shape[0], p) and S.shape == (p,) and Vh.shape == (p, X.shape[1])
    assert all(np.all(np.isfinite(a)) for a in (U, S, Vh))
    errs = svd_errors(dev, case)
    for nm, (e, nz, lim) in errs.items():
        print(f"{nm} {case}: worst error / noise {_worst(e, nz):.3g}, "
              f"{MARGIN * _worst(e, lim):.3g} against the bound's 16")
    for nm, (e, nz, lim) in errs.items():
        if case == "deficient" and nm == "UtU":
            continue                     # below: the zero singular values' vectors are completed
        assert np.all(np.asarray(e) <= lim), (nm, case, _worst(e, nz), _worst(e, lim))
    if case == "deficient":
        # S[8:] is zero in exact arithmetic; U stays orthonormal through the completion
        assert np.all(S[P.RANK_DEFICIENT:] <= MARGIN * P.noise("S", case)[P.RANK_DEFICIENT:])
        assert float(np.max(np.abs(U.T @ U - np.eye(p)))) <= 1e-10


def test_randomized_svd_float32_input(dev):
    """A float32 X is the fp64 run on the widened values, cast (d4)."""
    from gladsgp_amd.svd import randomized_svd
    X, om, p, k, q = P.case_inputs("d4")
    X32 = np.array(X, dtype=np.float32)
    got = randomized_svd(X32, p, k=k, q=q, omega=np.array(om), device=dev)
    ref = randomized_svd(X32.astype(np.float64), p, k=k, q=q, omega=np.array(om), device=dev)
    for g, r in zip(got, ref):
        assert g.dtype == np.float32 and r.dtype == np.float64
        np.testing.assert_array_equal(g, r.astype(np.float32))


# ======================================================================= (d) basis and weights
_CHAIN = {}


def weights_run(dev, regime):
    """standardize_y -> randomized_svd(y_std) -> pca_basis on the device outputs ->
    create_K_basis -> pc_weights, on the regime's ensemble given a mean and sd per column."""
    from gladsgp_amd import emulator
    from gladsgp_amd.svd import randomized_svd
    if regime not in _CHAIN:
        X, om, p, k, q = P.case_inputs(regime)
        n, ny = X.shape
        rng = np.random.default_rng(17)
        Y = X / np.std(X, ddof=1, axis=0) * rng.uniform(0.5, 20.0, ny) + rng.uniform(-50, 50, ny)
        data = emulator.EmulatorData(rng.random((n, 3)), Y, device=dev)
        data.standardize_y()
        ys = data.sim_data.y_std
        U, S, Vh = randomized_svd(ys, p, k=k, q=q, omega=torch.as_tensor(np.array(om)))
        K = gp_ref.pca_basis(S.cpu().numpy(), Vh.cpu().numpy(), p, n)
        data.create_K_basis(K)
        W, lam = emulator.pc_weights(data)
        torch.cuda.synchronize()
        _CHAIN[regime] = dict(y_std=ys.cpu().numpy().copy(), K=data.sim_data.K.cpu().numpy(),
                              w_hat=W.logical().cpu().numpy().copy(), lam=lam.cpu().numpy(),
                              S=S.cpu().numpy(), Vh=Vh.cpu().numpy(), n=n, p=p)
    return _CHAIN[regime]


def weights_errors(dev, regime):
    """{quantity: (per-PC error, per-PC noise)}: w_hat and LamSim against the 80-digit
    weights / diag(K K^T) of the device's own y_std and K."""
    c = weights_run(dev, regime)
    if "err" not in c:
        truth = P.weights(c["y_std"], c["K"])
        e_w, e_l = P.weights_noise(c["y_std"], c["K"], truth)
        w_t, lam_t = truth
        c["err"] = {"w_hat": (np.max(np.abs((c["w_hat"] - w_t.hi) - w_t.lo), axis=0), e_w),
                    "LamSim": (np.abs((c["lam"] - lam_t.hi) - lam_t.lo), e_l)}
    return c["err"]


@pytest.mark.parametrize("regime", ["d2", "d4", "d6"])
def test_basis_and_weights(dev, regime):
    c = weights_run(dev, regime)
    Kt = P.basis(c["S"], c["Vh"], c["p"], c["n"])
    assert Kt.err(c["K"]) <= 4 * EPS * Kt.scale()          # diag(S) Vh / sqrt(n): three roundings
    errs = weights_errors(dev, regime)
    for q, (e, nz) in errs.items():
        print(f"{q} {regime}: worst error / noise over the PCs {_worst(e, nz):.3g}")
    for q, (e, nz) in errs.items():
        assert np.all(e <= MARGIN * nz), (q, regime, _worst(e, nz))
