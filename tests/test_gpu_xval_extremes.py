"""gp_xval (csrc/xval.hip) on the device against a 50-digit truth, at the hyperparameter extremes
of tests/_mp_ref.py and on fold plans made for the kernel's edges (tests/_mp_xval_ref.py: the
truths, the noise, the plans).  Three quantities: xmean, xvar (shift = s + delta - s_pred) and
xq (no shift: 1/q, diag Q_FF^-1), each held to MARGIN = 16 times what fp64 itself delivers.

(a) the chain: gp_gram_ardse -> gp_potrf_inv -> gp_xval against the chain truth; the
    whole-design folds besides against the prior itself (mean 0, variance s_pred);
(b) the kernel alone: a hand-built factor holding the truth's L^-1 rounded to fp64, NaN in its
    strict upper triangle and padding, against the 50-digit result *of that array*; then the
    same with the L^-1 the device produced in (a).  This sets the factorisation's error aside;
(c) bit identities: alone = inside the batch of 4, folds listed in reverse, singleton folds =
    leave-one-out, a repeated call;
(d) exact scaling on the hand-built factor: w -> 2^(+-300) w and L^-1 -> 2^(-+100) L^-1 with
    shift -> 4^(+-100) shift.  These are the exponents the issue aims for; the CPU condition
    (tests/test_mp_xval_ref_cpu.py, _mp_xval_ref.magnitudes) allows them in every case: every
    leaf and product term of the kernels stays inside [2^-960, 2^960], the nearest being the
    sharp regime's L^-1, which would allow 313.

The four d = 8 regimes share X and run as one batch of 4; grid, d12, d32 run alone.  Every case
asserts info = 0 (kernels.xval raises otherwise); nothing is skipped.  tools/extremes_ratios.py
xval prints the measured error / noise of (a) and (b) as DESIGN.md section 7's table.

Measured on an MI355X (2026-10-21, 622 tests, this file alone): 38 s wall, nearly all of it the
50-digit truths and the fp64 ensembles on the host; slowest test test_chain[mid-130-loo], 3.8 s
(it is the first to need the n = 130 factorisation at 65 digits; 2.2 s for the next slowest).

Chain-layer findings: on the 1-D grid from n = 64 on the chain is above
16 x noise (up to 71 x) at the entries of _mp_xval_ref.FINDINGS and is held there to 16 x (noise
+ the explicit-inverse term of the factorisation).  The kernel alone is within 3.3 x noise of
its own truth everywhere, so gp_xval adds nothing to what L^-1 carries.
"""
import numpy as np
import pytest
import torch

import _mp_ref as M
import _mp_xval_ref as X

pytestmark = pytest.mark.gpu

MARGIN = M.MARGIN
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.as_tensor(np.array(x, dtype=np.float64, order="C"), device=dev)   # a copy


def _problems(group, n):
    return [M.problem(r, n) for r in M.GROUPS[group]]


def _xval(ch, W, folds, shift, dev):
    """{xmean, xvar, xq} as (batch, n) numpy: one call with the shift and one without, both into
    sentinel-filled outputs; info = 0 (``check`` raises otherwise); the mean does not depend on
    the shift."""
    from gladsgp_amd import kernels
    B, n = W.shape
    outs = []
    for sh in (shift, None):
        out = tuple(torch.full((B, n), SENTINEL, dtype=torch.float64, device=dev)
                    for _ in range(2))
        mean, var = kernels.xval(ch, W, folds, sh, out=out, check=True)
        outs.append((mean.cpu().numpy(), var.cpu().numpy()))
    assert np.array_equal(outs[0][0].view(np.int64), outs[1][0].view(np.int64))
    return {"xmean": outs[0][0], "xvar": outs[0][1], "xq": outs[1][1]}


def _hand_built(Linv, dev):
    """A kernels.Cholesky around a given L^-1 (batch, n, n) logical [b][i][j]: linv_buf
    (batch, npad, npad) column-major as the class documents, NaN in the strict upper triangle
    and in the padding (the kernel promises neither reaches a result, and its 16-B loads at odd
    n do read row n); a_buf, info, logdet are dummies."""
    from gladsgp_amd import kernels
    Linv = np.asarray(Linv, dtype=np.float64)
    B, n, _ = Linv.shape
    npad = kernels.padded_n(n)
    assert npad == 128 * ((n + 127) // 128)
    buf = np.full((B, npad, npad), np.nan)
    col, row = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    buf[:, :n, :n] = np.where(row >= col, np.transpose(Linv, (0, 2, 1)), np.nan)
    return kernels.Cholesky(n, torch.zeros((B, n, n), dtype=torch.float64, device=dev),
                            _t(buf, dev), torch.zeros(B, dtype=torch.int32, device=dev),
                            torch.zeros(B, dtype=torch.float64, device=dev))


_FACTOR, _RUNS = {}, {}


def _factor(group, n, dev):
    """The device's own factor of one regime group at one size, once per module: (Cholesky, its
    L^-1 downloaded (batch, n, n), W, shift)."""
    from gladsgp_amd import kernels
    if (group, n) not in _FACTOR:
        ps = _problems(group, n)
        G = kernels.gram(_t(ps[0].X, dev), _t(np.stack([p.beta for p in ps]), dev),
                         _t([p.s for p in ps], dev), _t([p.delta for p in ps], dev),
                         batch=len(ps))
        ch = kernels.cholesky_inverse(G)
        assert ch.info.cpu().tolist() == [0] * len(ps)
        _FACTOR[(group, n)] = (ch, ch.Linv.cpu().numpy().copy(),
                               _t(np.stack([p.w for p in ps]), dev),
                               _t([X.shift_of(p) for p in ps], dev))
    return _FACTOR[(group, n)]


def _truth_factor(group, n, dev):
    key = ("hi", group, n)
    if key not in _FACTOR:
        hi = np.stack([M.truth_of(r, n).Linv.hi for r in M.GROUPS[group]])
        _FACTOR[key] = _hand_built(hi, dev)
    return _FACTOR[key]


def _run(layer, group, n, plan, dev):
    """Outputs of one layer for one (group, n, plan), once per module.  Layers: ``chain`` (the
    device's factor as it stands), ``hi`` (hand-built from the truth's L^-1), ``dev`` (hand-built
    from the device's L^-1)."""
    key = (layer, group, n, plan)
    if key not in _RUNS:
        ch, Ldev, W, shift = _factor(group, n, dev)
        if layer == "hi":
            ch = _truth_factor(group, n, dev)
        elif layer == "dev":
            ch = _hand_built(Ldev, dev)
        _RUNS[key] = _xval(ch, W, X.folds_of(n, plan), shift, dev)
    return _RUNS[key]


def _sentinels_kept(out, n, plan):
    un = np.setdiff1d(np.arange(n), X.covered(X.folds_of(n, plan), n))
    for q in X.QUANTITIES:
        assert (out[q][:, un] == SENTINEL).all(), q


def xval_errors(dev, regime, n, plan):
    """{layer: {quantity: (error, noise, limit)}} of one case (tools/extremes_ratios.py makes
    DESIGN.md's table from this).  The ``dev`` layer's truth and noise are those of the L^-1 the
    device produced."""
    group = M.group_of(regime)
    b = M.GROUPS[group].index(regime)
    p = M.problem(regime, n)
    folds = X.folds_of(n, plan)
    res = {}
    ct = X.chain_truth(regime, n, plan)
    out = _run("chain", group, n, plan, dev)
    res["chain"] = {q: (ct.err(q, out[q][b]), X.chain_noise(q, regime, n, plan),
                        X.chain_limit(q, regime, n, plan)) for q in X.QUANTITIES}
    kt, kn = X.kernel_truth_hi(regime, n, plan), X.kernel_noise_hi(regime, n, plan)
    out = _run("hi", group, n, plan, dev)
    res["hi"] = {q: (kt.err(q, out[q][b]), kn[q], MARGIN * kn[q]) for q in X.QUANTITIES}
    Ldev = _factor(group, n, dev)[1][b]
    kt = X.kernel_truth(Ldev, p.w, folds, X.shift_of(p))
    kn = X.kernel_noise(Ldev, p.w, folds, X.shift_of(p), kt, p)
    out = _run("dev", group, n, plan, dev)
    res["dev"] = {q: (kt.err(q, out[q][b]), kn[q], MARGIN * kn[q]) for q in X.QUANTITIES}
    return res


_ERRORS = {}


def _errors(dev, regime, n, plan):
    key = (regime, n, plan)
    if key not in _ERRORS:
        _ERRORS[key] = xval_errors(dev, regime, n, plan)
    return _ERRORS[key]


def _held(dev, layer, regime, n, plan):
    errs = _errors(dev, regime, n, plan)[layer]
    for q, (err, nz, lim) in errs.items():
        print(f"{layer} {q} {regime} n={n} {plan}: err {err:.3e} noise {nz:.3e} "
              f"ratio {err / nz:.3g}, {MARGIN * err / lim:.3g} against the bound's 16")
    for q, (err, nz, lim) in errs.items():
        assert err <= lim, (layer, q, regime, n, plan, err / nz, MARGIN * err / lim)


# ========================================================================== (a) the chain
@pytest.mark.parametrize("regime,n,plan", X.REGIME_CASES)
def test_chain(dev, regime, n, plan):
    """Gram -> factorisation -> gp_xval: xmean, xvar and xq within MARGIN x the chain noise of
    the chain truth (plus the explicit-inverse term at _mp_xval_ref.FINDINGS); uncovered outputs
    keep the caller's sentinel."""
    group = M.group_of(regime)
    _sentinels_kept(_run("chain", group, n, plan, dev), n, plan)
    _held(dev, "chain", regime, n, plan)


@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("n,plan", [(1, "loo"), (1, "one"), (5, "whole"), (64, "whole")])
def test_chain_gives_the_prior(dev, regime, n, plan):
    """The fold that is the whole design, through T = 1 and T = 4: held to the same limit around
    the prior itself, mean 0 and variance s_pred.  mean = w - Q^-1 (Q w) is the heaviest
    cancellation the closed form has."""
    group = M.group_of(regime)
    b = M.GROUPS[group].index(regime)
    p = M.problem(regime, n)
    out = _run("chain", group, n, plan, dev)
    em = float(np.max(np.abs(out["xmean"][b])))
    ev = float(np.max(np.abs(out["xvar"][b] - p.s_pred)))
    lm, lv = (X.chain_limit(q, regime, n, plan) for q in ("xmean", "xvar"))
    print(f"prior {regime} n={n} {plan}: |mean| {em:.3e} (limit {lm:.3e}) "
          f"|var - s_pred| {ev:.3e} (limit {lv:.3e})")
    assert em <= lm and ev <= lv


# ==================================================================== (b) the kernel alone
@pytest.mark.parametrize("regime,n,plan", X.REGIME_CASES)
def test_kernel_on_the_truths_factor(dev, regime, n, plan):
    """The hand-built factor of truth.Linv.hi against the 50-digit result of that fp64 array."""
    _sentinels_kept(_run("hi", M.group_of(regime), n, plan, dev), n, plan)
    _held(dev, "hi", regime, n, plan)


@pytest.mark.parametrize("regime,n,plan", X.REGIME_CASES)
def test_kernel_on_the_devices_factor(dev, regime, n, plan):
    """The L^-1 the device produced in the chain, downloaded and hand-built again, against its
    own kernel truth: gp_xval's error without the factorisation's.  On a zero-padded and on a
    NaN-padded buffer of the same L^-1 the bits agree."""
    group = M.group_of(regime)
    a, b = _run("chain", group, n, plan, dev), _run("dev", group, n, plan, dev)
    for q in X.QUANTITIES:
        assert np.array_equal(a[q].view(np.int64), b[q].view(np.int64)), q
    _held(dev, "dev", regime, n, plan)


# ======================================================================== (c) bit identities
def _same(a, b, what):
    for q in X.QUANTITIES:
        assert np.array_equal(a[q].view(np.int64), b[q].view(np.int64)), \
            (what, q, float(np.nanmax(np.abs(a[q] - b[q]))))


@pytest.mark.parametrize("group,n,plan", X.CASES)
def test_bit_identities(dev, group, n, plan):
    """On the hand-built factor: a problem alone = the same problem inside its batch; the plan =
    the plan with its folds listed in reverse; its singleton folds = leave-one-out at those
    indices; a repeated call."""
    ch = _truth_factor(group, n, dev)
    _, _, W, shift = _factor(group, n, dev)
    folds = X.folds_of(n, plan)
    base = _run("hi", group, n, plan, dev)
    _same(_xval(ch, W, folds, shift, dev), base, "repeat")
    rev = [[i] for i in range(n)][::-1] if folds is None else folds[::-1]
    _same(_xval(ch, W, rev, shift, dev), base, "reversed")
    single = [F[0] for F in X.listed(folds, n) if len(F) == 1]
    if single and folds is not None:
        loo = _run("hi", group, n, "loo", dev)
        for q in X.QUANTITIES:
            assert np.array_equal(base[q][:, single].view(np.int64),
                                  loo[q][:, single].view(np.int64)), q
    hi = np.stack([M.truth_of(r, n).Linv.hi for r in M.GROUPS[group]])
    for b in range(len(M.GROUPS[group])):
        alone = _xval(_hand_built(hi[b:b + 1], dev), W[b:b + 1].contiguous(), folds,
                      shift[b:b + 1].contiguous(), dev)
        _same(alone, {q: base[q][b:b + 1] for q in X.QUANTITIES}, ("alone", b))


# ========================================================================== (d) exact scaling
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("group,n,plan", X.CASES)
def test_exact_scaling(dev, group, n, plan, sign):
    """w -> 2^k w (k = +-300): xmean times 2^k exactly, the xvar and xq bits unchanged.
    L^-1 -> 2^-k L^-1 with shift -> 4^k shift (k = +-100): the xmean bits unchanged, xvar and xq
    times 4^k exactly.  No absolute threshold anywhere in the kernels."""
    _, _, W, shift = _factor(group, n, dev)
    folds = X.folds_of(n, plan)
    base = _run("hi", group, n, plan, dev)
    cov = X.covered(folds, n)
    hi = np.stack([M.truth_of(r, n).Linv.hi for r in M.GROUPS[group]])

    def same(got, want, what):
        assert np.array_equal(got[:, cov].view(np.int64), want[:, cov].view(np.int64)), what

    k = sign * X.K_W
    got = _xval(_truth_factor(group, n, dev), W * 2.0 ** k, folds, shift, dev)
    same(got["xmean"], base["xmean"] * 2.0 ** k, ("w", k, "xmean"))
    same(got["xvar"], base["xvar"], ("w", k, "xvar"))
    same(got["xq"], base["xq"], ("w", k, "xq"))
    k = sign * X.K_LINV
    got = _xval(_hand_built(hi * 2.0 ** -k, dev), W, folds, shift * 4.0 ** k, dev)
    same(got["xmean"], base["xmean"], ("Linv", k, "xmean"))
    same(got["xvar"], base["xvar"] * 4.0 ** k, ("Linv", k, "xvar"))
    same(got["xq"], base["xq"] * 4.0 ** k, ("Linv", k, "xq"))
    assert np.all(np.isfinite(base["xmean"][:, cov])) and np.all(base["xq"][:, cov] > 0.0)
