"""GPU: gp_xval (csrc/xval.hip) and EmulatorXvalPrediction against the numpy closed form
tests/_xval_ref.closed_form (itself checked against brute-force refits in test_xval_cpu.py), under
the project's oracle-parity bounds of test_gpu_kernels.py / test_gpu_res.py:
|mean - ref| <= 1e-8 max(1, max|ref|), |var - ref| <= 1e-9 s; plus the bit-level identities between
its forms, strided / offset layouts with sentinels, and the refused fold.
"""
import numpy as np
import pytest
import torch

import _layouts as L
import _xval_ref as ref
from oracle import gp_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x, dev, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype)


def _factor(dev, n, d, batch):
    """(problems, Cholesky, w (batch, n), shift (batch,)) of problems 0 .. batch - 1 on the
    device: Gram and L^-1 by the project's own kernels."""
    from gladsgp_amd import kernels
    ps = [ref.problem(n, d, b) for b in range(batch)]
    G = kernels.gram(_t(ps[0]["X"], dev), _t(np.stack([p["beta"] for p in ps]), dev),
                     _t(np.array([p["s"] for p in ps]), dev),
                     _t(np.array([p["delta"] for p in ps]), dev), batch=batch)
    ch = kernels.cholesky_inverse(G)
    ch.check()
    return (ps, ch, _t(np.stack([p["w"] for p in ps]), dev),
            _t(np.array([p["shift"] for p in ps]), dev))


def _within(mean, var, n, d, folds, batch):
    for b in range(batch):
        rm, rv = ref.reference(n, d, b, ref.key(folds))
        cov = ~np.isnan(rm)
        assert np.array_equal(np.isnan(mean[b]), ~cov) and np.array_equal(np.isnan(var[b]), ~cov)
        em = np.max(np.abs(mean[b][cov] - rm[cov]))
        ev = np.max(np.abs(var[b][cov] - rv[cov]))
        print(f"n={n} b={b} mean err {em:.3e} var err {ev:.3e}")
        assert em <= 1e-8 * max(1.0, np.max(np.abs(rm[cov]))), (b, em)
        assert ev <= 1e-9 * ref.problem(n, d, b)["s"], (b, ev)


def _bits(a, b):
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))


def _d(n):
    return 8 if n >= 128 else 3


@pytest.mark.parametrize("n", [1, 2, 17, 128, 129, 200, 513])
def test_leave_one_out(dev, n):
    """One tile, a tile edge, padding rows, npad = 640; three problems with their own beta, s and
    delta."""
    from gladsgp_amd import kernels
    _, ch, w, shift = _factor(dev, n, _d(n), 3)
    mean, var = kernels.xval(ch, w, None, shift)
    _within(mean.cpu().numpy(), var.cpu().numpy(), n, _d(n), None, 3)


@pytest.mark.parametrize("n", [200, 513])
def test_folds(dev, n):
    """Folds of 1, 2, 15, 16, 17, 63 and 64 indices, sorted and not; the uncovered outputs keep
    the caller's sentinel."""
    from gladsgp_amd import kernels
    folds = ref.mixed_folds(n)
    _, ch, w, shift = _factor(dev, n, 8, 2)
    out = tuple(torch.full((2, n), -7.25, dtype=torch.float64, device=dev) for _ in range(2))
    mean, var = kernels.xval(ch, w, folds, shift, out=out)
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    cov = np.zeros(n, bool)
    cov[[i for F in folds for i in F]] = True
    assert (mean[:, ~cov] == -7.25).all() and (var[:, ~cov] == -7.25).all()
    mean[:, ~cov] = np.nan
    var[:, ~cov] = np.nan
    _within(mean, var, n, 8, folds, 2)


def test_null_form_equals_singleton_folds(dev):
    from gladsgp_amd import kernels
    n = 200
    _, ch, w, shift = _factor(dev, n, 8, 2)
    a = kernels.xval(ch, w, None, shift)
    b = kernels.xval(ch, w, [[i] for i in np.random.default_rng(1).permutation(n)], shift)
    _bits(a[0], b[0])
    _bits(a[1], b[1])


@pytest.mark.parametrize("n", [1, 17, 129, 513])
def test_leave_one_out_residual_is_alpha_times_var(dev, n):
    """gp_xval's leave-one-out form and gp_alpha walk the columns of L^-1 with one routine: with
    al_i = sum_k L^-1[k,i] z_k and q_i = sum_k L^-1[k,i]^2, mean = fl(w - fl(al / q)),
    var = fl(1 / q) (no shift) and alpha = al with the same bits, so with u = 2^-53
    |fl(w - mean) - fl(alpha var)| <= u (|mean| + |w - mean|) + 4 u |al / q|.  One row, a partial
    16-row tile, an odd n across the 128-row stride, several strides; three problems."""
    from gladsgp_amd import kernels
    _, ch, w, _ = _factor(dev, n, _d(n), 3)
    mean, var = kernels.xval(ch, w, None, None)
    al = kernels.alpha(ch, w)
    w, mean, var, al = (t.cpu().numpy() for t in (w, mean, var, al))
    err = np.abs((w - mean) - al * var)
    bound = 2.0 ** -52 * (np.abs(mean) + 8 * np.abs(al * var))
    print(f"n={n} max err {err.max():.3e} min slack {(bound - err).min():.3e}")
    assert np.isfinite(mean).all() and np.isfinite(var).all() and np.isfinite(al).all()
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]


def test_upper_triangle_is_never_read(dev):
    """An L^-1 whose strict upper triangle holds 1e300 gives the bits of the zeroed one, for
    leave-one-out and for folds."""
    from gladsgp_amd import kernels
    n = 200
    folds = ref.mixed_folds(n)
    _, ch, w, shift = _factor(dev, n, 8, 2)
    npad = ch.linv_buf.shape[1]
    dirty = ch.linv_buf.clone()
    r = torch.arange(npad, device=dev)
    dirty[:, r[:, None] > r[None, :]] = 1e300          # memory order [b, column, row]: row < column
    assert float(dirty[0, 5, 3]) == 1e300 and float(dirty[0, 3, 5]) == float(ch.linv_buf[0, 3, 5])
    ch2 = kernels.Cholesky(n, ch.a_buf, dirty, ch.info, ch.logdet)
    for f in (None, folds):
        a = kernels.xval(ch, w, f, shift)
        b = kernels.xval(ch2, w, f, shift)
        _bits(a[0], b[0])
        _bits(a[1], b[1])


def test_shift(dev):
    """shift=None equals a zeros tensor bit for bit; with a shift the variance is that minus the
    shift, rounded once."""
    from gladsgp_amd import kernels
    n = 129
    folds = [[3, 70, 128], [5], list(range(20, 60))]
    _, ch, w, shift = _factor(dev, n, 8, 2)
    for f in (None, folds):
        a = kernels.xval(ch, w, f, None)
        b = kernels.xval(ch, w, f, torch.zeros(2, dtype=torch.float64, device=dev))
        c = kernels.xval(ch, w, f, shift)
        _bits(a[0], b[0])
        _bits(a[1], b[1])
        _bits(a[0], c[0])
        v0, v1 = a[1].cpu().numpy(), c[1].cpu().numpy()
        cov = ~np.isnan(v0)
        want = v0 - shift.cpu().numpy()[:, None]
        assert (np.abs(v1 - want)[cov] <= np.spacing(np.abs(v1))[cov]).all()


def _raw(dev, ch, w, folds, shift, Li=None, We=None, Me=None, Ve=None, info=True):
    """gp_xval through ctypes with explicit layouts; returns (rc, info array or None)."""
    from gladsgp_amd import _capi
    lib = _capi.lib()
    n, batch = ch.n, ch.linv_buf.shape[0]
    npad = ch.linv_buf.shape[1]
    if folds is None:
        ptr = idx = None
        nfolds = nidx = 0
    else:
        ptr = _t(np.cumsum([0] + [len(F) for F in folds]), dev, torch.int32)
        idx = _t(np.concatenate([np.asarray(F, dtype=np.int64) for F in folds]), dev, torch.int32)
        nfolds, nidx = len(folds), int(idx.numel())
    inf = torch.full((batch,), 77, dtype=torch.int32, device=dev) if info else None
    nbytes = lib.gp_xval_ws_bytes(n, nfolds, nidx, batch)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    rc = lib.gp_xval(Li.ptr if Li else ch.linv_buf.data_ptr(), Li.ld if Li else npad,
                     Li.stride if Li else npad * npad, n, We.ptr if We else w.data_ptr(),
                     We.stride if We else n, ptr.data_ptr() if ptr is not None else None,
                     idx.data_ptr() if idx is not None else None, nfolds, nidx,
                     shift.data_ptr() if shift is not None else None, Me.ptr, Ve.ptr, Me.stride,
                     inf.data_ptr() if info else None, batch, ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, (inf.cpu().numpy() if info else None)


@pytest.mark.parametrize("case", ["odd_ld", "off8", "gap16"])
@pytest.mark.parametrize("form", ["loo", "folds"])
def test_layouts(dev, case, form):
    """Strided, offset and gapped L^-1, w_hat, mean and var: the bits of the tight call, nothing
    outside the covered outputs written, no padding read (the sentinels are NaN)."""
    n, batch = 200, 2
    folds = None if form == "loo" else ref.mixed_folds(n)
    _, ch, w, shift = _factor(dev, n, 8, batch)
    tight = [L.blank((batch, 1, n), device=dev) for _ in range(2)]
    rc, info = _raw(dev, ch, w, folds, shift, Me=tight[0], Ve=tight[1])
    assert rc == 0 and (info == 0).all()
    Li = L.place(ch.linv_buf.cpu().numpy(), case, device=dev)
    We = L.place(w.cpu().numpy()[:, None, :], case, device=dev)
    Me, Ve = (L.blank_case((batch, 1, n), case, device=dev) for _ in range(2))
    rc, info = _raw(dev, ch, w, folds, shift, Li, We, Me, Ve)
    assert rc == 0 and (info == 0).all()
    cov = np.zeros(n, bool)
    cov[list(range(n)) if folds is None else [i for F in folds for i in F]] = True
    written = np.broadcast_to(cov, (batch, 1, n))
    for e, t in ((Me, tight[0]), (Ve, tight[1])):
        e.check(written)
        got, want = e.extract(finite=False), t.extract(finite=False)
        assert np.isfinite(got[written]).all()
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    Li.check(False)
    We.check(False)
    _within(np.where(cov, Me.extract(False)[:, 0], np.nan),
            np.where(cov, Ve.extract(False)[:, 0], np.nan), n, 8, folds, batch)


def test_fold_of_65_is_refused_by_the_library(dev):
    """Handed straight to the C entry point, a fold of 65 indices (and one with an index out of
    range) gives info = -2 and touches no output; the valid fold beside them is produced."""
    n, batch = 200, 2
    _, ch, w, shift = _factor(dev, n, 8, batch)
    Me, Ve = (L.blank((batch, 1, n), device=dev) for _ in range(2))
    rc, info = _raw(dev, ch, w, [list(range(65))], shift, Me=Me, Ve=Ve)
    assert rc == 0 and (info == -2).all()
    Me.check(False)
    Ve.check(False)
    folds = [list(range(100, 165)), [3, n], [n + 5], [7, 9, 11]]
    rc, info = _raw(dev, ch, w, folds, shift, Me=Me, Ve=Ve)
    assert rc == 0 and (info == -2).all()
    written = np.zeros((batch, 1, n), bool)
    written[:, :, [7, 9, 11]] = True
    Me.check(written)
    Ve.check(written)
    _within(np.where(written[:, 0], Me.extract(False)[:, 0], np.nan),
            np.where(written[:, 0], Ve.extract(False)[:, 0], np.nan), n, 8, [[7, 9, 11]], batch)


def test_not_positive_definite_fold_is_reported(dev):
    """A column zeroed from its diagonal down makes Q_FF of the fold through it singular:
    info = that fold + 1, its outputs NaN, the other folds produced (their variances, which do
    not depend on z, bit for bit as before)."""
    from gladsgp_amd import kernels
    n = 129
    folds = [[0, 1], [100, 101, 102], [120], [128, 127]]
    _, ch, w, shift = _factor(dev, n, 8, 1)
    good = kernels.xval(ch, w, folds, shift)
    bad = ch.linv_buf.clone()
    bad[0, 101, 101:] = 0.0                             # column 101, from its diagonal down
    ch2 = kernels.Cholesky(n, ch.a_buf, bad, ch.info, ch.logdet)
    with pytest.raises(kernels.XvalNotPositiveDefinite, match=r"\[2\]"):
        kernels.xval(ch2, w, folds, shift)
    mean, var = kernels.xval(ch2, w, folds, shift, check=False)
    mean, var, v0 = mean.cpu().numpy()[0], var.cpu().numpy()[0], good[1].cpu().numpy()[0]
    assert np.isnan(mean[[100, 101, 102]]).all() and np.isnan(var[[100, 101, 102]]).all()
    rest = [0, 1, 120, 127, 128]
    assert np.isfinite(mean[rest]).all()
    assert np.array_equal(var[rest], v0[rest])


def test_n33_against_refits(dev):
    """Directly against brute-force refits (oracle.gp_ref.predict on the reduced design)."""
    from gladsgp_amd import kernels
    n = 33
    ps, ch, w, shift = _factor(dev, n, 3, 1)
    p = ps[0]
    for folds in (None, [list(range(9, 25))]):
        mean, var = kernels.xval(ch, w, folds, shift)
        rm, rv = ref.brute_force(p["X"], p["w"], p["beta"], p["s"], p["delta"], p["s_pred"], folds)
        cov = ~np.isnan(rm)
        mean, var = mean.cpu().numpy()[0], var.cpu().numpy()[0]
        assert np.array_equal(np.isnan(mean), ~cov)
        assert np.max(np.abs(mean[cov] - rm[cov])) <= 1e-8 * max(1.0, np.max(np.abs(rm[cov])))
        assert np.max(np.abs(var[cov] - rv[cov])) <= 1e-9 * p["s"]


# --------------------------------------------------------------------------- emulator level
def _ensemble(n=40, ny=50, d=3, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.random((n, d))
    modes = rng.standard_normal((4, ny)) * (0.5 ** np.arange(4))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + k) for k in range(4)], 1)
    y = (3.0 + coef @ modes + 1e-2 * rng.standard_normal((n, ny))).astype(np.float32)
    return t.astype(np.float32), y


def _samples(S, d, P, seed=1):
    rng = np.random.default_rng(seed)
    return {"betaU": rng.uniform(0.2, 3.0, (S, (d + 1) * P)),
            "lamUz": rng.uniform(0.5, 3.0, (S, P)),
            "lamWs": rng.uniform(200, 3000, (S, P)),
            "lamWOs": rng.uniform(50, 500, (S, 1))}


FOLDS = [[0, 5, 7], [1], list(range(20, 36))]


@pytest.fixture(scope="module")
def xmodel(dev, tmp_path_factory):
    from gladsgp_amd import model as gm
    t, y = _ensemble()
    _, model = gm.init_model(t, y, "xval", 3, data_dir=str(tmp_path_factory.mktemp("d")),
                             device=dev, verbose=False)
    return model, _samples(2, 3, 3)


def test_emulator_folds_match_refits_through_predict_units(dev, xmodel):
    from gladsgp_amd import emulator as em
    model, samples = xmodel
    S, P, n = 2, 3, model.n
    xv = em.EmulatorXvalPrediction(leave_out_inds=FOLDS, model=model, samples=samples)
    assert (xv.S, xv.m, xv.P) == (S, n, P)
    mean, var = xv.mean, xv.var
    assert mean.shape == var.shape == xv.w.shape == (S, n, P)
    cov = np.zeros(n, bool)
    cov[[i for F in FOLDS for i in F]] = True
    assert np.isnan(mean[:, ~cov]).all() and np.isnan(var[:, ~cov]).all()
    assert np.isfinite(mean[:, cov]).all() and np.isfinite(var[:, cov]).all()
    beta, s, delta, sp = em.gp_params(samples, em._np(model.LamSim), model.d, P, True)
    X = model.data.sim_data.t_dev
    w_hat = model.w_hat.transpose(0, 1).contiguous()           # (P, n)
    for F in FOLDS:
        rest = torch.as_tensor(np.setdiff1d(np.arange(n), F), device=dev)
        Fi = torch.as_tensor(np.asarray(F), device=dev)
        m_r, v_r = em.predict_units(X[rest].contiguous(), X[Fi].contiguous(),
                                    w_hat[:, rest].repeat(S, 1).contiguous(),
                                    _t(beta.reshape(S * P, -1), dev), _t(s.reshape(-1), dev),
                                    _t(delta.reshape(-1), dev), _t(sp.reshape(-1), dev))
        m_r = m_r.cpu().numpy().reshape(S, P, len(F)).transpose(0, 2, 1)
        v_r = v_r.cpu().numpy().reshape(S, P, len(F)).transpose(0, 2, 1)
        assert np.max(np.abs(mean[:, F] - m_r)) <= 1e-8 * max(1.0, np.max(np.abs(m_r)))
        assert (np.abs(var[:, F] - v_r) <= 1e-9 * s[:, None, :]).all()
    # the PC-space diagnostic, from its definition
    shift = (s + delta - sp)[:, None, :]
    want = (model.w_hat.cpu().numpy()[None] - mean) / np.sqrt(var + shift)
    got = xv.standardized_residuals
    assert got.shape == (S, n, P)
    np.testing.assert_allclose(got[:, cov], want[:, cov], rtol=1e-12, atol=0)
    assert np.isnan(got[:, ~cov]).all()


def test_emulator_default_is_leave_one_out(dev, xmodel):
    from gladsgp_amd import emulator as em
    model, samples = xmodel
    assert em.SepiaXvalEmulatorPrediction is em.EmulatorXvalPrediction
    xv = em.SepiaXvalEmulatorPrediction(model=model, samples=samples)
    assert isinstance(xv, em.EmulatorPrediction)
    assert np.isfinite(xv.mean).all() and np.isfinite(xv.var).all() and (xv.var > 0).all()
    ex = em.EmulatorXvalPrediction([[i] for i in range(model.n)], model=model, samples=samples,
                                   group=4)
    np.testing.assert_allclose(ex.mean, xv.mean, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ex.var, xv.var, rtol=0, atol=1e-10)
    sd_ = model.data.sim_data
    xv.w = xv.w.astype(np.float32)
    y = xv.get_y()
    assert y.dtype == np.float32 and y.shape == (2, model.n, sd_.K.shape[1])
    want = gp_ref.reconstruct_y(xv.w.astype(np.float64), sd_.K.cpu().numpy(),
                                sd_.y_mean.cpu().numpy(), sd_.y_sd.cpu().numpy())
    assert np.max(np.abs(y - want)) <= 2.0 ** -23 * np.max(np.abs(want))
    # without the error draws the band is the samples' own spread, which brackets their mean
    mean, lo, hi = xv.summary(0.025, add_error=False)
    assert mean.shape == lo.shape == hi.shape == (model.n, sd_.K.shape[1])
    assert (lo <= mean).all() and (mean <= hi).all()
    assert xv.sample_w(seed=3).shape == (2, model.n, 3)
    assert xv.error_draws(np.random.default_rng(0)).shape == (2, model.n)


def test_emulator_refuses_a_context(xmodel):
    from gladsgp_amd import emulator as em
    model, samples = xmodel
    with pytest.raises(ValueError, match="ctx"):
        em.EmulatorXvalPrediction(model=model, samples=samples, ctx=object())
