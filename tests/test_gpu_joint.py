"""GPU: gp_predict_cov / gp_mvn_draw (csrc/jointcov.hip) and EmulatorPrediction(realize="joint")
against the numpy closed form tests/_joint_ref.closed_form (itself checked against brute-force
conditioning and a 50-digit truth in test_joint_cpu.py), under the project's variance parity
bound |C - ref| <= 1e-9 s (test_gpu_xval.py, test_gpu_kernels.py); plus the bit-level identities
(symmetry, batching, layouts, masking, graph replay, split batches of draws), the draws against
the numpy restatement of the normal stream, their moments, and the non-positive-definite exit.
"""
import numpy as np
import pytest
import torch

import _joint_ref as ref
import _layouts as L
import _xval_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x, dev, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype)


def _bits(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def _setup(dev, n, m, d, batch=3, Xs=None, nugget=True):
    """Problems 0 .. batch - 1 of _xval_ref on the device, factorised by the project's own
    kernels; o["args"] are predict_cov's arguments after the factorisation."""
    from gladsgp_amd import kernels
    ps = [_xval_ref.problem(n, d, b) for b in range(batch)]
    Xs = ref.test_points(n, m, d) if Xs is None else Xs
    o = dict(ps=ps, Xs_np=Xs, X=_t(ps[0]["X"], dev), Xs=_t(Xs, dev),
             beta=_t(np.stack([p["beta"] for p in ps]), dev),
             s=_t(np.array([p["s"] for p in ps]), dev),
             sp=_t(np.array([p["s_pred"] if nugget else p["s"] for p in ps]), dev))
    G = kernels.gram(o["X"], o["beta"], o["s"], _t(np.array([p["delta"] for p in ps]), dev),
                     batch=batch)
    o["ch"] = kernels.cholesky_inverse(G)
    o["ch"].check()
    o["args"] = (o["X"], o["Xs"], o["beta"], o["s"], o["sp"])
    return o


def _sub(ch, b):
    from gladsgp_amd import kernels
    return kernels.Cholesky(ch.n, ch.a_buf[b:b + 1], ch.linv_buf[b:b + 1].contiguous(),
                            ch.info[b:b + 1], ch.logdet[b:b + 1])


def _within(C, n, m, d, batch, jitter=0.0):
    for b in range(batch):
        R = ref.reference(n, m, d, b, jitter)
        s = _xval_ref.problem(n, d, b)["s"]
        err = float(np.max(np.abs(C[b] - R)))
        print(f"n={n} m={m} d={d} b={b}: |C - ref| = {err:.3e} = {err / s:.3e} s")
        assert err <= 1e-9 * s, (b, err)


@pytest.mark.parametrize("n,m,d", ref.SHAPES)
def test_covariance(dev, n, m, d):
    """The smallest problem, a tile edge of n and of the 16-column MFMA tile, the first
    off-diagonal tile of C with its mirror, npad = 640 with three column tiles, and d beyond the
    cross-covariance's <8> template; three problems with their own beta, s and delta."""
    from gladsgp_amd import kernels
    o = _setup(dev, n, m, d)
    C = kernels.predict_cov(o["ch"], *o["args"])
    assert C.shape == (3, m, m)
    Ch = C.cpu().numpy()
    assert np.isfinite(Ch).all()
    _bits(Ch, np.ascontiguousarray(np.swapaxes(Ch, 1, 2)))        # C[i,j], C[j,i]: same bits
    _within(Ch, n, m, d, 3)
    # the diagonal is gp_predict's marginal variance
    w = _t(np.stack([p["w"] for p in o["ps"]]), dev)
    _, var = kernels.predict(o["ch"], o["X"], o["Xs"], o["beta"], o["s"], o["sp"], w)
    dv = (torch.diagonal(C, dim1=1, dim2=2) - var).abs().max(dim=1).values.cpu().numpy()
    for b in range(3):
        assert dv[b] <= 2e-9 * o["ps"][b]["s"]


def test_jitter_and_out(dev):
    from gladsgp_amd import kernels
    n, m, d = 17, 5, 3
    o = _setup(dev, n, m, d)
    jit = np.array([0.25, 0.0, 1e-3])
    out = torch.full((3, m, m), -7.25, dtype=torch.float64, device=dev)
    C = kernels.predict_cov(o["ch"], *o["args"], jitter=_t(jit, dev), out=out)
    assert C is out
    C0 = kernels.predict_cov(o["ch"], *o["args"]).cpu().numpy()
    Ch = C.cpu().numpy()
    for b in range(3):
        off = ~np.eye(m, dtype=bool)
        _bits(Ch[b][off], C0[b][off])
        R = ref.reference(n, m, d, b, float(jit[b]))
        assert np.max(np.abs(Ch[b] - R)) <= 1e-9 * o["ps"][b]["s"]


@pytest.mark.parametrize("n,m,d", [(17, 5, 3), (200, 130, 8)])
def test_a_problem_does_not_depend_on_its_batch(dev, n, m, d):
    from gladsgp_amd import kernels
    o = _setup(dev, n, m, d)
    C = kernels.predict_cov(o["ch"], *o["args"])
    for b in range(3):
        one = kernels.predict_cov(_sub(o["ch"], b), o["X"], o["Xs"], o["beta"][b:b + 1],
                                  o["s"][b:b + 1], o["sp"][b:b + 1])
        _bits(one[0], C[b])
    _bits(kernels.predict_cov(o["ch"], *o["args"]), C)            # equal inputs, equal bits


@pytest.mark.parametrize("m", [5, 70])
def test_no_training_points_gives_the_prior(dev, m):
    """n = 0: K** with s_pred + jitter itself on the diagonal, nothing subtracted, no workspace."""
    from gladsgp_amd import _capi, kernels
    d = 3
    ps = [_xval_ref.problem(17, d, b) for b in range(2)]
    Xs = ref.test_points(17, m, d)
    beta = _t(np.stack([p["beta"] for p in ps]), dev)
    s = _t(np.array([p["s"] for p in ps]), dev)
    sp = _t(np.array([p["s_pred"] for p in ps]), dev)
    jit = _t(np.array([0.25, 0.0]), dev)
    Xs_t, any16 = _t(Xs, dev), torch.zeros(2, dtype=torch.float64, device=dev)
    C = torch.full((2, m, m), -7.25, dtype=torch.float64, device=dev)
    assert _capi.lib().gp_predict_cov_ws_bytes(0, m, 2) == 0
    _capi.call("gp_predict_cov", any16.data_ptr(), 0, 0, any16.data_ptr(), d, Xs_t.data_ptr(), d,
               0, m, d, beta.data_ptr(), d, s.data_ptr(), sp.data_ptr(), jit.data_ptr(),
               C.data_ptr(), m, m * m, 2, None, 0, kernels._stream(dev))
    Ch = C.cpu().numpy()
    for b, p in enumerate(ps):
        want = ref.prior(Xs, p["beta"], p["s"], p["s_pred"], (0.25, 0.0)[b])
        assert np.array_equal(np.diag(Ch[b]), np.diag(want))
        assert np.max(np.abs(Ch[b] - want)) <= 1e-9 * p["s"]
        assert np.array_equal(Ch[b], Ch[b].T)


def _raw_cov(dev, o, n, m, d, batch, Xe, Xse, be, Ce, linv=None):
    from gladsgp_amd import _capi, kernels
    lib = _capi.lib()
    nbytes = int(lib.gp_predict_cov_ws_bytes(n, m, batch))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    linv = o["ch"].linv_buf if linv is None else linv
    _capi.call("gp_predict_cov", linv.data_ptr(), linv.stride(1), linv.stride(0), Xe.ptr, Xe.ld,
               Xse.ptr, Xse.ld, n, m, d, be.ptr, be.stride, o["s"].data_ptr(),
               o["sp"].data_ptr(), None, Ce.ptr, Ce.ld, Ce.stride, batch, ws.data_ptr(), nbytes,
               kernels._stream(dev))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,m,d", [(17, 5, 3), (200, 130, 8)])
def test_layouts(dev, n, m, d):
    """Offset and strided C (ldc = m + 3, gaps between problems) and strided X / Xs / beta:
    the tight call's bits, and every sentinel outside the m x m blocks unchanged."""
    from gladsgp_amd import kernels
    o = _setup(dev, n, m, d)
    want = kernels.predict_cov(o["ch"], *o["args"]).cpu().numpy()
    X, Xs = o["ps"][0]["X"], o["Xs_np"]
    beta = np.stack([p["beta"] for p in o["ps"]])
    Xe = L.embed(X[None], offset=1, ld=d + 2, device=dev)
    Xse = L.embed(Xs[None], offset=3, ld=d + 1, device=dev)
    be = L.embed(beta[:, None, :], offset=2, ld=d, stride=d + 3, device=dev)
    Ce = L.blank((3, m, m), offset=5, ld=m + 3, stride=(m + 3) * m + 7, device=dev)
    _raw_cov(dev, o, n, m, d, 3, Xe, Xse, be, Ce)
    _bits(Ce.extract(), want)
    Ce.check()
    for e in (Xe, Xse, be):
        e.check(False)


def test_masking(dev):
    """NaN in the strict upper triangle of L^-1 and in its padding rows: the same bits."""
    from gladsgp_amd import kernels
    n, m, d = 200, 130, 8
    o = _setup(dev, n, m, d)
    want = kernels.predict_cov(o["ch"], *o["args"])
    npad = o["ch"].linv_buf.shape[1]
    dirty = o["ch"].linv_buf.clone()
    r = torch.arange(npad, device=dev)
    dirty[:, r[:, None] > r[None, :]] = float("nan")   # memory order [b, column, row]: row < column
    dirty[:, :, n:] = float("nan")                      # padding rows
    assert torch.isnan(dirty[0, 5, 3]) and torch.isnan(dirty[0, 3, n])
    assert float(dirty[0, 3, 5]) == float(o["ch"].linv_buf[0, 3, 5])
    ch2 = kernels.Cholesky(n, o["ch"].a_buf, dirty, o["ch"].info, o["ch"].logdet)
    _bits(kernels.predict_cov(ch2, *o["args"]), want)


def test_graph_capture(dev):
    """gp_predict_cov + gp_potrf + gp_mvn_draw captured into a graph replay to the eager bits."""
    from gladsgp_amd import kernels
    n, m, d = 129, 17, 8
    o = _setup(dev, n, m, d)
    C = torch.empty((3, m, m), dtype=torch.float64, device=dev)
    draws = torch.empty((3, 3, m), dtype=torch.float64, device=dev)
    mean = _t(np.random.default_rng(3).standard_normal((3, m)), dev)
    info = []

    def chain():
        kernels.predict_cov(o["ch"], *o["args"], out=C)
        info[:] = [kernels.cholesky_inplace(C)[0]]
        kernels.mvn_draw(C, mean, 99, 2, 3, unit0=4, out=draws)

    chain()                                            # eager (and the workspaces allocated)
    torch.cuda.synchronize()
    assert not info[0].cpu().numpy().any()
    want_C, want = C.clone(), draws.clone()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain()
    C.zero_()
    draws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _bits(C, want_C)
    _bits(draws, want)


def _factor_of_reference(dev, m, batch=2):
    """R = gp_potrf(C) of the numpy reference covariances at (n, d) = (17, 3): the buffer keeps
    C in its other triangle.  Returns (buffer, logical R with that triangle, mean)."""
    from gladsgp_amd import kernels
    Cn = np.stack([ref.reference(17, m, 3, b) for b in range(batch)])
    buf = _t(Cn, dev)
    info, _ = kernels.cholesky_inplace(buf)
    assert not info.cpu().numpy().any()
    Rl = np.swapaxes(buf.cpu().numpy(), 1, 2)          # logical [b, i, k]
    if m > 1:
        iu = np.triu_indices(m, 1)
        assert np.array_equal(Rl[0][iu], Cn[0][iu])    # gp_potrf left C above the diagonal
    mean = np.random.default_rng([m, 1]).standard_normal((batch, m))
    return buf, Rl, mean


@pytest.mark.parametrize("nsamp", [1, 3, 17])
@pytest.mark.parametrize("m", [1, 5, 130, 257])
def test_mvn_draw_against_numpy(dev, m, nsamp):
    """mean + tril(R) xi with xi from oracle.rng_ref.normals; tolerance 1e-12 max_i (|mean_i| +
    sum_k |R_ik xi_k|) (gp_realize's, test_gpu_dropin.py; the m-term accumulation adds at most
    m 2^-52 ~ 6e-14 of that magnitude)."""
    from gladsgp_amd import kernels
    buf, Rl, mean = _factor_of_reference(dev, m)
    got = kernels.mvn_draw(buf, _t(mean, dev), 2024, 5, nsamp, unit0=3).cpu().numpy()
    want, mag = ref.draws(Rl, mean, 2024, 5, nsamp, unit0=3)
    assert got.shape == (2, nsamp, m)
    for b in range(2):
        for r in range(nsamp):
            err = np.max(np.abs(got[b, r] - want[b, r]))
            assert err <= 1e-12 * np.max(mag[b, r]), (b, r, err)
    # no mean
    got0 = kernels.mvn_draw(buf, None, 2024, 5, nsamp, unit0=3).cpu().numpy()
    want0, mag0 = ref.draws(Rl, None, 2024, 5, nsamp, unit0=3)
    assert np.max(np.abs(got0 - want0)) <= 1e-12 * np.max(mag0)


@pytest.mark.parametrize("m,nsamp", [(5, 3), (130, 17)])
def test_mvn_draw_split_batch(dev, m, nsamp):
    """Two calls of one problem each with unit0 = 0, 1: the bits of one call of two."""
    from gladsgp_amd import kernels
    buf, _, mean = _factor_of_reference(dev, m)
    mean = _t(mean, dev)
    both = kernels.mvn_draw(buf, mean, 7, 1, nsamp)
    for b in range(2):
        one = kernels.mvn_draw(buf[b:b + 1].contiguous(), mean[b:b + 1], 7, 1, nsamp, unit0=b)
        _bits(one[0], both[b])


def test_moments(dev):
    """4096 joint draws of two problems: every entry of the sample covariance within 5 standard
    errors sqrt((C_ii C_jj + C_ij^2) / nsamp) of C and every sample mean within
    5 sqrt(C_ii / nsamp) of the mean (the numpy restatement alone reaches 2.8 and 1.9 of those
    with this seed)."""
    from gladsgp_amd import kernels
    n, m, d, nsamp = 17, 8, 3, 4096
    o = _setup(dev, n, m, d, batch=2)
    C = kernels.predict_cov(o["ch"], *o["args"])
    Ch = C.cpu().numpy()
    w = _t(np.stack([p["w"] for p in o["ps"]]), dev)
    mean, _ = kernels.predict(o["ch"], o["X"], o["Xs"], o["beta"], o["s"], o["sp"], w)
    R = C.clone()
    info, _ = kernels.cholesky_inplace(R)
    assert not info.cpu().numpy().any()
    x = kernels.mvn_draw(R, mean, 2024, 3, nsamp).cpu().numpy()
    mu = mean.cpu().numpy()
    for b in range(2):
        dm = np.abs(x[b].mean(axis=0) - mu[b]) / np.sqrt(np.diag(Ch[b]) / nsamp)
        dev_ = x[b] - mu[b]
        Sc = dev_.T @ dev_ / nsamp
        se = np.sqrt((np.outer(np.diag(Ch[b]), np.diag(Ch[b])) + Ch[b] ** 2) / nsamp)
        dc = np.abs(Sc - Ch[b]) / se
        print(f"b={b}: mean {dm.max():.2f} sigma, covariance {dc.max():.2f} sigma")
        assert dm.max() <= 5.0 and dc.max() <= 5.0


def test_not_positive_definite_is_reported(dev):
    """jitter = -s_pred: every pivot fails, gp_potrf reports info > 0 for every problem."""
    from gladsgp_amd import kernels
    o = _setup(dev, 17, 5, 3)
    C = kernels.predict_cov(o["ch"], *o["args"], jitter=-o["sp"])
    info, _ = kernels.cholesky_inplace(C)
    assert (info.cpu().numpy() > 0).all()
    with pytest.raises(kernels.JointNotPositiveDefinite, match=r"sample 1, PC 0.*joint_jitter"):
        kernels.check_joint_info(info, 2, 2, 0.0)


def _duplicated(n, m, d):
    Xs = ref.test_points(n, m, d).copy()
    Xs[3] = Xs[0]                                      # duplicated test points
    Xs[m - 1] = Xs[0]
    Xs[2] = _xval_ref.problem(n, d, 0)["X"][4]         # a test point on a training point
    return Xs


def test_duplicate_points_with_the_nugget(dev):
    from gladsgp_amd import kernels
    n, m, d = 17, 9, 3
    Xs = _duplicated(n, m, d)
    o = _setup(dev, n, m, d, Xs=Xs)
    C = kernels.predict_cov(o["ch"], *o["args"])
    Ch = C.cpu().numpy()
    for b, p in enumerate(o["ps"]):
        R = ref.closed_form(p["X"], Xs, p["beta"], p["s"], p["delta"], p["s_pred"])
        assert np.max(np.abs(Ch[b] - R)) <= 1e-9 * p["s"]
    info, _ = kernels.cholesky_inplace(C)
    assert not info.cpu().numpy().any()
    assert torch.isfinite(kernels.mvn_draw(C, None, 1, 0, 3)).all()


def test_duplicate_points_with_the_default_jitter(dev):
    """No prediction nugget (s_pred = s) and jitter 1e-8 s: clean and finite."""
    from gladsgp_amd import kernels
    n, m, d = 17, 9, 3
    o = _setup(dev, n, m, d, Xs=_duplicated(n, m, d), nugget=False)
    C = kernels.predict_cov(o["ch"], *o["args"], jitter=1e-8 * o["s"])
    info, _ = kernels.cholesky_inplace(C)
    assert not info.cpu().numpy().any()
    assert torch.isfinite(kernels.mvn_draw(C, None, 1, 0, 3)).all()


# ------------------------------------------------------------------------------ emulator level
def _model(dev, tmp_path, n=33, P=3, S=4, m=9):
    from gladsgp_amd import model as gm
    rng = np.random.default_rng(0)
    d, ny = 4, 200
    t = rng.random((n, d))
    modes = rng.standard_normal((5, ny)) * (0.5 ** np.arange(5))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + k) for k in range(5)], 1)
    y = 3.0 + coef @ modes + 1e-2 * rng.standard_normal((n, ny))
    data, model = gm.init_model(t, y, "joint", P, data_dir=str(tmp_path), device=dev,
                                verbose=False)
    srng = np.random.default_rng(1)
    samples = {"betaU": srng.uniform(0.2, 3.0, (S, (d + 1) * P)),
               "lamUz": srng.uniform(0.5, 3.0, (S, P)),
               "lamWs": srng.uniform(200, 3000, (S, P)),
               "lamWOs": srng.uniform(50, 500, (S, 1))}
    t_pred = np.random.default_rng(7).random((m, d))
    return t, model, samples, t_pred


def test_emulator_joint(dev, tmp_path):
    from gladsgp_amd import kernels
    from gladsgp_amd.emulator import EmulatorPrediction, gp_params
    from oracle import gp_ref
    S, P, m = 4, 3, 9
    t, model, samples, t_pred = _model(dev, tmp_path)
    base = EmulatorPrediction(model=model, samples=samples, t_pred=t_pred)
    pred = EmulatorPrediction(model=model, samples=samples, t_pred=t_pred, realize="joint",
                              seed=5, nsamp=2)
    _bits(pred.mean, base.mean)
    _bits(pred.var, base.var)
    assert pred.w.shape == (S, m, P) and np.isfinite(pred.w).all()
    assert np.abs(pred.w - pred.mean).max() > 0
    # draws do not depend on the grouping
    one = EmulatorPrediction(model=model, samples=samples, t_pred=t_pred, realize="joint",
                             seed=5, nsamp=2, group=1)
    _bits(one.w, pred.w)
    _bits(one.joint_w_dev, pred.joint_w_dev)
    _bits(one.mean, base.mean)
    # the covariance: diagonal against .var, every block against the numpy reference
    C = pred.cov()
    assert C.shape == (S, P, m, m)
    beta, s, delta, sp = gp_params(samples, model.LamSim.cpu().numpy(), model.d, P, True)
    var = pred.var                                                  # (S, m, P)
    a = np.full(m, 1.0 / m)
    lf_mean, lf_var = pred.linear_functional(a)
    assert lf_mean.shape == (S, P) and lf_var.shape == (S, P)
    for i in range(S):
        for j in range(P):
            assert np.max(np.abs(np.diag(C[i, j]) - var[i, :, j])) <= 2e-9 * s[i, j]
            R = ref.closed_form(t, t_pred, beta[i, j], s[i, j], delta[i, j], sp[i, j])
            assert np.max(np.abs(C[i, j] - R)) <= 1e-9 * s[i, j]
            assert abs(lf_var[i, j] - a @ R @ a) <= 1e-9 * s[i, j]
            assert abs(lf_mean[i, j] - a @ pred.mean[i, :, j]) <= 1e-12 * np.abs(pred.mean).max()
    Cd = pred.cov(to_host=False)
    _bits(Cd, C)
    k_mean, k_var = pred.linear_functional(np.stack([a, np.eye(m)[2]]))
    assert k_mean.shape == (2, S, P)
    np.testing.assert_allclose(k_var[0], lf_var, rtol=0, atol=1e-15)
    np.testing.assert_allclose(k_var[1], C[:, :, 2, 2], rtol=0, atol=1e-15)
    # fresh joint draws: (k, S, m, P), reproducible, offset 0 / nsamp 2 are the constructor's
    sw = pred.sample_w(seed=5, offset=0, joint=True, nsamp=2)
    assert sw.shape == (2, S, m, P)
    _bits(sw[0], pred.w)
    _bits(sw, pred.joint_w_dev)
    assert np.abs(pred.sample_w(joint=True, nsamp=1)[0] - pred.w).max() > 0
    # get_y / summary take the joint .w as any other
    y = pred.get_y()
    Kd = model.data.sim_data.K.cpu().numpy()
    y_ref = gp_ref.reconstruct_y(pred.w, Kd, model.data.sim_data.y_mean.cpu().numpy(),
                                 model.data.sim_data.y_sd.cpu().numpy())
    np.testing.assert_allclose(y, y_ref, rtol=1e-10, atol=1e-10)
    mean_f, lo, hi = pred.summary(rng=np.random.default_rng(3))
    assert mean_f.shape == (m, Kd.shape[1]) and (lo <= hi).all()
    # the marginal modes are unchanged and refuse the joint-only calls
    with pytest.raises(ValueError, match="joint"):
        base.cov()
    with pytest.raises(ValueError, match="joint"):
        base.sample_w(joint=True)
    assert kernels.JointNotPositiveDefinite is not None


def test_emulator_joint_refusals(dev, tmp_path):
    from gladsgp_amd import kernels
    from gladsgp_amd.emulator import EmulatorPrediction
    t, model, samples, t_pred = _model(dev, tmp_path)
    kw = dict(model=model, samples=samples, realize="joint")
    with pytest.raises(kernels.JointNotPositiveDefinite, match=r"sample 0, PC 0.*joint_jitter"):
        EmulatorPrediction(t_pred=t_pred, joint_jitter=-2.0, **kw)
    with pytest.raises(ValueError, match="ctx"):
        EmulatorPrediction(t_pred=t_pred, ctx=object(), **kw)
    big = np.random.default_rng(2).random((EmulatorPrediction.joint_max_points + 1, 4))
    with pytest.raises(ValueError, match="joint_max_points"):
        EmulatorPrediction(t_pred=big, **kw)
    with pytest.raises(ValueError, match="realize"):
        EmulatorPrediction(model=model, samples=samples, t_pred=t_pred, realize="svd")
    # without the nugget the default jitter 1e-8 applies
    p0 = EmulatorPrediction(t_pred=t_pred, pred_nugget=False, **kw)
    assert p0.joint_jitter == 1e-8 and np.isfinite(p0.w).all()
    assert EmulatorPrediction(t_pred=t_pred, **kw).joint_jitter == 0.0
