"""GPU: gp_alpha / gp_mean_response (csrc/response.hip) and gladsgp_amd.response against the numpy
restatement tests/_response_ref.py: rounding-error bounds worked out from the arithmetic, the
project's oracle-parity bound |got - ref| <= 1e-8 max(1, max|ref|) against predict-and-average,
the bit identities, strided / offset layouts with sentinels, the emulator-level surfaces against
looping EmulatorPrediction, and graph capture.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _layouts as L
import _response_ref as rref
import _xval_ref as xref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BATCH = 3
ORDER = {"cyclic": 0, "ascending": 1}


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


@functools.lru_cache(maxsize=None)
def _problems(n, d, batch=BATCH):
    return tuple(xref.problem(n, d, b) for b in range(batch))


def _factor(dev, n, d, batch=BATCH):
    """(problems, Cholesky, w (batch, n)) of problems 0 .. batch - 1, each with its own beta, s
    and delta: Gram and L^-1 by the project's own kernels."""
    from gladsgp_amd import kernels
    ps = _problems(n, d, batch)
    G = kernels.gram(_t(ps[0]["X"], dev), _t(np.stack([p["beta"] for p in ps]), dev),
                     _t(np.array([p["s"] for p in ps]), dev),
                     _t(np.array([p["delta"] for p in ps]), dev), batch=batch)
    ch = kernels.cholesky_inverse(G)
    ch.check()
    return ps, ch, _t(np.stack([p["w"] for p in ps]), dev)


def _d(n):
    return 8 if n >= 128 else 3


# ------------------------------------------------------------------------------------ gp_alpha
@pytest.mark.parametrize("n", [1, 2, 17, 128, 129, 200, 513])
def test_alpha(dev, n):
    """alpha = L^-T (L^-1 w) against numpy on the downloaded L^-1: two dot-product bounds,
    doubled for numpy's own error."""
    from gladsgp_amd import kernels
    _, ch, w = _factor(dev, n, _d(n))
    got = kernels.alpha(ch, w).cpu().numpy()
    Li = np.tril(ch.Linv.cpu().numpy())
    wn = w.cpu().numpy()
    for b in range(BATCH):
        want = Li[b].T @ (Li[b] @ wn[b])
        bnd = 4 * (n + 1) * EPS * (np.abs(Li[b]).T @ (np.abs(Li[b]) @ np.abs(wn[b])))
        err = np.abs(got[b] - want)
        print(f"n={n} b={b} max err {err.max():.3e} max err/bound {np.max(err / bnd):.3e}")
        assert (err <= bnd).all(), (b, float(np.max(err / bnd)))


def test_alpha_never_reads_the_upper_triangle(dev):
    from gladsgp_amd import kernels
    n = 200
    _, ch, w = _factor(dev, n, 8)
    npad = ch.linv_buf.shape[1]
    dirty = ch.linv_buf.clone()
    r = torch.arange(npad, device=dev)
    dirty[:, r[:, None] > r[None, :]] = 1e300          # memory order [b, column, row]: row < column
    assert float(dirty[0, 5, 3]) == 1e300 and float(dirty[0, 3, 5]) == float(ch.linv_buf[0, 3, 5])
    ch2 = kernels.Cholesky(n, ch.a_buf, dirty, ch.info, ch.logdet)
    _bits(kernels.alpha(ch, w), kernels.alpha(ch2, w))


# ---------------------------------------------------------------------------- gp_mean_response
def _grid(T, lo, hi, rev=False):
    t = np.linspace(lo, hi, T) if T > 1 else np.array([0.5 * (lo + hi)])
    return t[::-1].copy() if rev else t


def _xint(I, nc, seed):
    return np.random.default_rng([I, nc, seed]).random((I, nc)) if nc > 0 else None


# (n, d, effects, order, T1, T2, I): the chunk edge (256 / 257), the tile edge (16 / 17), one
# node, the largest grid, no integration (d == nfree), GPFIT_MAX_DIM, reversed pairs
CASES = [
    (1, 1, [0], "cyclic", 1, None, 0),
    (17, 1, [0], "ascending", 11, None, 0),
    (17, 2, [(0, 1), (1, 0)], "ascending", 11, 16, 0),
    (256, 3, [0, 1, 2], "cyclic", 17, None, 10),
    (257, 3, [1], "ascending", 16, None, 1),
    (257, 3, [(2, 0), (0, 1)], "ascending", 17, 11, 20),
    (300, 8, list(range(8)), "cyclic", 11, None, 20),
    (300, 8, [(6, 2)], "ascending", 64, 17, 10),
    (300, 32, [0, 31], "cyclic", 64, None, 20),
    (300, 32, [(31, 3), (4, 30)], "ascending", 16, 1, 10),
]


def _run(dev, n, d, effects, order, T1, T2, I):
    """The kernel's surfaces (batch, E, ...) with the device's own alpha, and the inputs."""
    from gladsgp_amd import kernels
    ps, ch, w = _factor(dev, n, d)
    alpha = kernels.alpha(ch, w)
    nfree = 1 if T2 is None else 2
    t1 = _grid(T1, 0.0, 1.0)
    t2 = None if T2 is None else _grid(T2, 0.05, 0.9, rev=True)
    Xint = _xint(I, d - nfree, n)
    got = kernels.mean_response(
        _t(ps[0]["X"], dev), alpha, _t(np.stack([p["beta"] for p in ps]), dev),
        _t(np.array([p["s"] for p in ps]), dev), effects, _t(t1, dev),
        None if t2 is None else _t(t2, dev), None if Xint is None else _t(Xint, dev), order=order)
    return ps, alpha.cpu().numpy(), t1, t2, Xint, got.cpu().numpy()


@pytest.mark.parametrize("n,d,effects,order,T1,T2,I", CASES)
def test_mean_response(dev, n, d, effects, order, T1, T2, I):
    """Against ``direct`` with the device's own alpha: the worst-case rounding of the exponent
    ((d + 2) sum beta ulps of it, inputs in [0, 1]^d), one-ulp exps, the average, the products and
    an n-term sum in any order, doubled for numpy; and the project's parity bound against the
    oracle's predict-and-average (its own alpha)."""
    ps, alpha, t1, t2, Xint, got = _run(dev, n, d, effects, order, T1, T2, I)
    shape = (BATCH, len(effects), T1) if T2 is None else (BATCH, len(effects), T2, T1)
    assert got.shape == shape
    for b, p in enumerate(ps):
        c = 2 * ((d + 2) * p["beta"].sum() + I + n + 9) * EPS
        for e, eff in enumerate(effects):
            args = (eff, order, t1, t2, Xint)
            want = rref.direct(p["X"], alpha[b], p["beta"], p["s"], *args)
            bnd = c * rref.bound(p["X"], alpha[b], p["beta"], p["s"], *args)
            err = np.abs(got[b, e] - want)
            ref = rref.predicted(p["X"], p["w"], p["beta"], p["s"], p["delta"], *args)
            perr = np.max(np.abs(got[b, e] - ref))
            print(f"n={n} d={d} b={b} effect={eff}: max err {err.max():.3e}, err/bound "
                  f"{np.max(err / bnd):.3e}, against predict {perr:.3e}")
            assert (err <= bnd).all(), (b, eff, float(np.max(err / bnd)))
            assert perr <= 1e-8 * max(1.0, np.max(np.abs(ref))), (b, eff, perr)


def _operands(dev, n, d, nfree, I, T1, T2):
    from gladsgp_amd import kernels
    ps, ch, w = _factor(dev, n, d)
    return dict(X=_t(ps[0]["X"], dev), alpha=kernels.alpha(ch, w),
                beta=_t(np.stack([p["beta"] for p in ps]), dev),
                s=_t(np.array([p["s"] for p in ps]), dev), t1=_t(_grid(T1, 0, 1), dev),
                t2=None if nfree == 1 else _t(_grid(T2, 0, 1, rev=True), dev),
                Xint=_t(_xint(I, d - nfree, 1), dev))


@pytest.mark.parametrize("nfree", [1, 2])
def test_a_problem_alone_equals_it_in_the_batch(dev, nfree):
    from gladsgp_amd import kernels
    o = _operands(dev, 300, 8, nfree, 10, 11, 17)
    effects = [0, 5, 7] if nfree == 1 else [(0, 5), (7, 1)]
    order = "cyclic" if nfree == 1 else "ascending"
    full = kernels.mean_response(o["X"], o["alpha"], o["beta"], o["s"], effects, o["t1"], o["t2"],
                                 o["Xint"], order=order)
    for b in range(BATCH):
        one = kernels.mean_response(o["X"], o["alpha"][b:b + 1].contiguous(),
                                    o["beta"][b:b + 1].contiguous(), o["s"][b:b + 1].contiguous(),
                                    effects, o["t1"], o["t2"], o["Xint"], order=order)
        _bits(one[0], full[b])


@pytest.mark.parametrize("nfree", [1, 2])
def test_an_effect_alone_equals_it_among_64_and_beyond(dev, nfree):
    """64 effects in one call, 70 split over two: every surface has the bits of its own call."""
    from gladsgp_amd import kernels
    o = _operands(dev, 257, 8, nfree, 10, 11, 5)
    if nfree == 1:
        effects = [k % 8 for k in range(70)]
    else:
        pairs = [(a, b) for a in range(8) for b in range(8) if a != b]          # 56 ordered pairs
        effects = (pairs + pairs)[:70]
    call = lambda eff: kernels.mean_response(o["X"], o["alpha"], o["beta"], o["s"], eff, o["t1"],  # noqa
                                             o["t2"], o["Xint"])
    r64, r70 = call(effects[:64]), call(effects)
    assert r70.shape[1] == 70
    _bits(r64, r70[:, :64])
    for k in (0, 13, 63, 64, 69):
        _bits(call([effects[k]])[:, 0], r70[:, k])


def _raw(dev, n, d, batch, effects, nfree, order, T1, T2, I, Xe, Ae, Be, s, t1, t2, Ie, Oe):
    from gladsgp_amd import _capi
    host = (ctypes.c_int * (len(effects) * nfree))(*np.asarray(effects).reshape(-1).tolist())
    rc = _capi.lib().gp_mean_response(
        Xe.ptr, n, d, Xe.ld, Ae.ptr, Ae.stride, Be.ptr, Be.stride, s.data_ptr(), batch,
        ctypes.addressof(host), nfree, len(effects), ORDER[order], t1.data_ptr(), T1,
        t2.data_ptr() if t2 is not None else None, T2 or 0, Ie.ptr, I, Ie.ld, Oe.ptr, Oe.ld,
        Oe.stride, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", ["odd_ld", "off8", "gap16"])
@pytest.mark.parametrize("nfree", [1, 2])
def test_layouts(dev, case, nfree):
    """Strided, offset and gapped X (ldx > d), alpha, beta, Xint (ldi > columns) and out (lde and
    ldb with gaps), and gp_alpha's own operands: the bits of the tight call, nothing outside the
    surfaces written, no padding read (the sentinels are NaN)."""
    from gladsgp_amd import _capi, kernels
    n, d, I, T1 = 200, 8, 10, 11
    T2 = None if nfree == 1 else 5
    TT = T1 * (T2 or 1)
    effects = [3, 0] if nfree == 1 else [(7, 2), (0, 4)]
    order = "cyclic" if nfree == 1 else "ascending"
    ps, ch, w = _factor(dev, n, d)
    o = _operands(dev, n, d, nfree, I, T1, T2)
    # gp_alpha from placed operands
    lib = _capi.lib()
    Li = L.place(ch.linv_buf.cpu().numpy(), case, device=dev)
    We = L.place(w.cpu().numpy()[:, None, :], case, device=dev)
    Ae = L.blank_case((BATCH, 1, n), case, device=dev)
    ws = torch.empty(max(lib.gp_alpha_ws_bytes(n, BATCH), 256), dtype=torch.uint8, device=dev)
    rc = lib.gp_alpha(Li.ptr, Li.ld, Li.stride, n, We.ptr, We.stride, Ae.ptr, Ae.stride, BATCH,
                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    Ae.check()
    Li.check(False)
    We.check(False)
    _bits(Ae.extract()[:, 0], o["alpha"])
    # gp_mean_response reading that alpha in place
    tight = kernels.mean_response(o["X"], o["alpha"], o["beta"], o["s"], effects, o["t1"],
                                  o["t2"], o["Xint"], order=order)
    Xe = L.place(o["X"].cpu().numpy()[None], case, device=dev)
    Be = L.place(o["beta"].cpu().numpy()[:, None, :], case, device=dev)
    Ie = L.place(o["Xint"].cpu().numpy()[None], case, device=dev)
    Oe = L.blank_case((BATCH, len(effects), TT), case, device=dev)
    rc = _raw(dev, n, d, BATCH, effects, nfree, order, T1, T2, I, Xe, Ae, Be, o["s"], o["t1"],
              o["t2"], Ie, Oe)
    assert rc == 0
    Oe.check()
    for op in (Xe, Be, Ie):
        op.check(False)
    _bits(Oe.extract().reshape(tight.shape), tight)


def test_noops_write_nothing(dev):
    """E = 0 and batch = 0 through the C entry point: validated, nothing launched or written."""
    n, d = 17, 3
    o = _operands(dev, n, d, 1, 10, 11, None)
    Xe = L.place(o["X"].cpu().numpy()[None], "tight", device=dev)
    Ae = L.place(o["alpha"].cpu().numpy()[:, None, :], "tight", device=dev)
    Be = L.place(o["beta"].cpu().numpy()[:, None, :], "tight", device=dev)
    Ie = L.place(o["Xint"].cpu().numpy()[None], "tight", device=dev)
    Oe = L.blank((BATCH, 2, 11), device=dev)
    for batch, effects in ((BATCH, []), (0, [0, 1])):
        assert _raw(dev, n, d, batch, effects, 1, "cyclic", 11, None, 10, Xe, Ae, Be, o["s"],
                    o["t1"], None, Ie, Oe) == 0
        Oe.check(False)


# --------------------------------------------------------------------------- emulator level
def _ensemble(n=80, ny=40, d=8, seed=5):
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


PAIRS = [(1, 5), (6, 2)]


@pytest.fixture(scope="module")
def rmodel(dev, tmp_path_factory):
    from gladsgp_amd import model as gm
    t, y = _ensemble()
    _, model = gm.init_model(t, y, "resp", 3, data_dir=str(tmp_path_factory.mktemp("d")),
                             device=dev, verbose=False)
    return model, _samples(2, 8, 3)


def _looped(model, samples, effects, order, xi, design):
    """(S, E, nodes, P): EmulatorPrediction at the explicit points of every effect, averaged over
    the integration points in numpy."""
    from gladsgp_amd import emulator as em
    nfree = len(rref.free_dims(effects[0]))
    t2 = [None] if nfree == 1 else xi
    out = []
    for eff in effects:
        P = np.concatenate([rref.points(eff, order, v1, v2, design, model.d)
                            for v2 in t2 for v1 in xi])
        pr = em.EmulatorPrediction(model=model, samples=samples, t_pred=P)
        out.append(pr.w.reshape(pr.S, len(t2) * len(xi), -1, pr.P).mean(axis=2))
    return np.stack(out, axis=1)


@pytest.mark.parametrize("kind", ["main", "pairs"])
def test_emulator_surfaces_match_looped_predictions(dev, rmodel, kind):
    from gladsgp_amd import emulator as em
    from gladsgp_amd import response
    from oracle import gp_ref
    model, samples = rmodel
    S, P, T = 2, 3, 11
    if kind == "main":
        res = response.mean_response(model, samples)
        effects, order, grid = list(range(8)), "cyclic", (8, T)
        assert res.design.shape == (20, 7)
    else:
        res = response.mean_response_pairs(model, samples, PAIRS)
        effects, order, grid = PAIRS, "ascending", (2, T, T)
        assert res.design.shape == (10, 6)
    assert isinstance(res, em.EmulatorPrediction)
    m = int(np.prod(grid))
    assert (res.S, res.m, res.P) == (S, m, P) and res.grid == grid
    # the points are the reference's float32 ones
    np.testing.assert_array_equal(res.targets, np.linspace(0, 1, T).astype(np.float32))
    np.testing.assert_array_equal(res.design, res.design.astype(np.float32))
    w = res.w
    assert w.shape == (S, m, P) and (res.var == 0).all()
    want = _looped(model, samples, effects, order, res.targets, res.design).reshape(S, m, P)
    err = np.max(np.abs(w - want))
    print(f"{kind}: w err {err:.3e} (max |w| {np.max(np.abs(want)):.3e})")
    assert err <= 1e-8 * max(1.0, np.max(np.abs(want)))
    sd_ = model.data.sim_data
    ny = sd_.K.shape[1]
    y_want = gp_ref.reconstruct_y(want, sd_.K.cpu().numpy(), sd_.y_mean.cpu().numpy(),
                                  sd_.y_sd.cpu().numpy()).mean(axis=0).reshape(grid + (ny,))
    r = res.response()
    assert r.shape == grid + (ny,)
    yerr = np.max(np.abs(r - y_want))
    print(f"{kind}: response err {yerr:.3e}")
    assert yerr <= 1e-8 * max(1.0, np.max(np.abs(y_want)))
    assert res.get_y().shape == (S, m, ny)
    # S = 2: the band over the samples is their own spread, which brackets their mean
    mean, lo, hi = res.summary(0.025, add_error=False)
    assert mean.shape == lo.shape == hi.shape == (m, ny)
    tol = 1e-12 * np.max(np.abs(mean))
    assert (lo <= mean + tol).all() and (mean <= hi + tol).all()
    np.testing.assert_allclose(mean.reshape(r.shape), r, rtol=0, atol=tol)
    # with the error draws (the default): a finite band around the same mean
    mean_e, lo_e, hi_e = res.summary(0.025, rng=np.random.default_rng(0))
    assert mean_e.shape == (m, ny) and np.isfinite(lo_e).all() and np.isfinite(hi_e).all()
    np.testing.assert_allclose(mean_e, mean, rtol=0, atol=tol)
    with pytest.raises(ValueError, match="realize"):
        res.sample_w()
    # one GP per factorisation gives the same bits as all six at once
    if kind == "main":
        small = response.mean_response(model, samples, budget_bytes=1)
    else:
        small = response.mean_response_pairs(model, samples, PAIRS, budget_bytes=1)
    _bits(small.w, w)


def test_scalar_model(dev, tmp_path):
    """The reference's own use: one output, one PC (ny = P = 1).  response()[..., 0] is its
    Y_integrated_mean / y_response_pair, here against the looped predictions' get_y()."""
    from gladsgp_amd import emulator as em
    from gladsgp_amd import model as gm
    from gladsgp_amd import response
    rng = np.random.default_rng(11)
    t = rng.random((40, 3)).astype(np.float32)
    y = (np.sin(2 * np.pi * t @ [0.3, 0.9, 0.5]) + t[:, 1] ** 2)[:, None].astype(np.float32)
    _, model = gm.init_model(t, y, "scalar", 1, data_dir=str(tmp_path), device=dev, verbose=False)
    samples = _samples(2, 3, 1)
    res = response.mean_response(model, samples, ntarget=5, nintegrate=4)
    assert res.get_y().shape == (2, 15, 1)
    want = np.zeros((3, 5))
    for k in range(3):
        P = np.concatenate([rref.points(k, "cyclic", v, None, res.design, 3) for v in res.targets])
        pr = em.EmulatorPrediction(model=model, samples=samples, t_pred=P)
        want[k] = pr.get_y().mean(axis=0).reshape(5, 4).mean(axis=1)
    r = res.response()
    assert r.shape == (3, 5, 1)
    assert np.max(np.abs(r[..., 0] - want)) <= 1e-8 * max(1.0, np.max(np.abs(want)))
    rp = response.mean_response_pairs(model, samples, [(2, 0)], ntarget=3, nintegrate=4)
    assert rp.design.shape == (4, 1)
    wantp = np.zeros((3, 3))
    for i1, v2 in enumerate(rp.targets):
        for i2, v1 in enumerate(rp.targets):
            xp = np.zeros((4, 3))
            xp[:, 1] = rp.design[:, 0]                  # dim_int = [1]
            xp[:, 2] = v1                               # d1 = 2 at xx1[i1, i2] = xi[i2]
            xp[:, 0] = v2                               # d2 = 0 at xx2[i1, i2] = xi[i1]
            pr = em.EmulatorPrediction(model=model, samples=samples, t_pred=xp)
            wantp[i1, i2] = pr.get_y().mean()
    got = rp.response()[0, :, :, 0]
    assert np.max(np.abs(got - wantp)) <= 1e-8 * max(1.0, np.max(np.abs(wantp)))


def test_emulator_surface_arguments(dev, rmodel):
    from gladsgp_amd import response
    model, samples = rmodel
    res = response.mean_response(model, samples, dims=[6, 1], ntarget=5, nintegrate=4,
                                 round_f32=False, group=4)
    assert res.grid == (2, 5) and res.design.shape == (4, 7)
    np.testing.assert_array_equal(res.targets, np.linspace(0, 1, 5))
    full = response.mean_response(model, samples, targets=res.targets, design=res.design,
                                  round_f32=False)
    _bits(res.w.reshape(2, 2, 5, 3), full.w.reshape(2, 8, 5, 3)[:, [6, 1]])
    with pytest.raises(ValueError, match="design"):
        response.mean_response_pairs(model, samples, PAIRS, design=np.zeros((10, 7)))


def test_graph_capture(dev):
    """gp_alpha + gp_mean_response captured on a side stream and replayed once: the bits of the
    eager calls."""
    from gladsgp_amd import kernels
    n, d = 200, 8
    o = _operands(dev, n, d, 2, 10, 11, 17)
    _, ch, w = _factor(dev, n, d)
    effects = [(1, 5), (6, 2)]
    al = torch.empty((BATCH, n), dtype=torch.float64, device=dev)
    out = torch.empty((BATCH, 2, 17, 11), dtype=torch.float64, device=dev)

    def both():
        kernels.alpha(ch, w, out=al)
        kernels.mean_response(o["X"], al, o["beta"], o["s"], effects, o["t1"], o["t2"],
                              o["Xint"], out=out)

    both()                                             # eager (and the workspace allocated)
    torch.cuda.synchronize()
    want_al, want = al.clone(), out.clone()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    al.zero_()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _bits(al, want_al)
    _bits(out, want)
