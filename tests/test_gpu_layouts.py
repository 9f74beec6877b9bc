"""GPU: every C-ABI kernel on strided, offset and sub-view operands (include/gpfit.h, layout
contract; DESIGN.md "Operand layouts and the branches they select").

Each operand lives in one guarded allocation (tests/_layouts.py): NaN outside the logical region
of an input, a sentinel bit pattern outside what the header says an output writes, checked by
integer comparison after the call.  Every case is compared with the numpy fp64 oracle at the
tolerance the tight test of the same operation states (tests/test_gpu_kernels.py's docstring,
test_gpu_fitside.py, test_gpu_mcmc.py) and, bit for bit, with the tight call on the same values:
a layout changes which load / store instructions run, not the order of the arithmetic.

Layout cases (ids): tight | odd_ld | off8 | off16 | odd_stride | gap16, see _layouts.dims.
"""
import ctypes

import numpy as np
import pytest
import torch

import _layouts as L
from oracle import gp_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


def _call(name, *args):
    from gladsgp_amd import _capi
    return _capi.call(name, *args)


def _lib():
    from gladsgp_amd import _capi
    return _capi.lib()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _t(x, dev, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device=dev)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _vec(v, ld, dev):
    """Per-problem vectors (B, len) at element offset 1, problem b at b * ld."""
    v = np.asarray(v)
    return L.embed(v[:, None, :], offset=1, ld=v.shape[1], stride=ld, device=dev)


def _vec_out(B, length, ld, dev):
    return L.blank((B, 1, length), offset=1, ld=length, stride=ld, device=dev)


def _rows(X, ld, dev):
    """Row-major design matrix / beta rows at element offset 1 with row stride ld."""
    return L.embed(np.asarray(X)[None], offset=1, ld=ld, device=dev)


# ------------------------------------------------------------------------------------------
# gp_gram_ardse / gp_cross_ardse
# ------------------------------------------------------------------------------------------
def _gram_inputs(n, d, m):
    rng = np.random.default_rng(1000 * n + d)
    return dict(X=rng.random((n, d)), Xs=rng.random((m, d)), beta=rng.uniform(0.5, 5.0, (3, d)),
                s=np.array([1.3, 0.7, 2.0]), delta=np.array([1e-6, 1e-4, 1e-2]))


def _run_gram(dev, n, d, case):
    p = _cached(("gram_in", n, d), lambda: _gram_inputs(n, d, 133))
    X, bt = _rows(p["X"], d + 3, dev), _rows(p["beta"], d + 2, dev)
    G = L.blank_case((3, n, n), case, dev)
    s, delta = _t(p["s"], dev), _t(p["delta"], dev)
    _call("gp_gram_ardse", X.ptr, n, d, X.ld, bt.ptr, bt.ld, s.data_ptr(), delta.data_ptr(), G.ptr,
          G.ld, G.stride, 3, _st(dev))
    torch.cuda.synchronize()
    G.check()
    X.check(False)
    bt.check(False)
    return L.cm(G.extract())


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("d", [3, 9, 17])
@pytest.mark.parametrize("n", [65, 130])
def test_gram_layouts(dev, n, d, case):
    p = _cached(("gram_in", n, d), lambda: _gram_inputs(n, d, 133))
    tight = _cached(("gram", n, d), lambda: _run_gram(dev, n, d, "tight"))
    G = tight if case == "tight" else _run_gram(dev, n, d, case)
    for b in range(3):
        ref = gp_ref.gram_ardse(p["X"], p["beta"][b], p["s"][b], p["delta"][b])
        assert np.max(np.abs(G[b] - ref)) <= 8 * EPS * p["s"][b]
        np.testing.assert_array_equal(G[b], G[b].T)
    assert _same_bits(G, tight)


def _run_cross(dev, n, m, d, case):
    p = _cached(("gram_in", n, d), lambda: _gram_inputs(n, d, m))
    X, Xs, bt = _rows(p["X"], d + 3, dev), _rows(p["Xs"], d + 1, dev), _rows(p["beta"], d + 2, dev)
    Kt = L.blank_case((3, m, n), case, dev)
    s = _t(p["s"], dev)
    _call("gp_cross_ardse", X.ptr, n, X.ld, Xs.ptr, m, Xs.ld, d, bt.ptr, bt.ld, s.data_ptr(),
          Kt.ptr, Kt.ld, Kt.stride, 3, _st(dev))
    torch.cuda.synchronize()
    Kt.check()
    for op in (X, Xs, bt):
        op.check(False)
    return Kt.extract()                                   # [b, j, i] = K*[j, i]


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("d", [3, 9, 17])
def test_cross_layouts(dev, d, case):
    n, m = 70, 133
    p = _cached(("gram_in", n, d), lambda: _gram_inputs(n, d, m))
    tight = _cached(("cross", n, d), lambda: _run_cross(dev, n, m, d, "tight"))
    Kt = tight if case == "tight" else _run_cross(dev, n, m, d, case)
    for b in range(3):
        ref = gp_ref.cross_ardse(p["Xs"], p["X"], p["beta"][b], p["s"][b])
        assert np.max(np.abs(Kt[b] - ref)) <= 8 * EPS * p["s"][b]
    assert _same_bits(Kt, tight)


# ------------------------------------------------------------------------------------------
# gp_potrf_inv_ws / gp_potrf_ws / gp_trtri
# ------------------------------------------------------------------------------------------
def _lower(n):
    """Memory-order (col, row) mask of the lower triangle (row >= col)."""
    return np.triu(np.ones((n, n), bool))[None]


def _spd(n, B):
    rng = np.random.default_rng(n)
    X = rng.random((n, 8))
    return np.stack([gp_ref.gram_ardse(X, rng.uniform(0.5, 5, 8), 1.0, 1e-4) for _ in range(B)])


class _path:
    """gp_set_potrf_path for the calls inside, the previous value restored afterwards."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.prev = _lib().gp_set_potrf_path(self.path)

    def __exit__(self, *exc):
        _lib().gp_set_potrf_path(self.prev)


def _run_potrf_inv(dev, G, path, case, finite=True):
    """gp_potrf_inv_ws with A and L^-1 in `case`: (L, Linv padded, logdet, info), guards checked."""
    B, n, _ = G.shape
    npad = _lib().gp_padded_n(n)
    A = L.place(L.cm(G), case, mask=_lower(n), device=dev)
    Li = L.blank_case((B, npad, npad), case, dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    logdet = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    ws = _ws(_lib().gp_potrf_inv_ws_bytes(n, B), dev)
    with _path(path):
        _call("gp_potrf_inv_ws", A.ptr, n, A.ld, A.stride, Li.ptr, Li.ld, Li.stride, B,
              info.data_ptr(), logdet.data_ptr(), ws.data_ptr(), ws.numel(), _st(dev))
    torch.cuda.synchronize()
    A.check(written=_lower(n))        # strict upper triangle and rows n..lda-1 untouched
    Li.check()                        # rows npad..ldinv-1 and the inter-problem gaps untouched
    Lf = L.cm(A.extract(finite=False))
    return (np.tril(Lf), L.cm(Li.extract(finite=finite)), logdet.cpu().numpy(),
            info.cpu().tolist())


def _run_potrf(dev, G, path, case):
    B, n, _ = G.shape
    A = L.place(L.cm(G), case, mask=_lower(n), device=dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    logdet = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    ws = _ws(_lib().gp_potrf_ws_bytes(n, B), dev)
    with _path(path):
        _call("gp_potrf_ws", A.ptr, n, A.ld, A.stride, B, info.data_ptr(), logdet.data_ptr(),
              ws.data_ptr(), ws.numel(), _st(dev))
    torch.cuda.synchronize()
    A.check(written=_lower(n))
    return np.tril(L.cm(A.extract(finite=False))), logdet.cpu().numpy(), info.cpu().tolist()


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("path", [0, 1], ids=["auto", "sweep"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [64, 129, 192, 200])
def test_factorisation_layouts(dev, n, B, path, case):
    """gp_potrf_inv_ws and gp_potrf_ws with A (and L^-1) in every layout, on the persistent
    kernel (path 0) and the blocked sweep (path 1): test_cholesky_inverse's and
    test_potrf_plain_matches_potrf_inv's assertions, the guards, and the tight call's bits."""
    G = _cached(("spd", n, B), lambda: _spd(n, B))
    tight = _cached(("potrf_inv", n, B, path), lambda: _run_potrf_inv(dev, G, path, "tight"))
    Lg, Linv, logdet, info = tight if case == "tight" else _run_potrf_inv(dev, G, path, case)
    assert info == [0] * B
    assert np.all(np.isfinite(Lg))
    npad = Linv.shape[-1]
    for b in range(B):
        Lref = np.linalg.cholesky(G[b])
        assert np.linalg.norm(Lg[b] @ Lg[b].T - G[b]) / np.linalg.norm(G[b]) <= 1e-13
        assert np.max(np.abs(Lg[b] - Lref)) <= 1e-10 * np.max(np.abs(Lref))
        assert np.max(np.abs(Linv[b][:n, :n] @ Lg[b] - np.eye(n))) <= 1e-9
        np.testing.assert_allclose(logdet[b], 2 * np.sum(np.log(np.diag(Lref))), rtol=0,
                                   atol=1e-9 * n)
        # exactly zero above the diagonal and in the padding, from a NaN-filled buffer
        assert np.all(np.triu(Linv[b], 1) == 0)
        assert np.all(Linv[b][n:, :] == 0) and np.all(Linv[b][:, n:] == 0)
        np.testing.assert_allclose(Lg[b], Lref, rtol=0, atol=1e-12)
    assert Linv.shape == (B, npad, npad)
    assert _same_bits(Lg, tight[0]) and _same_bits(Linv, tight[1])
    assert _same_bits(logdet, tight[2])
    # the plain factorisation: the same L and logdet, bit for bit
    L2, logdet2, info2 = _run_potrf(dev, G, path, case)
    assert info2 == [0] * B
    assert _same_bits(L2, Lg) and _same_bits(logdet2, logdet)


@pytest.mark.parametrize("case", ["off8", "odd_stride"])
@pytest.mark.parametrize("path", [0, 1], ids=["auto", "sweep"])
def test_factorisation_layouts_non_pd(dev, path, case):
    n, B = 129, 3
    rng = np.random.default_rng(9)
    Gs = []
    for b in range(B):
        M = rng.standard_normal((n, n))
        G = M @ M.T + n * np.eye(n)
        if b == 1:
            G[70, 70] = -3.0
        Gs.append(G)
    G = np.stack(Gs)
    Lg, _, _, info = _run_potrf_inv(dev, G, path, case, finite=False)
    assert info == [0, 71, 0]
    _, _, info2 = _run_potrf(dev, G, path, case)
    assert info2 == [0, 71, 0]
    for b in (0, 2):
        assert np.linalg.norm(Lg[b] @ Lg[b].T - G[b]) / np.linalg.norm(G[b]) <= 1e-13


def _run_trtri(dev, Lf, case):
    B, n, _ = Lf.shape
    npad = _lib().gp_padded_n(n)
    Lin = L.place(L.cm(Lf), case, mask=_lower(n), device=dev)    # strict upper: NaN, never read
    Li = L.blank_case((B, npad, npad), case, dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    _call("gp_trtri", Lin.ptr, n, Lin.ld, Lin.stride, Li.ptr, Li.ld, Li.stride, B,
          info.data_ptr(), _st(dev))
    torch.cuda.synchronize()
    Lin.check(False)
    Li.check()
    return L.cm(Li.extract()), info.cpu().tolist()


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [64, 129, 192, 200])
def test_trtri_layouts(dev, n, B, case):
    G = _cached(("spd", n, B), lambda: _spd(n, B))
    Lf = np.linalg.cholesky(G)
    tight = _cached(("trtri", n, B), lambda: _run_trtri(dev, Lf, "tight"))
    Li, info = tight if case == "tight" else _run_trtri(dev, Lf, case)
    assert info == [0] * B
    for b in range(B):
        inv = np.linalg.inv(Lf[b])
        Xb = Li[b][:n, :n]
        assert np.all(np.triu(Li[b], 1) == 0)
        assert np.all(Li[b][n:, :] == 0) and np.all(Li[b][:, n:] == 0)
        assert np.max(np.abs(Xb - inv)) <= 1e-10 * np.abs(inv).max()
        assert np.max(np.abs(Xb @ Lf[b] - np.eye(n))) <= 1e-10
    assert _same_bits(Li, tight[0])


# ------------------------------------------------------------------------------------------
# the prediction family
# ------------------------------------------------------------------------------------------
M_PRED, CHUNK, B_PRED = 300, 128, 2
_LINV_FOR = {"tight": "tight", "odd_ld": "tight", "off8": "off16", "off16": "off16",
             "odd_stride": "gap16", "gap16": "gap16"}


def _pred_problem(dev, n, d):
    """Inputs, the oracle and the all-tight device pipeline gram -> potrf_inv -> gp_predict."""
    rng = np.random.default_rng(n * 7 + d)
    m, B = M_PRED, B_PRED
    p = dict(n=n, d=d, X=rng.random((n, d)), Xs=rng.random((m, d)),
             beta=rng.uniform(0.5, 3, (B, d)), s=np.array([1.5, 0.8]),
             delta=np.array([1e-3, 2e-3]), W=rng.standard_normal((B, n)))
    p["sp"] = p["s"] + 0.01
    p["ref"] = [gp_ref.predict(p["X"], p["Xs"], p["W"][b], p["beta"][b], p["s"][b],
                               p["delta"][b], s_pred=p["sp"][b]) for b in range(B)]
    npad = _lib().gp_padded_n(n)
    p["npad"] = npad
    st = _st(dev)
    X, Xs, bt, W = (_t(p[k], dev) for k in ("X", "Xs", "beta", "W"))
    s, delta, sp = (_t(p[k], dev) for k in ("s", "delta", "sp"))
    G = torch.empty((B, n, n), dtype=torch.float64, device=dev)
    _call("gp_gram_ardse", X.data_ptr(), n, d, d, bt.data_ptr(), d, s.data_ptr(),
          delta.data_ptr(), G.data_ptr(), n, n * n, B, st)
    Li = torch.full((B, npad, npad), float("nan"), dtype=torch.float64, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    logdet = torch.empty(B, dtype=torch.float64, device=dev)
    ws = _ws(_lib().gp_potrf_inv_ws_bytes(n, B), dev)
    _call("gp_potrf_inv_ws", G.data_ptr(), n, n, n * n, Li.data_ptr(), npad, npad * npad, B,
          info.data_ptr(), logdet.data_ptr(), ws.data_ptr(), ws.numel(), st)
    mean = torch.empty((B, m), dtype=torch.float64, device=dev)
    var = torch.empty((B, m), dtype=torch.float64, device=dev)
    pws = _ws(_lib().gp_predict_ws_bytes(n, m, B, CHUNK), dev)
    _call("gp_predict", Li.data_ptr(), npad, npad * npad, X.data_ptr(), d, Xs.data_ptr(), d, n,
          m, d, bt.data_ptr(), d, s.data_ptr(), sp.data_ptr(), W.data_ptr(), n,
          mean.data_ptr(), var.data_ptr(), m, B, pws.data_ptr(), pws.numel(), CHUNK, st)
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [0] * B
    p.update(Linv=Li.cpu().numpy(), Lbuf=G.cpu().numpy(), logdet=logdet.cpu().numpy(),
             mean=mean.cpu().numpy(), var=var.cpu().numpy())
    for b in range(B):                       # test_predict_edges' tolerances
        mr, vr = p["ref"][b]
        np.testing.assert_allclose(p["mean"][b], mr, rtol=0, atol=1e-9 * max(1, np.abs(mr).max()))
        np.testing.assert_allclose(p["var"][b], vr, rtol=0, atol=1e-10 * p["s"][b])
    return p


class _PredOps:
    """The padded operands shared by the prediction calls (each at element offset 1)."""

    def __init__(self, p, dev):
        n, d = p["n"], p["d"]
        self.X, self.Xs = _rows(p["X"], d + 3, dev), _rows(p["Xs"], d + 1, dev)
        self.bt = _rows(p["beta"], d + 2, dev)
        self.W = _vec(p["W"], n + 5, dev)
        self.s, self.sp, self.delta = (_t(p[k], dev) for k in ("s", "sp", "delta"))
        self.dev, self.p = dev, p

    def outputs(self):
        return (_vec_out(B_PRED, M_PRED, M_PRED + 7, self.dev),
                _vec_out(B_PRED, M_PRED, M_PRED + 7, self.dev))

    def cross_args(self):
        p = self.p
        return (self.X.ptr, self.X.ld, self.Xs.ptr, self.Xs.ld, p["n"], M_PRED, p["d"],
                self.bt.ptr, self.bt.ld, self.s.data_ptr())

    def verify(self, mean, var, bits=True):
        """Guards of mean / var (m..ldo-1 and after the last problem), inputs unchanged, the
        tight gp_predict's bits (or, bits=False, the oracle alone)."""
        torch.cuda.synchronize()
        mean.check()
        var.check()
        for op in (self.X, self.Xs, self.bt, self.W):
            op.check(False)
        mh, vh = mean.extract()[:, 0, :], var.extract()[:, 0, :]
        if bits:
            assert _same_bits(mh, self.p["mean"]) and _same_bits(vh, self.p["var"])
        for b in range(B_PRED):
            mr, vr = self.p["ref"][b]
            np.testing.assert_allclose(mh[b], mr, rtol=0, atol=1e-9 * max(1, np.abs(mr).max()))
            np.testing.assert_allclose(vh[b], vr, rtol=0, atol=1e-10 * self.p["s"][b])
        return mh, vh


PRED_SHAPES = [(130, 5), (130, 12), (600, 8)]


@pytest.mark.parametrize("case", L.ALIGNED_CASES)
@pytest.mark.parametrize("n,d", PRED_SHAPES)
def test_predict_layouts(dev, n, d, case):
    """gp_predict, gp_predict_ex (padded; z computed or shipped), gp_predict_z and
    gp_predict_cross + gp_predict_solve with L^-1 in the layouts its alignment rule admits and
    every other operand padded and offset: the tight gp_predict's bits."""
    p = _cached(("pred", n, d), lambda: _pred_problem(dev, n, d))
    o = _PredOps(p, dev)
    npad, B, m, st = p["npad"], B_PRED, M_PRED, _st(dev)
    Li = L.place(p["Linv"], case, device=dev)
    pws = _ws(_lib().gp_predict_ws_bytes(n, m, B, CHUNK), dev)
    tail = (B, pws.data_ptr(), pws.numel(), CHUNK)

    mean, var = o.outputs()
    _call("gp_predict", Li.ptr, Li.ld, Li.stride, *o.cross_args(), o.sp.data_ptr(), o.W.ptr,
          o.W.stride, mean.ptr, var.ptr, mean.stride, *tail, st)
    o.verify(mean, var)

    mean, var = o.outputs()
    _call("gp_predict_ex", Li.ptr, Li.ld, Li.stride, *o.cross_args(), o.sp.data_ptr(), o.W.ptr,
          o.W.stride, mean.ptr, var.ptr, mean.stride, *tail, 0, None, 0, st)
    o.verify(mean, var)

    # z = L^-1 w shipped: gp_predict_z, then gp_predict_ex reads z and never w_hat (all NaN)
    z = _vec_out(B, npad, npad + 3, dev)
    zws = _ws(_lib().gp_predict_z_ws_bytes(n, B), dev)
    _call("gp_predict_z", Li.ptr, Li.ld, Li.stride, 0, n, o.W.ptr, o.W.stride, z.ptr, z.stride,
          B, zws.data_ptr(), zws.numel(), st)
    torch.cuda.synchronize()
    z.check()
    zh = z.extract()[:, 0, :]
    assert np.all(zh[:, n:] == 0)
    for b in range(B):
        zr = np.tril(L.cm(p["Linv"][b])[:n, :n]) @ p["W"][b]
        np.testing.assert_allclose(zh[b, :n], zr, rtol=0, atol=1e-9 * max(1, np.abs(zr).max()))
    nan_w = _vec_out(B, n, n + 5, dev)
    mean, var = o.outputs()
    _call("gp_predict_ex", Li.ptr, Li.ld, Li.stride, *o.cross_args(), o.sp.data_ptr(), nan_w.ptr,
          nan_w.stride, mean.ptr, var.ptr, mean.stride, *tail, 0, z.ptr, z.stride, st)
    o.verify(mean, var)
    z.check()
    assert _same_bits(z.extract()[:, 0, :], zh)           # an input here: left as it was

    mean, var = o.outputs()
    cws = _ws(_lib().gp_predict_prepared_ws_bytes(n, m, B, CHUNK), dev)
    _call("gp_predict_cross", *o.cross_args(), B, cws.data_ptr(), cws.numel(), CHUNK, st)
    _call("gp_predict_solve", Li.ptr, Li.ld, Li.stride, n, m, o.sp.data_ptr(), o.W.ptr,
          o.W.stride, mean.ptr, var.ptr, mean.stride, B, cws.data_ptr(), cws.numel(), CHUNK, st)
    o.verify(mean, var)
    Li.check(False)


def _run_predict_chol(dev, p, o, case):
    n, B, m = p["n"], B_PRED, M_PRED
    Lf = L.place(p["Lbuf"], case, mask=_lower(n), device=dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    ws = _ws(_lib().gp_predict_chol_ws_bytes(n, m, B, CHUNK), dev)
    mean, var = o.outputs()
    _call("gp_predict_chol", Lf.ptr, Lf.ld, Lf.stride, *o.cross_args(), o.sp.data_ptr(),
          o.W.ptr, o.W.stride, mean.ptr, var.ptr, mean.stride, B, info.data_ptr(),
          ws.data_ptr(), ws.numel(), CHUNK, _st(dev))
    mh, vh = o.verify(mean, var, bits=False)
    Lf.check(False)
    assert info.cpu().tolist() == [0] * B
    return mh, vh


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("n,d", PRED_SHAPES)
def test_predict_chol_layouts(dev, n, d, case):
    """gp_predict_chol with the factor L in every layout.  Its L^-1 comes from gp_trtri, which
    agrees with gp_potrf_inv's to rounding only (test_predict_from_cholesky_factor), so the
    bit-for-bit comparison is with the tight gp_predict_chol call, not with gp_predict."""
    p = _cached(("pred", n, d), lambda: _pred_problem(dev, n, d))
    o = _PredOps(p, dev)
    tight = _cached(("pchol", n, d), lambda: _run_predict_chol(dev, p, o, "tight"))
    mh, vh = tight if case == "tight" else _run_predict_chol(dev, p, o, case)
    assert _same_bits(mh, tight[0]) and _same_bits(vh, tight[1])


@pytest.mark.parametrize("ctx", [False, True], ids=["serial", "ctx"])
@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("n,d", PRED_SHAPES)
def test_fit_predict_layouts(dev, n, d, case, ctx):
    """gp_fit_predict with G in every layout (L^-1 in the nearest layout its alignment rule
    admits), without and with a context: mean / var, L, L^-1 and logdet are the bits of the
    tight gram -> potrf_inv -> predict sequence."""
    p = _cached(("pred", n, d), lambda: _pred_problem(dev, n, d))
    o = _PredOps(p, dev)
    B, m, npad = B_PRED, M_PRED, p["npad"]
    G = L.blank_case((B, n, n), case, dev)
    Li = L.blank_case((B, npad, npad), _LINV_FOR[case], dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    logdet = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    ws = _ws(_lib().gp_fit_predict_ws_bytes(n, m, B, CHUNK), dev)
    mean, var = o.outputs()
    h = ctypes.c_void_p()
    if ctx:
        _call("gp_ctx_create", -1.0, -1, ctypes.addressof(h))
    try:
        _call("gp_fit_predict", *o.cross_args(), o.delta.data_ptr(), o.sp.data_ptr(), o.W.ptr,
              o.W.stride, G.ptr, G.ld, G.stride, Li.ptr, Li.ld, Li.stride, info.data_ptr(),
              logdet.data_ptr(), mean.ptr, var.ptr, mean.stride, B, ws.data_ptr(), ws.numel(),
              CHUNK, h.value, _st(dev))
        torch.cuda.synchronize()
    finally:
        if ctx:
            _call("gp_ctx_destroy", h.value)
    o.verify(mean, var)
    G.check()
    Li.check()
    assert info.cpu().tolist() == [0] * B
    low = _lower(n)[0]
    Lg = G.extract(finite=False)
    assert all(_same_bits(Lg[b][low], p["Lbuf"][b][low]) for b in range(B))
    assert _same_bits(Li.extract(), p["Linv"])
    assert _same_bits(logdet.cpu().numpy(), p["logdet"])


# ------------------------------------------------------------------------------------------
# gp_trmv / gp_nll / gp_loglik
# ------------------------------------------------------------------------------------------
def _nll_problem(n):
    B, d = 3, 4
    rng = np.random.default_rng(n + 5)
    X = rng.random((n, d))
    beta = rng.uniform(0.5, 4, (B, d))
    s, delta = rng.uniform(0.5, 2, B), rng.uniform(1e-3, 1e-2, B)
    G = np.stack([gp_ref.gram_ardse(X, beta[b], s[b], delta[b]) for b in range(B)])
    Lf = np.linalg.cholesky(G)
    w = np.stack([Lf[b] @ rng.standard_normal(n) for b in range(B)])
    Linv = np.stack([np.tril(np.linalg.inv(Lf[b])) for b in range(B)])
    logdet = np.array([2 * np.sum(np.log(np.diag(Lf[b]))) for b in range(B)])
    z = np.stack([Linv[b] @ w[b] for b in range(B)])
    nll = 0.5 * np.sum(z * z, axis=1) + 0.5 * logdet
    return dict(X=X, beta=beta, s=s, delta=delta, w=w, Linv=Linv, logdet=logdet, z=z, nll=nll)


def _run_trmv_nll(dev, p, n, case, padded):
    B = 3
    Li = L.place(L.cm(p["Linv"]), case, device=dev)
    w = _vec(p["w"], n + 5, dev) if padded else _vec(p["w"], n, dev)
    z = _vec_out(B, n, n + 3 if padded else n, dev)
    _call("gp_trmv", Li.ptr, Li.ld, Li.stride, n, w.ptr, w.stride, z.ptr, z.stride, B, _st(dev))
    nll = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    work = L.blank((1, 1, B * n), device=dev)
    logdet = _t(p["logdet"], dev)
    _call("gp_nll", Li.ptr, Li.ld, Li.stride, n, w.ptr, w.stride, logdet.data_ptr(), nll.data_ptr(),
          work.ptr, B, _st(dev))
    torch.cuda.synchronize()
    z.check()
    work.check()
    Li.check(False)
    w.check(False)
    return z.extract()[:, 0, :], nll.cpu().numpy()


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("n", [130, 600])
def test_trmv_nll_layouts(dev, n, case):
    p = _cached(("nll", n), lambda: _nll_problem(n))
    tight = _cached(("trmv", n), lambda: _run_trmv_nll(dev, p, n, "tight", False))
    z, nll = _run_trmv_nll(dev, p, n, case, True)
    for b in range(3):
        np.testing.assert_allclose(z[b], p["z"][b], rtol=0,
                                   atol=1e-9 * max(1, np.abs(p["z"][b]).max()))
    assert np.all(np.abs(nll - p["nll"]) <= 1e-9 * np.maximum(1.0, np.abs(p["nll"])))
    assert _same_bits(z, tight[0]) and _same_bits(nll, tight[1])


def _run_loglik(dev, p, n, path, padded):
    B, d = 3, 4
    X = _rows(p["X"], d + 3 if padded else d, dev)
    bt = _rows(p["beta"], d + 2 if padded else d, dev)
    w = _vec(p["w"], n + 5 if padded else n, dev)
    nb = _lib().gp_loglik_ws_bytes(n, B)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    ll = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((B,), 99, dtype=torch.int32, device=dev)
    s, delta = _t(p["s"], dev), _t(p["delta"], dev)
    with _path(path):
        _call("gp_loglik", X.ptr, n, d, X.ld, bt.ptr, bt.ld, s.data_ptr(), delta.data_ptr(), w.ptr,
              w.stride, B, ws.data_ptr(), nb,
              ll.data_ptr(), info.data_ptr(), _st(dev))
    torch.cuda.synchronize()
    for op in (X, bt, w):
        op.check(False)
    assert info.cpu().tolist() == [0] * B
    return ll.cpu().numpy()


@pytest.mark.parametrize("path", [0, 1], ids=["auto", "sweep"])
@pytest.mark.parametrize("n", [130, 600])
def test_loglik_layouts(dev, n, path):
    p = _cached(("nll", n), lambda: _nll_problem(n))
    tight = _run_loglik(dev, p, n, path, False)
    ll = _run_loglik(dev, p, n, path, True)
    ref = -p["nll"]
    assert np.all(np.abs(ll - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))), (ll, ref)
    assert _same_bits(ll, tight)


# ------------------------------------------------------------------------------------------
# gp_dgemm / gp_gemm_ex
# ------------------------------------------------------------------------------------------
def _gemm_mats(ta, tb, m, n, k):
    rng = np.random.default_rng(m + n + k + ta * 2 + tb)
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    return A, B, rng.standard_normal((m, n))


def _run_gemm(dev, ta, tb, A, B, C0, cases, alpha=0.7, beta=-1.3, ex=False, track=True):
    """C = alpha op(A) op(B) + beta C with (A, B, C) in the layouts `cases`."""
    m, n = C0.shape
    k = A.shape[0] if ta else A.shape[1]
    Ae = L.place(L.cm(A)[None], cases[0], device=dev, track=track)
    Be = L.place(L.cm(B)[None], cases[1], device=dev, track=track)
    Ce = L.place(L.cm(C0)[None], cases[2], device=dev)
    ws = _ws(_lib().gp_dgemm_ws_bytes(m, n, k), dev)
    if ex:
        _call("gp_gemm_ex", ta, tb, m, n, k, alpha, Ae.ptr, 0, Ae.ld, Be.ptr, 0, Be.ld, beta,
              Ce.ptr, Ce.ld, ws.data_ptr(), ws.numel(), _st(dev))
    else:
        _call("gp_dgemm", ta, tb, m, n, k, alpha, Ae.ptr, Ae.ld, Be.ptr, Be.ld, beta, Ce.ptr,
              Ce.ld, ws.data_ptr(), ws.numel(), _st(dev))
    torch.cuda.synchronize()
    Ce.check()                                            # rows m..ldc-1 untouched
    if track:
        Ae.check(False)
        Be.check(False)
    return L.cm(Ce.extract()[0])


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,n,k", [(70, 33, 129), (128, 64, 64), (17, 5, 60000)])
def test_gemm_layouts(dev, m, n, k, ta, tb, case):
    """General and split-K GEMM with A, B and C in one layout each (one problem: odd_stride and
    gap16 differ from off16 by the base offset and the size of ld only)."""
    A, B, C0 = _cached(("gemm_in", m, n, k, ta, tb), lambda: _gemm_mats(ta, tb, m, n, k))
    tight = _cached(("gemm", m, n, k, ta, tb),
                    lambda: _run_gemm(dev, ta, tb, A, B, C0, ["tight"] * 3))
    got = _run_gemm(dev, ta, tb, A, B, C0, [case] * 3)
    ref = 0.7 * ((A.T if ta else A) @ (B.T if tb else B)) - 1.3 * C0
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.sqrt(k) * np.abs(ref).max())
    assert _same_bits(got, tight)
    assert _same_bits(_run_gemm(dev, ta, tb, A, B, C0, [case] * 3, ex=True), tight)


_TS = {"tsk": (1, 0, 512, 25, 70000), "tsm": (0, 0, 20000, 25, 300),
       "tsm_t": (1, 1, 25, 20000, 300)}


def _ts_mats(kind):
    ta, tb, m, n, k = _TS[kind]
    rng = np.random.default_rng(m + n + k)
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    return A, B, rng.standard_normal((m, n))


@pytest.mark.parametrize("kind", ["tsk", "tsm", "tsm_t"])
def test_gemm_tall_skinny_big_operand_off8(dev, kind):
    """The big operand of each tall-skinny kernel at an even ld with an 8-B-only base: the 16-B
    tsk form must be refused (blas.hip ts_vec_ok); the result is the tight call's bits."""
    ta, tb, m, n, k = _TS[kind]
    A, B, C0 = _cached(("ts_in", kind), lambda: _ts_mats(kind))
    tight = _run_gemm(dev, ta, tb, A, B, C0, ["tight"] * 3, track=False)
    cases = ["tight", "off8", "tight"] if kind == "tsm_t" else ["off8", "tight", "tight"]
    got = _run_gemm(dev, ta, tb, A, B, C0, cases, track=False)
    ref = 0.7 * ((A.T if ta else A) @ (B.T if tb else B)) - 1.3 * C0
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.sqrt(k) * np.abs(ref).max())
    assert _same_bits(got, tight)


@pytest.mark.parametrize("kind", ["general", "splitk", "tsk", "tsm", "tsm_t"])
def test_gemm_beta_zero_does_not_read_c(dev, kind):
    """beta = 0: C is not read, so a NaN-filled C gives the finite result of a zero-filled one."""
    if kind in _TS:
        ta, tb, m, n, k = _TS[kind]
        A, B, _ = _cached(("ts_in", kind), lambda: _ts_mats(kind))
    else:
        ta, tb = 0, 0
        m, n, k = (70, 33, 129) if kind == "general" else (17, 5, 60000)
        A, B, _ = _cached(("gemm_in", m, n, k, ta, tb), lambda: _gemm_mats(ta, tb, m, n, k))
    nan = _run_gemm(dev, ta, tb, A, B, np.full((m, n), np.nan), ["tight"] * 3, beta=0.0,
                    track=False)
    zero = _run_gemm(dev, ta, tb, A, B, np.zeros((m, n)), ["tight"] * 3, beta=0.0, track=False)
    assert np.all(np.isfinite(nan))
    assert _same_bits(nan, zero)
    ref = 0.7 * ((A.T if ta else A) @ (B.T if tb else B))
    np.testing.assert_allclose(nan, ref, rtol=1e-12, atol=1e-12 * np.sqrt(k) * np.abs(ref).max())


# ------------------------------------------------------------------------------------------
# gp_sim_stats / gp_standardize / gp_field
# ------------------------------------------------------------------------------------------
def _run_stats(dev, Y, padded):
    n, ny = Y.shape
    Ye = L.embed(Y[None], offset=1, ld=ny + 3, device=dev) if padded else L.embed(Y[None],
                                                                                  device=dev)
    mu, sd = L.blank((1, 1, ny), device=dev), L.blank((1, 1, ny), device=dev)
    _call("gp_sim_stats", Ye.ptr, n, ny, Ye.ld, 1e-6, mu.ptr, sd.ptr, _st(dev))
    off, ldo = (1, ny + 5) if padded else (0, ny)
    out = L.blank((1, n, ny), offset=off, ld=ldo, device=dev)
    _call("gp_standardize", Ye.ptr, n, ny, Ye.ld, mu.ptr, sd.ptr, out.ptr, out.ld, 0, _st(dev))
    back = L.blank((1, n, ny), offset=off, ld=ldo, device=dev)
    _call("gp_standardize", out.ptr, n, ny, out.ld, mu.ptr, sd.ptr, back.ptr, back.ld, 1,
          _st(dev))
    torch.cuda.synchronize()
    for op in (mu, sd, out, back):
        op.check()
    Ye.check(False)
    return mu.extract()[0, 0], sd.extract()[0, 0], out.extract()[0], back.extract()[0]


def test_sim_stats_standardize_layouts(dev):
    rng = np.random.default_rng(0)
    n, ny = 37, 1001
    Y = rng.standard_normal((n, ny)) * rng.uniform(0, 3, ny) + rng.standard_normal(ny)
    Y[:, 5] = 2.5
    mu_r, sd_r, ystd_r = gp_ref.standardize(Y, 1e-6)
    tight = _run_stats(dev, Y, False)
    mu, sd, ystd, back = _run_stats(dev, Y, True)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(sd, sd_r, rtol=1e-13)
    assert sd[5] == 1e-6
    np.testing.assert_allclose(ystd, ystd_r, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(back, Y, rtol=1e-12, atol=1e-12)
    for a, b in zip((mu, sd, ystd, back), tight):
        assert _same_bits(a, b)


def _field_inputs():
    rng = np.random.default_rng(5)
    rows, P, ncols = 70, 9, 1001
    return dict(W=rng.standard_normal((rows, P)), K=rng.standard_normal((P, ncols)),
                sd=rng.uniform(0.5, 2, ncols), mu=rng.standard_normal(ncols))


def _run_field(dev, p, f32, off, ldy, padded):
    rows, P = p["W"].shape
    ncols = p["K"].shape[1]
    W = _rows(p["W"], P + 3, dev) if padded else L.embed(p["W"][None], device=dev)
    K = _rows(p["K"], ncols + 1, dev) if padded else L.embed(p["K"][None], device=dev)
    dt = np.float32 if f32 else np.float64
    Y = L.blank((1, rows, ncols), offset=off, ld=ldy, device=dev, dtype=dt)
    sd, mu = _t(p["sd"], dev), _t(p["mu"], dev)
    _call("gp_field", W.ptr, W.ld, rows, P, K.ptr, K.ld, ncols, sd.data_ptr(), mu.data_ptr(), None,
          Y.ptr, Y.ld, int(f32), _st(dev))
    torch.cuda.synchronize()
    Y.check()
    W.check(False)
    K.check(False)
    return Y.extract()[0]


def _field_generic(dev, p):
    """gp_dgemm + gp_standardize(inverse = 1), the arithmetic gp_field promises bit for bit."""
    rows, P = p["W"].shape
    ncols = p["K"].shape[1]
    W, K = _t(p["W"], dev), _t(p["K"], dev)
    Y = torch.empty((rows, ncols), dtype=torch.float64, device=dev)
    out = torch.empty_like(Y)
    _call("gp_dgemm", 0, 0, ncols, rows, P, 1.0, K.data_ptr(), ncols, W.data_ptr(), P, 0.0,
          Y.data_ptr(), ncols, None, 0, _st(dev))
    mu, sd = _t(p["mu"], dev), _t(p["sd"], dev)
    _call("gp_standardize", Y.data_ptr(), rows, ncols, ncols, mu.data_ptr(), sd.data_ptr(),
          out.data_ptr(), ncols, 1, _st(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("off,ldy", [(0, 1004), (1, 1004), (0, 1003)],
                         ids=["ld4_aligned", "ld4_off1", "ld_odd"])
def test_field_layouts(dev, off, ldy, f32):
    p = _cached("field_in", _field_inputs)
    generic = _cached("field_generic", lambda: _field_generic(dev, p))
    tight = _cached(("field", f32), lambda: _run_field(dev, p, f32, 0, 1001, False))
    Y = _run_field(dev, p, f32, off, ldy, True)
    ref = (p["W"] @ p["K"]) * p["sd"] + p["mu"]
    np.testing.assert_allclose(Y, ref, rtol=1e-6 if f32 else 1e-12,
                               atol=(1e-6 if f32 else 1e-12) * np.abs(ref).max())
    want = generic.astype(np.float32) if f32 else generic
    assert np.array_equal(Y, want) and np.array_equal(Y, tight)


# ------------------------------------------------------------------------------------------
# gp_mean_var / gp_shift_diag / gp_rowscale / gp_syevj
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 255, 257, 262145, 300001])
def test_mean_var(dev, N, ddof):
    if N == 1 and ddof == 1:
        assert _lib().gp_mean_var(16, 1, 1, 16, 16, None) == -3      # ddof >= N is rejected
        return
    x = 1e6 + np.random.default_rng(N).standard_normal(N)            # mean 1e6, sd 1
    xe = L.embed(x[None, None, :], offset=1, device=dev)
    out = L.blank((1, 1, 2), offset=1, device=dev)
    work = L.blank((1, 1, 1024), device=dev)
    _call("gp_mean_var", xe.ptr, N, ddof, out.ptr, work.ptr, _st(dev))
    torch.cuda.synchronize()
    out.check()
    work.check()
    xe.check(False)
    got = out.extract()[0, 0]
    np.testing.assert_allclose(got[0], np.mean(x), rtol=1e-12)
    np.testing.assert_allclose(got[1], np.var(x, ddof=ddof), rtol=1e-12, atol=0)


@pytest.mark.parametrize("r", [1, 25, 257])
def test_shift_diag(dev, r):
    rng = np.random.default_rng(r)
    A = rng.standard_normal((r, r))
    # a positive diagonal: the trace is a sum of like-signed terms, so the order in which the
    # kernel adds them moves it by a few ulp and rtol 1e-14 is meaningful without an atol
    A[np.diag_indices(r)] = rng.uniform(1, 2, r)
    Ae = L.embed(L.cm(A)[None], offset=1, ld=r + 3, device=dev)
    _call("gp_shift_diag", Ae.ptr, r, Ae.ld, 0.37, _st(dev))
    torch.cuda.synchronize()
    Ae.check(written=np.eye(r, dtype=bool)[None])         # off-diagonal bits and padding
    got = L.cm(Ae.extract()[0])
    np.testing.assert_allclose(np.diag(got), np.diag(A) + 0.37 * np.trace(A), rtol=1e-14, atol=0)


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("rows,cols", [(1, 1), (25, 1001), (300, 7)])
def test_rowscale(dev, rows, cols, inv):
    rng = np.random.default_rng(rows + cols)
    M = rng.standard_normal((rows, cols))
    f = rng.uniform(0.5, 2, rows)
    f[rows // 2] = 0.0
    Me = L.embed(L.cm(M)[None], offset=1, ld=rows + 3, device=dev)
    fe = L.embed(f[None, None, :], offset=1, device=dev)
    _call("gp_rowscale", Me.ptr, rows, cols, Me.ld, fe.ptr, inv, _st(dev))
    torch.cuda.synchronize()
    Me.check()
    fe.check(False)
    g = np.where(f != 0, 1.0 / np.where(f != 0, f, 1.0), 0.0) if inv else f
    got = L.cm(Me.extract()[0])
    np.testing.assert_allclose(got, M * g[:, None], rtol=1e-15, atol=0)
    assert np.all(got[rows // 2] == 0)                    # inv = 1: a row of zeros, not inf


def _syevj_matrix(r, kind):
    rng = np.random.default_rng(r)
    if kind == "repeated":
        Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
        lam = np.concatenate([[5.0, 5.0, 5.0], rng.uniform(0.1, 4, r - 3)])
        A = (Q * lam) @ Q.T
    else:                                                 # PSD of rank r - 2
        M = rng.standard_normal((r, r - 2))
        A = M @ M.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("want_sqrt", [0, 1])
@pytest.mark.parametrize("kind", ["repeated", "rank_deficient"])
@pytest.mark.parametrize("r", [63, 64, 65, 101])
def test_syevj_layouts(dev, r, kind, want_sqrt):
    A = _syevj_matrix(r, kind)
    w_ref = np.linalg.eigh(A)[0][::-1]
    Ae = L.embed(L.cm(A)[None], offset=1, ld=r + 3, device=dev)
    V = L.blank((1, r, r), offset=1, ld=r + 5, device=dev)
    W = L.blank((1, 1, r), offset=1, device=dev)
    sweeps = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("gp_syevj", Ae.ptr, r, Ae.ld, W.ptr, V.ptr, V.ld, 30, 1e-15, sweeps.data_ptr(),
          want_sqrt, _st(dev))
    torch.cuda.synchronize()
    Ae.check()                                            # A is destroyed, its padding is not
    V.check()
    W.check()
    Wh, Vh = W.extract()[0, 0], L.cm(V.extract()[0])
    assert np.all(np.diff(Wh) <= 0)
    if want_sqrt:                                         # sqrt(max(eig, 0)): >= 0, never NaN
        assert np.all(Wh >= 0)
        eig, w_cmp = Wh * Wh, np.maximum(w_ref, 0)
    else:
        eig, w_cmp = Wh, w_ref
    np.testing.assert_allclose(eig, w_cmp, rtol=1e-11, atol=1e-11 * w_ref.max())
    np.testing.assert_allclose(Vh.T @ Vh, np.eye(r), atol=1e-12)
    np.testing.assert_allclose(Vh @ np.diag(eig) @ Vh.T, A, atol=1e-10 * np.abs(A).max())
    assert int(sweeps[0]) < 30
