"""GPU: gp_nll_grad (csrc/nllgrad.hip), kernels.nll_grad and kernels.nll_value_grad.

Accuracy is measured against the 50-digit gradient of tests/_nll_grad_ref.py as
max_e |g - truth|_e / G_e (G the gross sums: the gradient itself cancels to zero at an optimum)
and held to that module's limit: 16 x the larger error of the LAPACK and the blocked
explicit-inverse fp64 restatements against the same truth, floor 4 eps.  Everything else is bit
for bit: repeated runs, a problem alone against the same problem inside a batch, a buffer whose
never-named elements hold NaN, and strided / offset / gapped layouts.
"""
import os

import numpy as np
import pytest
import torch

import _layouts as L
import _nll_grad_ref as R
from _mp_ref import DD, EPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


def _factor(dev, X, beta, s, delta):
    """beta (batch, d), s, delta (batch,) -> Cholesky of the batch on the device."""
    from gladsgp_amd import kernels
    ch = kernels.cholesky_inverse(kernels.gram(_t(X, dev), _t(beta, dev), _t(s, dev),
                                               _t(delta, dev), batch=len(s)))
    assert (ch.info == 0).all()
    return ch


def _grad(dev, X, beta, s, delta, w):
    from gladsgp_amd import kernels
    ch = _factor(dev, X, beta, s, delta)
    return kernels.nll_grad(ch, _t(X, dev), _t(beta, dev), _t(s, dev), _t(w, dev)).cpu().numpy()


def _batch3(n, d):
    """Three problems on one scattered design with their own beta, s, delta and w; the first has
    s = 0.7 and delta = 1e-2."""
    X, beta0, _, _, w0 = R.scattered(n, d, 0.7, 1e-2, 1000 + 37 * n + d)
    rng = np.random.default_rng(n + 100 * d)
    beta = np.stack([beta0, rng.uniform(0.5, 5.0, d), rng.uniform(0.5, 5.0, d)])
    w = np.stack([w0, R.c2_w(X, 7), np.cos(3.0 * X @ rng.random(d))])
    return X, beta, np.array([0.7, 1.05, 0.4]), np.array([1e-2, 3e-3, 2.5e-2]), w


SHAPES = [(n, 8) for n in (1, 2, 15, 16, 63, 64)] + \
         [(n, d) for n in (17, 65) for d in (1, 8, 9, 32)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_against_the_truth(dev, n, d):
    X, beta, s, delta, w = _batch3(n, d)
    got = _grad(dev, X, beta, s, delta, w)
    assert got.shape == (3, d + 2)
    worst = []
    for b in range(3):
        inp = (X, beta[b], s[b], delta[b], w[b])
        g, G = R.truth(*inp)
        lim = R.limit(*inp, g, G)
        r = R.ratio(got[b], g, G)
        print(f"n={n} d={d} b={b}: ratio {r / EPS:.2f} eps, limit {lim / EPS:.1f} eps")
        worst.append((r, lim))
    for r, lim in worst:
        assert r <= lim


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_against_the_golden_truth(dev, golden_dir, name):
    """n = 130, 200, 321: several tiles per side, a ragged last tile, k-ranges of every length."""
    z = np.load(os.path.join(golden_dir, "nll_grad_truth.npz"))
    X, beta, s, delta, w = R.golden_inputs(name)
    g = DD.__new__(DD)
    g.hi, g.lo = z[name + "_g_hi"], z[name + "_g_lo"]
    lim = R.limit_from(float(z[name + "_lapack"]), float(z[name + "_explicit"]))
    got = _grad(dev, X, beta[None], np.array([s]), np.array([delta]), w[None])
    r = R.ratio(got[0], g, z[name + "_G"])
    print(f"{name}: ratio {r / EPS:.2f} eps, limit {lim / EPS:.1f} eps")
    assert r <= lim


def test_c1_grid_near_its_optimum(dev):
    """BASELINE config 1 at theta = [1.436, 0.3926] (kappa-limited: the LAPACK restatement is
    5e5 eps of G off there), against its own limit."""
    inp = R.c1_grid()
    X, beta, s, delta, w = inp
    g, G = R.truth(*inp)
    lim = R.limit(*inp, g, G)
    got = _grad(dev, X, beta[None], np.array([s]), np.array([delta]), w[None])
    r = R.ratio(got[0], g, G)
    print(f"c1 grid: ratio {r / EPS:.4g} eps, limit {lim / EPS:.4g} eps, "
          f"ratio / limit {r / lim:.3f}")
    assert r <= lim


# ------------------------------------------------------------------------------------ bitwise
NB, DB, BATCH = 200, 8, 5


@pytest.fixture(scope="module")
def five(dev):
    from gladsgp_amd import kernels
    X = np.random.default_rng(5).random((NB, DB))
    rng = np.random.default_rng(6)
    beta = rng.uniform(0.5, 5.0, (BATCH, DB))
    s, delta = rng.uniform(0.5, 2.0, BATCH), rng.uniform(1e-3, 1e-1, BATCH)
    w = np.stack([R.c2_w(X, 20 + b) for b in range(BATCH)])
    ch = _factor(dev, X, beta, s, delta)
    ops = dict(X=_t(X, dev), beta=_t(beta, dev), s=_t(s, dev), w=_t(w, dev))
    ops["alpha"] = kernels.alpha(ch, ops["w"])
    base = kernels.nll_grad(ch, ops["X"], ops["beta"], ops["s"], ops["w"], ops["alpha"])
    assert torch.isfinite(base).all()
    return ch, ops, base


def test_same_inputs_same_bits(dev, five):
    from gladsgp_amd import kernels
    ch, o, base = five
    again = kernels.nll_grad(ch, o["X"], o["beta"], o["s"], o["w"], o["alpha"])
    assert torch.equal(again, base)
    assert torch.equal(kernels.nll_grad(ch, o["X"], o["beta"], o["s"], o["w"]), base)


@pytest.mark.parametrize("b", [0, 3])
def test_alone_equals_in_batch(dev, five, b):
    from gladsgp_amd import kernels
    ch, o, base = five
    one = kernels.Cholesky(ch.n, ch.a_buf[b:b + 1].contiguous(),
                           ch.linv_buf[b:b + 1].contiguous(), ch.info[b:b + 1],
                           ch.logdet[b:b + 1])
    got = kernels.nll_grad(one, o["X"], o["beta"][b:b + 1].contiguous(),
                           o["s"][b:b + 1].contiguous(), o["w"][b:b + 1].contiguous(),
                           o["alpha"][b:b + 1].contiguous())
    assert torch.equal(got[0], base[b])


def test_unnamed_elements_are_never_used(dev, five):
    """The strict upper triangle, the padding rows and the padding columns of L^-1 filled with
    NaN: the bits of the zeroed buffer."""
    from gladsgp_amd import kernels
    ch, o, base = five
    npad = ch.linv_buf.shape[1]
    buf = ch.linv_buf.clone()                       # [b, col, row]
    col = torch.arange(npad, device=dev)[:, None]
    row = torch.arange(npad, device=dev)[None, :]
    named = (row >= col) & (row < NB) & (col < NB)
    buf[:, ~named] = float("nan")
    poisoned = kernels.Cholesky(ch.n, ch.a_buf, buf, ch.info, ch.logdet)
    got = kernels.nll_grad(poisoned, o["X"], o["beta"], o["s"], o["w"], o["alpha"])
    assert torch.equal(got, base)


def _raw(dev, Li, Xe, Be, s, Ae, Ge, n, d, batch):
    from gladsgp_amd import _capi
    lib = _capi.lib()
    ws = torch.empty(max(lib.gp_nll_grad_ws_bytes(n, d, batch), 256), dtype=torch.uint8,
                     device=dev)
    rc = lib.gp_nll_grad(Li.ptr, Li.ld, Li.stride, Xe.ptr, Xe.ld, n, d, Be.ptr, Be.stride,
                         s.data_ptr(), Ae.ptr, Ae.stride, Ge.ptr, Ge.stride, batch,
                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc


@pytest.mark.parametrize("case", ["odd_ld", "off8", "off16", "odd_stride", "gap16"])
def test_layouts(dev, five, case):
    """Strided, offset and gapped L^-1, X, beta, alpha and grad: the bits of the tight call,
    nothing outside grad's d + 2 values written, no padding read (the sentinels are NaN)."""
    ch, o, base = five
    Li = L.place(ch.linv_buf.cpu().numpy(), case, device=dev, track=False)
    Xe = L.place(o["X"].cpu().numpy()[None], case, device=dev)
    Be = L.place(o["beta"].cpu().numpy()[:, None, :], case, device=dev)
    Ae = L.place(o["alpha"].cpu().numpy()[:, None, :], case, device=dev)
    Ge = L.blank_case((BATCH, 1, DB + 2), case, device=dev)
    assert _raw(dev, Li, Xe, Be, o["s"], Ae, Ge, NB, DB, BATCH) == 0
    got = Ge.extract()[:, 0, :]
    assert np.array_equal(got.view(np.uint64), base.cpu().numpy().view(np.uint64))
    Ge.check()
    for e in (Xe, Be, Ae):
        e.check(written=False)


def test_value_grad_marks_a_non_positive_definite_problem(dev):
    """A negative delta (K not positive definite) gives NaN in its row and its info; its batch
    neighbours have the bits they have beside a valid problem."""
    from gladsgp_amd import kernels
    X, beta, s, delta, w = _batch3(65, 8)
    ops = [_t(a, dev) for a in (X, beta, s)]
    good = kernels.nll_value_grad(*ops, _t(delta, dev), _t(w, dev))
    bad_delta = delta.copy()
    bad_delta[1] = -1.2                              # s + delta < 0: the first pivot fails
    val, grad, info = kernels.nll_value_grad(*ops, _t(bad_delta, dev), _t(w, dev))
    assert info.tolist()[0] == 0 and info.tolist()[2] == 0 and info.tolist()[1] > 0
    assert torch.isnan(val[1]) and torch.isnan(grad[1]).all()
    for b in (0, 2):
        assert torch.equal(val[b], good[0][b]) and torch.equal(grad[b], good[1][b])
    assert (good[2] == 0).all() and torch.isfinite(good[1]).all()
    # the value is gp_nll's and the gradient is the truth's
    inp = (X, beta[0], s[0], delta[0], w[0])
    g, G = R.truth(*inp)
    assert R.ratio(grad[0].cpu().numpy(), g, G) <= R.limit(*inp, g, G)
    # kappa(K) <= (n s + delta) / delta < 1e4: both values are good to 1e-12, so 1e-9 only
    # tells gp_nll's quantity from another
    ref = R.grad_lapack(*inp)[0]
    assert abs(float(val[0]) - ref) <= 1e-9 * max(1.0, abs(ref))
