"""GPU: gp_sobol_replicates (csrc/sobol.hip) against the numpy restatement tests/_sobol_ref.py
under the per-element summation bound computed from the inputs, the bit-level identities between
its four row modes, strided / offset layouts with sentinels, and the public analysis
(gladsgp_amd.sensitivity) on a known answer and on an emulator.
"""
import os

import numpy as np
import pytest
import torch

import _layouts as L
import _sobol_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_ref_d3_m6.npz")
IDENTITY, INDEX, PHILOX, JACKKNIFE = range(4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(N, p, d, seed=0):
    """Correlated outputs (fAB_i near fB, as a Saltelli stack's are), output-major."""
    rng = np.random.default_rng(seed)
    fA = rng.standard_normal((p, N)) + 0.5
    fB = rng.standard_normal((p, N)) + 0.5
    mix = rng.uniform(0.0, 1.0, (d, p, 1))
    fAB = fB[None] + mix * (fA[None] - fB[None]) + 0.05 * rng.standard_normal((d, p, N))
    return fA, fB, fAB


def _t(x, dev, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype)


def _run(dev, fA, fB, fAB, mode, rows=None, pcvar=None, clamp=False, **kw):
    """sobol_replicates on host arrays -> host arrays (first, total, gfirst, gtotal)."""
    from gladsgp_amd import sensitivity as sn
    out = sn.sobol_replicates(_t(fA, dev), _t(fB, dev), _t(fAB, dev), mode,
                              idx=None if rows is None else _t(rows, dev, torch.int32),
                              pcvar=None if pcvar is None else _t(pcvar, dev), clamp=clamp, **kw)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _within(out, want, with_general):
    names = [("first", 0), ("total", 1)] + ([("gfirst", 2), ("gtotal", 3)] if with_general else [])
    for nm, k in names:
        err = np.abs(out[k] - want[nm])
        bound = want["b_" + nm]
        assert np.isfinite(out[k]).all(), nm
        assert (err <= bound).all(), (nm, float(err.max()), float((err / bound).max()))


def _bits(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("N,p,d,n_draw,R", [(256, 8, 8, 256, 67), (100, 3, 1, 99, 5),
                                            (2, 1, 2, 2, 3), (257, 25, 11, 300, 9)])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("general", [False, True])
def test_index_mode_matches_restatement(dev, N, p, d, n_draw, R, clamp, general):
    fA, fB, fAB = _operands(N, p, d, seed=N + d)
    if N == 2:
        fB = fB + 3.0                                  # a replicate of one row keeps a variance
    rng = np.random.default_rng(7)
    rows = rng.integers(0, N, (R, n_draw)).astype(np.int32)
    pcvar = rng.dirichlet(np.ones(p)) if general else None
    want = ref.replicates(fA, fB, fAB, rows, pcvar=pcvar, clamp=clamp)
    out = _run(dev, fA, fB, fAB, INDEX, rows, pcvar=pcvar, clamp=clamp)
    assert out[0].shape == (R, p, d) and out[1].shape == (R, p, d)
    assert (out[2] is None) == (not general)
    _within(out, want, general)
    if clamp:
        assert (out[0] >= 0).all()


def test_identity_equals_index_and_matches_reference_golden(dev):
    g = np.load(GOLDEN)
    fA, fB, fAB = ref.to_output_major(g["fA"], g["fB"], g["fAB"])
    N = fA.shape[1]
    rows = np.arange(N, dtype=np.int32)[None]
    ident = _run(dev, fA, fB, fAB, IDENTITY, pcvar=g["pcvar"])
    _bits(ident, _run(dev, fA, fB, fAB, INDEX, rows, pcvar=g["pcvar"]))
    want = ref.replicates(fA, fB, fAB, rows, pcvar=g["pcvar"])
    for k, (b, theirs) in enumerate((("b_first", "first_order"), ("b_total", "total_index"),
                                     ("b_gfirst", "gen_first_order"),
                                     ("b_gtotal", "gen_total_index"))):
        err = np.abs(ident[k][0] - g[theirs])
        assert (err <= want[b][0]).all(), (theirs, float(err.max()))


def test_jackknife_equals_explicit_rows(dev):
    N, p, d = 100, 3, 5
    fA, fB, fAB = _operands(N, p, d, seed=1)
    pcvar = np.array([0.5, 0.3, 0.2])
    jk = _run(dev, fA, fB, fAB, JACKKNIFE, pcvar=pcvar, clamp=True)
    assert jk[0].shape == (N, p, d)
    _bits(jk, _run(dev, fA, fB, fAB, INDEX, ref.jackknife_rows(N), pcvar=pcvar, clamp=True))


@pytest.mark.parametrize("N", [256, 100])
def test_philox_equals_index_on_rebuilt_rows(dev, N):
    p, d, R, seed, offset = 4, 8, 33, 0x1234_5678_9ABC_DEF1, (5 << 32) | 77
    fA, fB, fAB = _operands(N, p, d, seed=2)
    rows = ref.philox_rows(N, N, R, seed, offset)
    assert rows.min() >= 0 and rows.max() < N
    ph = _run(dev, fA, fB, fAB, PHILOX, R=R, seed=seed, offset=offset, clamp=True)
    _bits(ph, _run(dev, fA, fB, fAB, INDEX, rows, clamp=True))
    other = _run(dev, fA, fB, fAB, PHILOX, R=R, seed=seed, offset=offset + 1, clamp=True)
    assert not np.array_equal(ph[0], other[0])


def test_philox_rows_are_uniform(dev):
    """256 x 1000 draws over N = 100 rows: every row's count within 6 sigma of its binomial mean,
    for the rows the kernel provably used (PHILOX = INDEX on them, bit for bit; n_draw = 1000 is
    also past the rows a lane keeps in registers)."""
    N, p, d, R, M, seed, offset = 100, 1, 1, 256, 1000, 42, 1 << 40
    fA, fB, fAB = _operands(N, p, d, seed=3)
    rows = ref.philox_rows(N, M, R, seed, offset)
    assert rows.min() >= 0 and rows.max() < N
    counts = np.bincount(rows.ravel(), minlength=N)
    mean, sigma = R * M / N, np.sqrt(R * M * (1 / N) * (1 - 1 / N))
    assert (np.abs(counts - mean) <= 6 * sigma).all(), (counts.min(), counts.max(), mean, sigma)
    ph = _run(dev, fA, fB, fAB, PHILOX, R=R, n_draw=M, seed=seed, offset=offset)
    _bits(ph, _run(dev, fA, fB, fAB, INDEX, rows))


def test_global_gather_path(dev):
    from gladsgp_amd import sensitivity as sn
    d, p, R = 8, 2, 16
    N = sn.lds_points(d) + 1
    fA, fB, fAB = _operands(N, p, d, seed=4)
    rng = np.random.default_rng(8)
    rows = rng.integers(0, N, (R, N)).astype(np.int32)
    pcvar = np.array([0.7, 0.3])
    want = ref.replicates(fA, fB, fAB, rows, pcvar=pcvar, clamp=True)
    _within(_run(dev, fA, fB, fAB, INDEX, rows, pcvar=pcvar, clamp=True), want, True)
    # and the largest resident N beside it
    N1 = N - 1
    want = ref.replicates(fA[:, :N1], fB[:, :N1], fAB[:, :, :N1], rows[:, :N1] % N1, pcvar=pcvar)
    _within(_run(dev, fA[:, :N1], fB[:, :N1], fAB[:, :, :N1], INDEX, rows[:, :N1] % N1,
                 pcvar=pcvar), want, True)


def test_out_of_range_rows_are_clamped(dev):
    """The C entry point clamps an index outside [0, N) (the Python wrapper refuses it first)."""
    from gladsgp_amd import _capi, sensitivity as sn
    from gladsgp_amd.kernels import _stream
    N, p, d, R = 50, 2, 3, 4
    fA, fB, fAB = _operands(N, p, d, seed=5)
    rows = np.random.default_rng(1).integers(-20, N + 20, (R, N)).astype(np.int32)
    with pytest.raises(ValueError, match="outside"):
        _run(dev, fA, fB, fAB, INDEX, rows)
    a, b, ab, ix = _t(fA, dev), _t(fB, dev), _t(fAB, dev), _t(rows, dev, torch.int32)
    first = torch.empty((R, p, d), dtype=torch.float64, device=dev)
    total = torch.empty_like(first)
    _capi.call("gp_sobol_replicates", a.data_ptr(), b.data_ptr(), ab.data_ptr(), N, p * N, N, p, d,
               INDEX, ix.data_ptr(), N, N, R, 0, 0, None, 0, first.data_ptr(), total.data_ptr(),
               p * d, None, None, 0, _stream(dev))
    torch.cuda.synchronize()
    _bits((first.cpu().numpy(), total.cpu().numpy()),
          _run(dev, fA, fB, fAB, INDEX, np.clip(rows, 0, N - 1))[:2])


@pytest.mark.parametrize("mode", [INDEX, PHILOX, JACKKNIFE])
def test_layouts(dev, mode):
    """Odd ldf > N, padded strideAB, ldi > n_draw, ldr > p d, ldg > d and 8-byte-offset bases:
    bit-identical to the tight layout, no padding element read (NaN sentinels would poison the
    result) or written (the allocations' bits outside the results are unchanged)."""
    from gladsgp_amd import _capi
    from gladsgp_amd.kernels import _stream
    N, p, d = 100, 3, 5
    R, M = (N, N - 1) if mode == JACKKNIFE else (7, 90)
    fA, fB, fAB = _operands(N, p, d, seed=6)
    pcvar = np.array([0.5, 0.3, 0.2])
    rows = np.random.default_rng(2).integers(0, N, (R, M)).astype(np.int32)
    seed, offset = 11, 5
    tight = _run(dev, fA, fB, fAB, mode, rows if mode == INDEX else None, pcvar=pcvar, clamp=True,
                 **(dict(R=R, n_draw=M, seed=seed, offset=offset) if mode == PHILOX else {}))
    ldf, strideAB, ldi, ldr, ldg = 103, 3 * 103 + 7, M + 3, p * d + 2, d + 3
    eA = L.embed(fA[None], offset=1, ld=ldf, device=dev)
    eB = L.embed(fB[None], offset=3, ld=ldf, device=dev)
    eAB = L.embed(fAB, offset=1, ld=ldf, stride=strideAB, device=dev)
    ePc = L.embed(pcvar[None, None], offset=1, device=dev)
    pad = np.full((R, ldi), -(1 << 30), dtype=np.int32)        # padding: far out of range
    pad[:, :M] = rows
    ix = torch.from_numpy(np.concatenate([[7], pad.ravel()]).astype(np.int32)).to(dev)
    oF = L.blank((1, R, p * d), offset=1, ld=ldr, device=dev)
    oT = L.blank((1, R, p * d), offset=3, ld=ldr, device=dev)
    oGF = L.blank((1, R, d), offset=1, ld=ldg, device=dev)
    oGT = L.blank((1, R, d), offset=1, ld=ldg, device=dev)
    _capi.call("gp_sobol_replicates", eA.ptr, eB.ptr, eAB.ptr, ldf, strideAB, N, p, d, mode,
               ix.data_ptr() + 4 if mode == INDEX else None, ldi, M, R, seed, offset, ePc.ptr, 1,
               oF.ptr, oT.ptr, ldr, oGF.ptr, oGT.ptr, ldg, _stream(dev))
    torch.cuda.synchronize()
    got = (oF.extract()[0].reshape(R, p, d), oT.extract()[0].reshape(R, p, d),
           oGF.extract()[0], oGT.extract()[0])
    _bits(got, tight)
    for e in (eA, eB, eAB, ePc):
        e.check(written=False)
    for o in (oF, oT, oGF, oGT):
        o.check()
    np.testing.assert_array_equal(ix.cpu().numpy()[1:].reshape(R, ldi), pad)


def test_deterministic(dev):
    N, p, d, R = 256, 8, 8, 200
    fA, fB, fAB = _operands(N, p, d, seed=9)
    pcvar = np.full(p, 1.0 / p)
    kw = dict(R=R, seed=3, pcvar=pcvar, clamp=True)
    _bits(_run(dev, fA, fB, fAB, PHILOX, **kw), _run(dev, fA, fB, fAB, PHILOX, **kw))


def test_known_answer_through_the_public_api(dev):
    """f(x) = sum c_i x_i on the unit cube: first = total = c_i^2 / sum c^2 exactly."""
    from gladsgp_amd import sensitivity as sn
    c = np.array([4.0, 2.0, 1.0, 0.5, 0.25])
    exact = c ** 2 / np.sum(c ** 2)
    first, total, res = sn.saltelli_sensitivity_indices(lambda x: (x @ c)[:, None], 5, 10, seed=0,
                                                        n_resamples=999)
    assert first.shape == total.shape == (1, 5)
    assert set(res) == {"first_order", "total_index"}
    print("known answer: max |first - exact|", np.abs(first[0] - exact).max(),
          "max |total - exact|", np.abs(total[0] - exact).max())
    assert (np.abs(first[0] - exact) <= 0.01).all()
    assert (np.abs(total[0] - exact) <= 0.01).all()
    for est, key in ((first, "first_order"), (total, "total_index")):
        ci = res[key].confidence_interval
        assert ci.low.shape == ci.high.shape == (1, 5)
        assert np.isfinite(ci.low).all() and np.isfinite(ci.high).all()
        assert (ci.low <= est).all() and (est <= ci.high).all()
        assert res[key].bootstrap_distribution.shape == (1, 5, 999)
        assert res[key].standard_error.shape == (1, 5)
    # bootstrap=False: the reference's (first, total, None)
    f2, t2, none = sn.saltelli_sensitivity_indices(lambda x: (x @ c)[:, None], 5, 10,
                                                   bootstrap=False, seed=0)
    assert none is None
    np.testing.assert_array_equal(f2, first)
    np.testing.assert_array_equal(t2, total)


def test_sobol_indices_rows_given_or_drawn(dev):
    """sobol_indices with the rows handed over (INDEX) equals the seeded run (PHILOX) on the same
    rows, intervals included; the percentile method brackets its own distribution's median."""
    from gladsgp_amd import sensitivity as sn
    N, p, d, R, seed = 64, 3, 4, 199, 17
    fA, fB, fAB = _operands(N, p, d, seed=10)
    fA, fB, fAB = fA.T, fB.T, np.transpose(fAB, (0, 2, 1))        # the reference's orientation
    pcvar = np.array([0.6, 0.3, 0.1])
    drawn = sn.sobol_indices(fA, fB, fAB, pcvar, n_resamples=R, seed=seed, device=dev).numpy()
    given = sn.sobol_indices(fA, fB, fAB, pcvar, idx=ref.philox_rows(N, N, R, seed),
                             device=dev).numpy()
    np.testing.assert_array_equal(drawn.first_order, given.first_order)
    for name in ("first_order", "total_index", "general_first_order", "general_total_index"):
        a, b = drawn[name], given[name]
        np.testing.assert_array_equal(a.bootstrap_distribution, b.bootstrap_distribution)
        np.testing.assert_array_equal(a.confidence_interval.low, b.confidence_interval.low)
        np.testing.assert_array_equal(a.confidence_interval.high, b.confidence_interval.high)
        assert a.bootstrap_distribution.shape[-1] == R
    pct = sn.sobol_indices(fA, fB, fAB, pcvar, n_resamples=R, seed=seed, method="percentile",
                           device=dev).numpy()
    for name in ("total_index", "general_total_index"):
        med = np.median(pct[name].bootstrap_distribution, axis=-1)
        ci = pct[name].confidence_interval
        assert (ci.low <= med).all() and (med <= ci.high).all() and (ci.low < ci.high).all()
        np.testing.assert_allclose(
            ci.low, np.percentile(pct[name].bootstrap_distribution, 2.5, axis=-1), rtol=1e-12)
    none = sn.sobol_indices(fA, fB, fAB, pcvar, n_resamples=0, device=dev)
    assert none.statistics == {}
    np.testing.assert_array_equal(none.first_order.cpu().numpy(), drawn.first_order)


def _ensemble(n=80, ny=900, d=8, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.random((n, d))
    modes = rng.standard_normal((6, ny)) * (0.5 ** np.arange(6))[:, None]
    coef = np.stack([np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + k) for k in range(6)], 1)
    return t, 3.0 + coef @ modes + 1e-2 * rng.standard_normal((n, ny))


def test_end_to_end_on_an_emulator(dev, tmp_path):
    from gladsgp_amd import model as gm, sensitivity as sn
    t, y = _ensemble()
    d, P, S = t.shape[1], 4, 3
    _, model = gm.init_model(t, y, "sobol", P, data_dir=str(tmp_path), device=dev, verbose=False)
    rng = np.random.default_rng(1)
    samples = {"betaU": rng.uniform(0.2, 3.0, (S, (d + 1) * P)),
               "lamUz": rng.uniform(0.5, 3.0, (S, P)),
               "lamWs": rng.uniform(200, 3000, (S, P)),
               "lamWOs": rng.uniform(50, 500, (S, 1))}
    pcvar = np.array([0.55, 0.25, 0.15, 0.05])
    func = sn.emulator_func(model, samples)
    out = sn.PCA_saltelli_sensitivity_indices(func, d, 5, pcvar, seed=1, n_resamples=200,
                                              batched=True)
    first, total, gfirst, gtotal, res = out
    N = 32
    assert first.shape == total.shape == (P, d) and gfirst.shape == gtotal.shape == (d,)
    assert set(res) == {"first_order", "total_index", "general_first_order",
                        "general_total_index"}
    assert res["first_order"].confidence_interval.low.shape == (P, d)
    assert res["general_total_index"].confidence_interval.high.shape == (d,)
    # the restatement on the same EmulatorPrediction outputs
    A, B = sn.saltelli_design(d, 5, seed=1)
    f = func(sn.saltelli_points(A, B))
    assert f.shape == ((d + 2) * N, P) and f.dtype == np.float64
    f = f.reshape(d + 2, N, P)
    fA, fB, fAB = ref.to_output_major(f[0], f[1], f[2:])
    want = ref.replicates(fA, fB, fAB, np.arange(N)[None], pcvar=pcvar)
    _within((first[None], total[None], gfirst[None], gtotal[None]), want, True)
    one = sn.PCA_saltelli_sensitivity_indices(func, d, 5, pcvar, bootstrap=False, seed=1)
    assert one[4] is None
    for x, z in zip(out[:4], one[:4]):
        np.testing.assert_allclose(z, x, rtol=1e-12, atol=1e-12)
