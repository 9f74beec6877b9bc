"""GPU: gp_sobol_exact (csrc/sobolx.hip), kernels.sobol_exact, sensitivity.exact_indices and
GP.sobol_indices against tests/_sobol_exact_ref.py.

The limit per quantity is the project's rule of 16 x what fp64 itself delivers, in units of the
quantity's positive majorant A (the same sum with |alpha|):
    tiny cases (n <= 24, d <= 3, M <= 2), against the 50-digit truth:
                                                        16 max(|np - truth|, C0 eps A)
    larger cases, against the fp64 restatement:         16 C0 eps A
with C0 = 6 the restatement's own measured error over the tiny cases
(tests/test_sobol_exact_ref_cpu.py::test_restatement_against_truth), not the kernel's.  The index
tolerances are the first-order propagation of those limits through S_i and T_i, computed from the
reference's values (index_tolerance): there is no separate constant.  Every test prints its worst
observed ratio before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _sobol_exact_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
LIM = 16 * R.C0 * EPS
SENT = np.uint64(0x7FF8C0DEC0DEC0DE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def _bits(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


class Strided:
    """``values`` (any rank) at ``offset + sum_i index_i strides_i`` elements of one allocation
    whose every other element -- the gaps, the leading offset and a trailing guard -- holds a NaN
    sentinel: a stray read poisons the result, a stray write shows in :meth:`untouched`."""

    def __init__(self, shape, strides, dev, values=None, offset=0):
        idx = np.full(shape, offset, dtype=np.int64)
        for ax, (sz, st) in enumerate(zip(shape, strides)):
            sh = [1] * len(shape)
            sh[ax] = sz
            idx = idx + (np.arange(sz, dtype=np.int64) * st).reshape(sh)
        assert idx.size == 0 or np.unique(idx).size == idx.size, "overlapping strides"
        self.idx = idx
        size = (int(idx.max()) + 1 if idx.size else offset) + 64
        host = np.full(size, SENT, dtype=np.uint64)
        if values is not None:
            v = np.ascontiguousarray(values, dtype=np.float64).reshape(shape)
            host[idx] = v.view(np.uint64)
        self.initial = host.copy()
        self.buf = torch.from_numpy(host.view(np.float64)).to(dev)
        self.ptr = self.buf.data_ptr() + 8 * offset

    def get(self):
        return self.buf.cpu().numpy()[self.idx]

    def untouched(self):
        now = self.buf.cpu().numpy().view(np.uint64)
        free = np.zeros(now.size, bool)
        free[self.idx.reshape(-1)] = True
        bad = (now != self.initial) & ~free
        assert not bad.any(), f"{int(bad.sum())} elements outside the operand changed, first at " \
                              f"{int(np.flatnonzero(bad)[0])}"


def _raw(dev, X, alpha, beta, s, M, lo=None, hi=None, pad=False):
    """The C call on operands placed with gaps (``pad``: ldx > d, lda > n, ldbeta > d, incE > 1,
    padded ldq / ldqa / ldqg, every buffer off its allocation's start) or tightly; sentinels in
    every gap, checked untouched.  Returns (E (U,), Q (G, M, M, 2 d + 1)) as numpy."""
    from gladsgp_amd import _capi
    lib = _capi.lib()
    n, d = X.shape
    U = alpha.shape[0]
    G = U // M
    nq = 2 * d + 1
    g = 1 if pad else 0
    ldx, lda, ldb, incE = d + 3 * g, n + 5 * g, d + 2 * g, 1 + 2 * g
    ldq = nq + 4 * g
    ldqa = M * ldq + 3 * g
    ldqg = M * ldqa + 7 * g
    Xe = Strided((n, d), (ldx, 1), dev, X, offset=3 * g)
    Ae = Strided((U, n), (lda, 1), dev, alpha, offset=g)
    Be = Strided((U, d), (ldb, 1), dev, beta, offset=5 * g)
    Ee = Strided((U,), (incE,), dev, offset=2 * g)
    Qe = Strided((G, M, M, nq), (ldqg, ldqa, ldq, 1), dev, offset=9 * g)
    se = _t(s, dev)
    loe = None if lo is None else _t(lo, dev)
    hie = None if hi is None else _t(hi, dev)
    nbytes = lib.gp_sobol_exact_ws_bytes(n, d, G, M)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    rc = lib.gp_sobol_exact(Xe.ptr, n, d, ldx, G, M, Ae.ptr, lda, Be.ptr, ldb, se.data_ptr(),
                            None if loe is None else loe.data_ptr(),
                            None if hie is None else hie.data_ptr(), Ee.ptr, incE, Qe.ptr, ldq,
                            ldqa, ldqg, ws.data_ptr(), nbytes,
                            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for op in (Xe, Ae, Be, Ee, Qe):
        op.untouched()
    for op, v in ((Xe, X), (Ae, alpha), (Be, beta)):          # the inputs are intact
        _bits(op.get(), np.ascontiguousarray(v, dtype=np.float64))
    E, Q = Ee.get(), Qe.get()
    assert np.isfinite(E).all() and np.isfinite(Q).all(), "a sentinel reached the result"
    return E, Q


def _call(dev, X, alpha, beta, s, M, lo=None, hi=None):
    from gladsgp_amd import kernels
    E, Q = kernels.sobol_exact(_t(X, dev), _t(alpha, dev), _t(beta, dev), _t(s, dev), group=M,
                               lo=None if lo is None else _t(lo, dev),
                               hi=None if hi is None else _t(hi, dev))
    return E.cpu().numpy(), Q.cpu().numpy()


def _check(tag, E, Q, ref, limE, limQ):
    """|E - ref| <= limE and |Q - ref| <= limQ elementwise (limits in absolute units); prints the
    worst observed error over the limit and in units of eps A first."""
    eE, eQ = np.abs(E - ref["E"]), np.abs(Q - ref["Q"])
    AE, AQ = R.to_float(ref["AE"]), R.to_float(ref["AQ"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rE = np.nanmax(np.where(limE > 0, eE / limE, np.where(eE > 0, np.inf, 0.0)))
        rQ = np.nanmax(np.where(limQ > 0, eQ / limQ, np.where(eQ > 0, np.inf, 0.0)))
        uE = np.nanmax(np.where(AE > 0, eE / (EPS * AE), 0.0))
        uQ = np.nanmax(np.where(AQ > 0, eQ / (EPS * AQ), 0.0))
    print(f"{tag}: E err {uE:.2f} eps A ({rE:.3f} of the limit), Q err {uQ:.2f} eps A "
          f"({rQ:.3f} of the limit)")
    assert rE <= 1.0 and rQ <= 1.0, (tag, float(rE), float(rQ))
    _bits(Q, np.ascontiguousarray(np.swapaxes(Q, 1, 2)))     # both triangles, the same bits


@functools.lru_cache(maxsize=None)
def _tiny(regime, n, d, G, M):
    X, beta, s, alpha, lo, hi = R.make_case(n, d, G * M, regime, 0)
    tr = R.mp_moments(X, alpha, beta, s, M, lo, hi)
    ref = R.np_moments(X, alpha, beta, s, M, lo, hi)
    return (X, beta, s, alpha, lo, hi), tr, ref


# ------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("n,d,G,M", R.TINY_CASES)
def test_tiny_cases_against_the_truth(dev, regime, n, d, G, M):
    """n <= 24, d <= 3, M <= 2 in every regime against the 50-digit truth:
    16 max(the restatement's own error, C0 eps A) per quantity."""
    (X, beta, s, alpha, lo, hi), tr, ref = _tiny(regime, n, d, G, M)
    E, Q = _raw(dev, X, alpha, beta, s, M, lo, hi, pad=(n % 2 == 1))
    AE, AQ = R.to_float(tr["AE"]), R.to_float(tr["AQ"])
    limE = 16 * np.maximum(R.abs_err(ref["E"], tr["E"]), R.C0 * EPS * AE)
    limQ = 16 * np.maximum(R.abs_err(ref["Q"], tr["Q"]), R.C0 * EPS * AQ)
    truth = dict(E=R.to_float(tr["E"]), Q=R.to_float(tr["Q"]), AE=AE, AQ=AQ)
    # the truth rounded to fp64 is within eps/2 |truth| <= eps/2 A of itself: well inside the limit
    _check(f"tiny {regime} n={n} d={d} G={G} M={M}", E, Q, truth, limE, limQ)


# every n of {1, 7, 64, 65, 129, 200}, every d of {1, 3, 8, 17, 32} (32 only with n <= 65), every
# (G, M) of {(1,1), (3,1), (1,2), (2,5)}, padded and tight layouts
LARGER = [(200, 8, 2, 5, True), (129, 3, 3, 1, False), (65, 32, 1, 2, True), (64, 17, 1, 1, False),
          (7, 1, 2, 5, True), (1, 8, 1, 2, False), (65, 17, 3, 1, True), (129, 8, 1, 2, True),
          (64, 32, 1, 1, False), (200, 3, 1, 1, True), (1, 1, 1, 1, True)]


@pytest.mark.parametrize("n,d,G,M,pad", LARGER)
def test_larger_shapes_against_the_restatement(dev, n, d, G, M, pad):
    """Tile-straddling n, both dimension paths (d <= 8 and above), grouped and single units,
    padded strides with sentinels in every gap: 16 C0 eps A per quantity."""
    X, beta, s, alpha, lo, hi = R.make_case(n, d, G * M, "plain", 1)
    ref = R.np_moments(X, alpha, beta, s, M)
    E, Q = _raw(dev, X, alpha, beta, s, M, pad=pad)
    _check(f"n={n} d={d} G={G} M={M}", E, Q, ref, LIM * ref["AE"], LIM * ref["AQ"])


@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("regime", [r for r in R.REGIMES if r != "plain"])
def test_regimes(dev, regime, d):
    """Each regime at the tile-straddling n = 65, two units of one group, on both dimension
    paths.  flat: V -> 0, only E and Q are held to the limit.  sharp: J_0 underflows for most
    point pairs and every Q_not_i must still be finite and within the limit (a quotient by J_i
    gives 0/0 here).  subbox: same-sign brackets.  widebox.  mixed: beta apart by 1e4."""
    n, M = 65, 2
    X, beta, s, alpha, lo, hi = R.make_case(n, d, M, regime, 2)
    ref = R.np_moments(X, alpha, beta, s, M, lo, hi)
    E, Q = _raw(dev, X, alpha, beta, s, M, lo, hi, pad=True)
    assert np.isfinite(Q).all()
    if regime == "sharp":
        J0 = R.np_two_point(X, beta[0], beta[1], np.zeros(d), np.ones(d))[..., 0]
        # exp(-5000 (a - a')^2) is 0 in fp64 beyond |a - a'| = 0.386: 38 % of uniform pairs
        assert (J0 == 0).mean() > 0.3, "the case must underflow J_0 for a large share of pairs"
        assert (np.abs(Q[..., 1 + d:]) > 0).all()
    _check(f"{regime} d={d}", E, Q, ref, LIM * ref["AE"], LIM * ref["AQ"])


# -------------------------------------------------------------------------------- indices
@pytest.mark.parametrize("n,d,G,M", [(65, 3, 2, 1), (129, 8, 1, 2), (64, 17, 1, 1), (40, 1, 1, 2)])
def test_indices(dev, n, d, G, M):
    """Well-conditioned GPs (beta in [0.5, 5], delta = 1e-4): S_i and T_i against the reference
    within the first-order propagation of the E and Q limits; sum_i S_i <= 1, S_i <= T_i; d = 1
    gives 1."""
    from gladsgp_amd import sensitivity
    X, beta, s, alpha = R.conditioned_case(n, d, G * M, seed=3)
    ref = R.np_moments(X, alpha, beta, s, M)
    E, Q = _call(dev, X, alpha, beta, s, M)
    _check(f"conditioned n={n} d={d}", E, Q, ref, LIM * ref["AE"], LIM * ref["AQ"])
    _, V, first, total = sensitivity.indices_from_moments(E.reshape(G, M), Q)
    _, Vr, fr, tr = R.np_indices(ref["E"], ref["Q"], M)
    tf, tt = R.index_tolerance(ref, M, LIM)
    print(f"n={n} d={d}: V {Vr} worst |dS| / tol {np.max(np.abs(first - fr) / tf):.3f} "
          f"|dT| / tol {np.max(np.abs(total - tr) / tt):.3f} "
          f"(tol <= {max(tf.max(), tt.max()):.1e})")
    assert (Vr > 0).all() and max(tf.max(), tt.max()) < 1e-6, "the case must be well conditioned"
    assert (np.abs(first - fr) <= tf).all() and (np.abs(total - tr) <= tt).all()
    assert (first.sum(-1) <= 1 + tf.sum(-1)).all()
    assert (first <= total + tf + tt).all()
    if d == 1:
        assert (np.abs(first - 1) <= tf).all() and (np.abs(total - 1) <= tt).all()


# ----------------------------------------------------------------------------------- bits
def test_bit_identities(dev):
    """Q(a,b) = Q(b,a); the (a,a) entries of an M = 5 call are the M = 1 call's; a unit's E and Q
    do not depend on G, on its position or on the strides; two runs agree."""
    n, d, U = 129, 8, 10
    X, beta, s, alpha, _, _ = R.make_case(n, d, U, "plain", 5)
    E5, Q5 = _call(dev, X, alpha, beta, s, 5)                # G = 2, M = 5
    E5b, Q5b = _call(dev, X, alpha, beta, s, 5)
    _bits(E5, E5b)
    _bits(Q5, Q5b)
    _bits(Q5, np.ascontiguousarray(np.swapaxes(Q5, 1, 2)))
    E1, Q1 = _call(dev, X, alpha, beta, s, 1)                # G = 10, M = 1
    _bits(E1, E5)
    _bits(Q1[:, 0, 0], Q5[:, np.arange(5), np.arange(5)].reshape(U, -1))
    # padded strides, and the M = 10 grouping: the same pairs, the same bits
    Ep, Qp = _raw(dev, X, alpha, beta, s, 5, pad=True)
    _bits(Ep, E5)
    _bits(Qp, Q5)
    E10, Q10 = _call(dev, X, alpha, beta, s, 10)
    _bits(E10, E5)
    _bits(Q10[0, :5, :5], Q5[0])
    _bits(Q10[0, 5:, 5:], Q5[1])
    # units 3..4 and 7 alone, at other positions of other batches
    Es, Qs = _call(dev, X, alpha[3:5], beta[3:5], s[3:5], 2)
    _bits(Es, E5[3:5])
    _bits(Qs[0], Q5[0, 3:5, 3:5])
    Es, Qs = _call(dev, X, alpha[[7, 2, 7]], beta[[7, 2, 7]], s[[7, 2, 7]], 1)
    _bits(Es, E5[[7, 2, 7]])
    _bits(Qs[[0, 2], 0, 0], np.stack([Q5[1, 2, 2], Q5[1, 2, 2]]))
    # d > 8: the chunked path
    X, beta, s, alpha, _, _ = R.make_case(65, 17, 4, "plain", 6)
    E2, Q2 = _call(dev, X, alpha, beta, s, 2)
    E1, Q1 = _call(dev, X, alpha, beta, s, 1)
    _bits(E1, E2)
    _bits(Q1[:, 0, 0], Q2[:, np.arange(2), np.arange(2)].reshape(4, -1))
    _bits(Q2, np.ascontiguousarray(np.swapaxes(Q2, 1, 2)))


def test_empty_sizes(dev):
    """n = 0: E and Q are written as 0 (the strided elements only).  G = 0: nothing is written."""
    from gladsgp_amd import kernels
    E, Q = _raw(dev, np.zeros((0, 3)), np.zeros((4, 0)), np.ones((4, 3)), np.ones(4), 2, pad=True)
    assert (E == 0).all() and (Q == 0).all() and Q.shape == (2, 2, 2, 7)
    X = torch.zeros((5, 3), dtype=torch.float64, device=dev)
    E, Q = kernels.sobol_exact(X, torch.zeros((0, 5), dtype=torch.float64, device=dev),
                               torch.zeros((0, 3), dtype=torch.float64, device=dev),
                               torch.zeros(0, dtype=torch.float64, device=dev))
    assert E.shape == (0,) and Q.shape == (0, 1, 1, 7)


def test_graph_capture(dev):
    """gp_sobol_exact captured on a side stream and replayed once: the bits of the eager call."""
    from gladsgp_amd import kernels
    X, beta, s, alpha, _, _ = R.make_case(129, 8, 4, "plain", 7)
    Xd, ad, bd, sd = _t(X, dev), _t(alpha, dev), _t(beta, dev), _t(s, dev)
    E = torch.empty(4, dtype=torch.float64, device=dev)
    Q = torch.empty((2, 2, 2, 17), dtype=torch.float64, device=dev)
    kernels.sobol_exact(Xd, ad, bd, sd, group=2, out=(E, Q))     # eager (workspace allocated)
    torch.cuda.synchronize()
    wantE, wantQ = E.clone(), Q.clone()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        kernels.sobol_exact(Xd, ad, bd, sd, group=2, out=(E, Q))
    E.zero_()
    Q.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _bits(E, wantE)
    _bits(Q, wantQ)


# -------------------------------------------------------------------------------- surface
@pytest.fixture(scope="module")
def small(dev):
    from gladsgp_amd import emulator as em
    e = R.small_emulator()
    data = em.EmulatorData(e["t"], e["y"], device=dev)
    data.standardize_y()
    data.create_K_basis(e["K"])
    return em.EmulatorModel(data), e


def _surface_reference(model, e, M):
    """The restatement fed the device's own gp_params / alpha, units grouped by PC."""
    from gladsgp_amd import response
    S, P = e["S"], e["P"]
    alpha, beta, s, S_, P_ = response.unit_alpha(model, e["samples"])
    assert (S_, P_) == (S, P)
    X = model.data.sim_data.t_dev.cpu().numpy()
    g = lambda a: R.group_by_pc(a.cpu().numpy(), S, P)       # noqa: E731
    return R.np_moments(X, g(alpha), g(beta), g(s), M)


def test_exact_indices_mean_mode(dev, small):
    from gladsgp_amd import sensitivity
    model, e = small
    S, P, d = e["S"], e["P"], e["d"]
    res = sensitivity.exact_indices(model, e["samples"], pcvar=e["pcvar"])
    assert res.average == "mean" and res.first_order.device.type == "cuda"
    h = res.numpy()
    assert h.first_order.shape == (P, d) and h.total_index.shape == (P, d)
    assert h.mean.shape == (P,) and h.variance.shape == (P,)
    assert h.general_first_order.shape == (d,) and h.general_total_index.shape == (d,)
    ref = _surface_reference(model, e, S)
    Eb, V, fr, tr = R.np_indices(ref["E"], ref["Q"], S)
    tf, tt = R.index_tolerance(ref, S, LIM)
    print(f"mean mode: S {fr.tolist()} T {tr.tolist()} tol <= {max(tf.max(), tt.max()):.1e}; "
          f"|dS| / tol {np.max(np.abs(h.first_order - fr) / tf):.3f} "
          f"|dT| / tol {np.max(np.abs(h.total_index - tr) / tt):.3f}")
    assert (np.abs(h.first_order - fr) <= tf).all() and (np.abs(h.total_index - tr) <= tt).all()
    dE = LIM * ref["AE"].reshape(P, S).mean(-1)
    assert (np.abs(h.mean - Eb) <= dE).all()
    assert (np.abs(h.variance - V) <= LIM * ref["AQ"].reshape(P, S, S, -1).mean((1, 2))[:, 0] +
            2 * np.abs(Eb) * dE).all()
    # general indices: sum_p pcvar_p index_p, from the device's own values
    np.testing.assert_allclose(h.general_first_order, e["pcvar"] @ h.first_order, rtol=4 * EPS)
    np.testing.assert_allclose(h.general_total_index, e["pcvar"] @ h.total_index, rtol=4 * EPS)
    np.testing.assert_array_equal(h.interaction, h.total_index - h.first_order)
    none = sensitivity.exact_indices(model, e["samples"], group=3)
    assert none.general_first_order is None and none.general_total_index is None
    _bits(none.first_order, res.first_order)         # the factorisation's grouping: no effect
    with pytest.raises(ValueError, match="^interval"):
        res.interval()


def test_exact_indices_sample_mode(dev, small):
    from gladsgp_amd import sensitivity
    model, e = small
    S, P, d = e["S"], e["P"], e["d"]
    res = sensitivity.exact_indices(model, e["samples"], pcvar=e["pcvar"], average="sample")
    h = res.numpy()
    assert h.first_order.shape == (S, P, d) and h.total_index.shape == (S, P, d)
    assert h.mean.shape == (S, P) and h.general_first_order.shape == (S, d)
    ref = _surface_reference(model, e, 1)
    _, _, fr, tr = R.np_indices(ref["E"], ref["Q"], 1)        # units (j, a)
    tf, tt = R.index_tolerance(ref, 1, LIM)
    sp = lambda a: np.swapaxes(a.reshape(P, S, d), 0, 1)     # noqa: E731
    assert (np.abs(h.first_order - sp(fr)) <= sp(tf)).all()
    assert (np.abs(h.total_index - sp(tr)) <= sp(tt)).all()
    # every entry equals the call on that posterior sample alone
    for a in (0, S - 1):
        one = {k: v[a:a + 1] for k, v in e["samples"].items()}
        r1 = sensitivity.exact_indices(model, one, pcvar=e["pcvar"], average="sample")
        _bits(r1.first_order[0], res.first_order[a])
        _bits(r1.total_index[0], res.total_index[a])
        _bits(r1.general_total_index[0], res.general_total_index[a])
        rm = sensitivity.exact_indices(model, one, average="mean")      # S = 1: the same function
        _bits(rm.first_order, res.first_order[a])
    np.testing.assert_allclose(h.general_first_order,
                               np.einsum("p,spd->sd", e["pcvar"], h.first_order), rtol=4 * EPS)
    # the band over the posterior samples
    iv = res.interval(0.9)
    assert set(iv) == {"first_order", "total_index", "general_first_order", "general_total_index"}
    for name, ci in iv.items():
        v = getattr(h, name)
        np.testing.assert_allclose(ci.low.cpu().numpy(), np.quantile(v, 0.05, axis=0),
                                   rtol=8 * EPS, atol=8 * EPS)
        np.testing.assert_allclose(ci.high.cpu().numpy(), np.quantile(v, 0.95, axis=0),
                                   rtol=8 * EPS, atol=8 * EPS)


def test_exact_indices_on_a_sub_box(dev, small):
    from gladsgp_amd import sensitivity
    model, e = small
    S = e["S"]
    lo, hi = np.array([0.2, 0.0, 0.3]), np.array([0.7, 1.0, 0.9])
    res = sensitivity.exact_indices(model, e["samples"], lo=lo, hi=hi).numpy()
    from gladsgp_amd import response
    alpha, beta, s, _, P = response.unit_alpha(model, e["samples"])
    g = lambda a: R.group_by_pc(a.cpu().numpy(), S, P)       # noqa: E731
    ref = R.np_moments(model.data.sim_data.t_dev.cpu().numpy(), g(alpha), g(beta), g(s), S, lo, hi)
    _, _, fr, tr = R.np_indices(ref["E"], ref["Q"], S)
    tf, tt = R.index_tolerance(ref, S, LIM)
    assert (np.abs(res.first_order - fr) <= tf).all() and (np.abs(res.total_index - tr) <= tt).all()
    with pytest.raises(ValueError, match="^lo, hi"):
        sensitivity.exact_indices(model, e["samples"], lo=0.5, hi=0.5)


def test_saltelli_consistency(dev, small):
    """A check against a sign or definition slip, not an accuracy test: every exact index lies
    within 6 bootstrap standard errors of the Saltelli estimate of the same function from the
    seeded design (tests/test_sobol_exact_ref_cpu.py shows the references alone meeting the
    margin for this seed)."""
    from gladsgp_amd import sensitivity
    model, e = small
    first, total, gfirst, gtotal, res = sensitivity.PCA_saltelli_sensitivity_indices(
        sensitivity.emulator_func(model, e["samples"], cast=None), e["d"], R.SALTELLI_M,
        e["pcvar"], seed=R.SALTELLI_SEED, n_resamples=R.SALTELLI_RESAMPLES)
    ex = sensitivity.exact_indices(model, e["samples"], pcvar=e["pcvar"]).numpy()
    for name, est in (("first_order", first), ("total_index", total),
                      ("general_first_order", gfirst), ("general_total_index", gtotal)):
        z, ok = R.within_margin(getattr(ex, name), est, res[name].standard_error)
        print(f"{name}: exact {np.round(getattr(ex, name), 4).tolist()} estimate "
              f"{np.round(est, 4).tolist()} worst z {z.max():.2f}")
        assert ok, (name, z)


def test_gp_sobol_indices(dev):
    """GP.sobol_indices on the C1 toy (n = 64, d = 1, nugget 1e-3): one unit through
    _kernel_params, against the reference fed the same alpha; d = 1 gives 1.  And an ARD fit of
    a two-dimensional toy on a sub-box."""
    from gladsgp_amd import gpmodule as GPmodule
    from gladsgp_amd import kernels
    x = np.vstack(np.linspace(1 / 8, 7 / 8, 64))
    y = x * np.sin(2 * np.pi * x)
    gp = GPmodule.GP(covariance=GPmodule.squared_exponential, cov_para={"nugget": 1e-3},
                     device=dev)
    gp.fit(x, y, np.array([1.0, 0.5]), jac=True)

    def reference(gp, lo=None, hi=None):
        alpha = kernels.alpha(gp._chol, gp._y).cpu().numpy()
        ref = R.np_moments(gp._x, alpha, gp._beta.cpu().numpy(), np.array([gp._s]), 1, lo, hi)
        _, V, fr, tr = R.np_indices(ref["E"], ref["Q"], 1)
        tf, tt = R.index_tolerance(ref, 1, LIM)
        return V, fr[0], tr[0], tf[0], tt[0]

    first, total = gp.sobol_indices()
    V, fr, tr, tf, tt = reference(gp)
    print(f"C1: theta {gp.theta} V {V} S {first} T {total} tol {tf} {tt}")
    assert first.shape == (1,) and total.shape == (1,)
    assert np.abs(first - fr) <= tf and np.abs(total - tr) <= tt
    assert np.abs(first - 1) <= tf and np.abs(total - 1) <= tt
    rng = np.random.default_rng(2)
    x2 = rng.random((40, 2))
    y2 = np.sin(3 * x2[:, 0]) + 0.3 * x2[:, 1] ** 2 + 0.2 * x2[:, 0] * x2[:, 1]
    gp2 = GPmodule.GP(covariance=GPmodule.squared_exponential, cov_para={"nugget": 1e-2},
                      device=dev, ard=True)
    gp2.fit(x2, y2, np.array([1.0, 0.5, 0.5]), jac=True)
    lo, hi = np.array([0.1, 0.2]), np.array([0.9, 0.7])
    first, total = gp2.sobol_indices(lo=lo, hi=hi)
    V, fr, tr, tf, tt = reference(gp2, lo, hi)
    print(f"ARD: theta {gp2.theta} V {V} S {first} T {total} tol {tf} {tt}")
    assert (np.abs(first - fr) <= tf).all() and (np.abs(total - tr) <= tt).all()
    assert first[0] > first[1] and (first <= total + tf + tt).all()
