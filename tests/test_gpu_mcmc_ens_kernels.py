"""GPU: the ensemble forms of the Metropolis group kernels (gp_mcmc_ens_prep, _decide, _step)
called directly.  Chain c of a call must be what gp_mcmc_group_* gives for that chain alone: the
numpy restatement tests/_mcmc_group_ref.py is run once per chain, and every chain's buffers are
compared with it by test_gpu_mcmc_group.py's own comparison (bit for bit where that file says so;
through exp / log / log1p within its documented margins: 16, 40 for dlp, 360 for lp, times e_ref,
plus 4 ulp; the same input conditions, asserted on the restatement alone).  ``ll_all`` is drawn
by the test, so no factorisation runs: a case is a few launches of C workgroups.

Layouts.  Every buffer of gp_mcmc_state holds the C chains at its stride between two guard bands:
  packed   stride = the buffer's per-chain extent;
  padded   stride = extent + PAD, the PAD doubles between chains filled with the guard pattern;
  shared   packed, but lam and the four step buffers have stride 0 (one copy for all chains).
beta / s / delta / ll_all are chain-major as the header lays them out.  A chain's image is cut out
of these buffers and checked as if it were alone, which also shows that no other chain wrote into
it; the guard bands, the padding and (test_chain_does_not_depend_on_the_others) the bits of chain
0 under a different chain 1 are checked directly.

Largest |gpu - ref_longdouble| / e_ref seen on an MI355X over this file: beta 4.56, cand betaU
13.8, dlp 1.51, lp 1.0, state betaU 2.3 (the margins are that file's: 16, 40, 360).  This file
has cases of P = 1 and 3, where e_ref is the largest of one or three samples of the
restatement's own rounding, so its ratios run higher than that file's (P >= 63 there but for one
case); the kernels' arithmetic is the single-chain kernels'
(test_one_chain_equals_the_group_kernels: the same bits), so a ratio is a property of the
inputs, not of the chain axis.
"""
import ctypes

import numpy as np
import pytest
import torch

import _mcmc_group_ref as ref
import test_gpu_mcmc_group as single
from gladsgp_amd import _capi, kernels

pytestmark = pytest.mark.gpu

F64 = np.float64
GUARD, GUARD_BITS = single.GUARD, single.GUARD_BITS
PAD = 5                                    # guard doubles between chains (odd: misaligns them)
SHARED = ("lam", "step_betaU", "step_lamUz", "step_lamWs", "step_lamWOs")
OUTPUTS = ("beta", "s", "delta")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    seen = {}
    yield seen
    print("\nmcmc ensemble kernels, max |gpu - ref_longdouble| / e_ref: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(seen.items())))


def _pattern(n):
    a = np.empty(n, dtype=F64)
    a.view(np.int64)[:] = GUARD_BITS
    return a


class DeviceEnsemble:
    """The buffers of C chains in one of the layouts, the strides and chain 0's gp_mcmc_state."""

    def __init__(self, cases, dev, layout, g_out=None, _tensors=None):
        self.cases, self.dev, self.layout = cases, dev, layout
        st0 = cases[0]["st"]
        self.C, self.P, self.d = len(cases), st0["P"], st0["d"]
        self.ext = {nm: int(np.size(st0[nm])) for nm in ref.ARRAYS}
        self.stride = {}
        for nm in ref.ARRAYS:
            if layout == "shared" and nm in SHARED:
                self.stride[nm] = 0
            else:
                self.stride[nm] = self.ext[nm] + (PAD if layout == "padded" else 0)
        if _tensors is None:
            self.t = {}
            for nm in ref.ARRAYS:
                full = _pattern(2 * GUARD + (self.C - 1) * self.stride[nm] + self.ext[nm])
                for c in reversed(range(self.C)):      # stride 0: chain 0's values stay
                    o = GUARD + c * self.stride[nm]
                    full[o:o + self.ext[nm]] = np.asarray(cases[c]["st"][nm], F64).reshape(-1)
                self.t[nm] = torch.from_numpy(full).to(dev)
            if "ll_all" in cases[0]:
                ll = np.concatenate([_pattern(GUARD)] + [c["ll_all"] for c in cases]
                                    + [_pattern(GUARD)])
                self.t["ll_all"] = torch.from_numpy(ll).to(dev)
            self.new_outputs(g_out if g_out is not None else len(cases[0]["kinds"]))
        else:
            self.t = _tensors
        S = self.S = _capi.McmcState()
        T = self.T = _capi.McmcStrides()
        for nm in ref.ARRAYS:
            setattr(S, nm, self.ptr(nm))
            setattr(T, nm, self.stride[nm])
        S.P, S.d = self.P, self.d
        for i in range(4):
            S.dist[i], S.steptype[i] = st0["dist"][i], st0["steptype"][i]
            S.pa[i], S.pb[i], S.lo[i], S.hi[i] = (st0[k][i] for k in ("pa", "pb", "lo", "hi"))

    def ptr(self, nm):
        return self.t[nm].data_ptr() + 8 * GUARD

    def clone(self):
        return DeviceEnsemble(self.cases, self.dev, self.layout,
                              _tensors={k: v.clone() for k, v in self.t.items()})

    def new_outputs(self, g):
        self.g_out = g
        rows = self.C * (2 ** g - 1) * self.P
        for nm, n in (("beta", rows * self.d), ("s", rows), ("delta", rows)):
            self.t[nm] = torch.from_numpy(_pattern(n + 2 * GUARD)).to(self.dev)

    def host(self):
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def chain_image(self, h, c):
        """Chain c's part of the host image ``h`` as a single-chain image of
        test_gpu_mcmc_group.py (its buffers between synthetic guard bands)."""
        out = {}
        for nm in ref.ARRAYS:
            o = GUARD + c * self.stride[nm]
            out[nm] = np.concatenate([_pattern(GUARD), h[nm][o:o + self.ext[nm]],
                                      _pattern(GUARD)])
        rows = {"ll_all": (2 ** len(self.cases[0]["kinds"]) - 1) * self.P}
        for nm in OUTPUTS:
            rows[nm] = (2 ** self.g_out - 1) * self.P * (self.d if nm == "beta" else 1)
        for nm, n in rows.items():
            if nm in h:
                out[nm] = np.concatenate([_pattern(GUARD), h[nm][GUARD + c * n:GUARD + (c + 1) * n],
                                          _pattern(GUARD)])
        return out

    def outside_intact(self, h):
        """The guard bands and the padding between chains still hold the guard pattern."""
        for nm, a in h.items():
            keep = np.ones(a.size, bool)
            if nm in ref.ARRAYS:
                for c in range(self.C):
                    o = GUARD + c * self.stride[nm]
                    keep[o:o + self.ext[nm]] = False
            else:
                keep[GUARD:-GUARD] = False
            assert keep[:GUARD].all() and keep[-GUARD:].all()
            assert np.all(a.view(np.int64)[keep] == GUARD_BITS), f"outside the chains of {nm}"

    def _kinds(self, kinds):
        return (ctypes.c_int * len(kinds))(*kinds)

    def _st(self):
        return ctypes.addressof(self.S), ctypes.addressof(self.T), self.C

    def prep(self, kinds, first):
        k = self._kinds(kinds)
        _capi.call("gp_mcmc_ens_prep", *self._st(), ctypes.addressof(k), len(kinds), int(first),
                   self.ptr("beta"), self.ptr("s"), self.ptr("delta"), kernels._stream(self.dev))

    def decide(self, kinds, last):
        k = self._kinds(kinds)
        _capi.call("gp_mcmc_ens_decide", *self._st(), ctypes.addressof(k), len(kinds), int(last),
                   self.ptr("ll_all"), kernels._stream(self.dev))

    def step(self, kinds, last, kinds_next, first):
        k, kn = self._kinds(kinds), self._kinds(kinds_next)
        _capi.call("gp_mcmc_ens_step", *self._st(), ctypes.addressof(k), len(kinds), int(last),
                   self.ptr("ll_all"), ctypes.addressof(self.S), ctypes.addressof(kn),
                   len(kinds_next), int(first), self.ptr("beta"), self.ptr("s"),
                   self.ptr("delta"), kernels._stream(self.dev))


def _share(cases):
    """Give every chain chain 0's lam and steps (the `shared` layout holds one copy)."""
    for c in cases[1:]:
        for nm in SHARED:
            c["st"][nm] = cases[0]["st"][nm].copy()
    return cases


def _run_and_check(dev, cases, layout, ratios):
    """gp_mcmc_ens_prep then gp_mcmc_ens_decide on all chains; every chain against its own
    restatement.  Returns the references and the three host images."""
    if layout == "shared":
        _share(cases)
    refs = [single._reference(c) for c in cases]
    E = DeviceEnsemble(cases, dev, layout)
    h0 = E.host()
    E.prep(cases[0]["kinds"], cases[0]["first"])
    hA = E.host()
    E.decide(cases[0]["kinds"], cases[0]["last"])
    hB = E.host()
    for h in (hA, hB):
        E.outside_intact(h)
    for c, (case, R) in enumerate(zip(cases, refs)):
        i0, iA, iB = (E.chain_image(h, c) for h in (h0, hA, hB))
        single._check_prep(case, R, i0, iA, ratios)
        single._check_decide(case, R, iA, iB, ratios)
    return refs, (h0, hA, hB), E


# ------------------------------------------------------------------------------------- cases
LAYOUTS = ("packed", "padded", "shared")


def shape_cases(C, P, d, g):
    """C chains with their own states, uniforms and ll_all under one drawn group of g distinct
    codes; first / last take all four combinations over g = 1..4 for every (C, P, d)."""
    rng = np.random.default_rng([P, d, g])
    kinds = rng.permutation(np.arange(1, d + 4))[:g]
    first, last = (g + P + C) % 2, (g // 2 + d) % 2
    return [single._case(ref.default_state(P, d, seed=10 * c + g), kinds, first, last, seed=c)
            for c in range(C)]


@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("P", [1, 3, 65])
@pytest.mark.parametrize("C", [1, 2, 5])
def test_shapes(dev, ratios, C, P, d, g):
    """One and several workgroups, one GP, a partial wave and two waves; the layout rotates so
    that every (C, P, d) meets all three over g = 1..4 and its repeats."""
    layout = LAYOUTS[(C + P + d + g) % 3]
    _run_and_check(dev, shape_cases(C, P, d, g), layout, ratios)


WP, WD = 65, 5
WOS_GROUPS = {"wos_at_0": [WD + 3, 4, WD + 2, 2], "wos_at_1": [4, WD + 3, WD + 2, 2],
              "wos_at_2": [4, WD + 2, WD + 3, 2], "wos_at_3": [4, WD + 2, 2, WD + 3]}


def wos_cases(name):
    """lamWOs at position q of the group; chains 0 and 2 are steered to accept it, chain 1 to
    reject it (test_gpu_mcmc_group's shift of the lamWOs state sets)."""
    kinds = WOS_GROUPS[name]
    return [single._case(ref.default_state(WP, WD, seed=40 + c + len(name)), kinds, 1, 1, seed=c,
                         shift=single._wos_shift(kinds, WD, WP, 1.0 if c != 1 else -1.0))
            for c in range(3)]


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("name", list(WOS_GROUPS))
def test_lamwos_decided_both_ways_in_one_call(dev, ratios, name, layout):
    cases = wos_cases(name)
    refs, _, _ = _run_and_check(dev, cases, layout, ratios)
    q = WOS_GROUPS[name].index(WD + 3)
    took = [bool(R[F64]["dec"]["accept"][q, 0]) for R in refs]
    assert took == [True, False, True], "the shift did not steer lamWOs: pick another seed"
    for R, t in zip(refs, took):                       # later updates read the set lamWOs selects
        for i in range(q + 1, 4):
            assert np.all(((R[F64]["dec"]["slots"][i] - (2 ** i - 1)) >> q) & 1 == t)


@pytest.mark.parametrize("P,d,g", [(3, 1, 2), (65, 5, 4)])
def test_one_chain_equals_the_group_kernels(dev, P, d, g):
    """nchains = 1, with strides that would be errors for two chains: every buffer holds the bits
    gp_mcmc_group_prep / _decide / _step leave."""
    case = shape_cases(1, P, d, g)[0]
    case["first"] = case["last"] = 1
    nxt = [int(c) for c in np.random.default_rng(g).permutation(np.arange(1, d + 4))[:g]]
    for merged in (False, True):
        A = single.DeviceState(case["st"], dev, case["ll_all"], g)
        E = DeviceEnsemble([case], dev, "packed")
        for nm in ref.ARRAYS:                          # never read: one chain
            setattr(E.T, nm, -3)
        for D in (A, E):
            D.prep(case["kinds"], 1)
            if merged:
                D.step(case["kinds"], 1, nxt, 1)
            else:
                D.decide(case["kinds"], 1)
        a, e = A.host(), E.host()
        assert sorted(a) == sorted(e)
        for nm in a:
            single._same_bits(f"{nm} (merged {merged})", e[nm], a[nm])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C,P,last", [(2, 65, 0), (5, 3, 1)])
def test_merged_step_equals_decide_then_prep(dev, C, P, last, layout):
    """gp_mcmc_ens_step against gp_mcmc_ens_decide + gp_mcmc_ens_prep on a copy of the same
    buffers, every buffer bit for bit; the two groups have different sizes, so ll_all and the
    outputs use different chain offsets."""
    d = 5
    kinds, nxt = [2, d + 3, d + 1], [d + 2, 1, 3, 4]
    cases = [single._case(ref.default_state(P, d, seed=31 + c), kinds, 1, last, seed=c,
                          shift=single._wos_shift(kinds, d, P, 1.0 if c % 2 else -1.0))
             for c in range(C)]
    if layout == "shared":
        _share(cases)
    D = DeviceEnsemble(cases, dev, layout)
    D.prep(kinds, 1)
    D.new_outputs(len(nxt))
    E = D.clone()
    E.g_out = D.g_out
    before = D.host()
    D.decide(kinds, last)
    D.prep(nxt, last)
    E.step(kinds, last, nxt, last)
    two, one = D.host(), E.host()
    E.outside_intact(one)
    for nm in two:
        single._same_bits(nm, one[nm], two[nm])
    for nm in ("acc", "scratch", "beta", "s", "delta", "ll"):
        assert np.any(single._bits(two[nm]) != single._bits(before[nm])), nm
    # every chain's rows of the next group's batch were written, and nothing beyond them
    rows = (2 ** len(nxt) - 1) * P
    s = one["s"][GUARD:-GUARD]
    assert s.size == C * rows and not np.any(s.view(np.int64) == GUARD_BITS)


@pytest.mark.parametrize("layout", ["packed", "padded"])
def test_chain_does_not_depend_on_the_others(dev, layout):
    """The same chain 0 beside two different chains 1: chain 0's buffers and batch rows keep
    their bits (and chain 1's differ, so the second run did change something)."""
    P, d, g = 65, 5, 3
    a = shape_cases(2, P, d, g)
    b = shape_cases(2, P, d, g)
    b[1] = single._case(ref.default_state(P, d, seed=77), a[0]["kinds"], a[0]["first"],
                        a[0]["last"], seed=9)
    images = []
    for cases in (a, b):
        E = DeviceEnsemble(cases, dev, layout)
        E.prep(cases[0]["kinds"], 1)
        E.decide(cases[0]["kinds"], 1)
        h = E.host()
        images.append([E.chain_image(h, c) for c in range(2)])
    for nm in images[0][0]:
        single._same_bits(f"chain 0: {nm}", images[1][0][nm], images[0][0][nm])
    assert any(np.any(single._bits(images[1][1][nm]) != single._bits(images[0][1][nm]))
               for nm in ("betaU", "ll", "s", "lp"))
