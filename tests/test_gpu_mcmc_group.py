"""GPU: the three Metropolis group kernels of csrc/mcmc.hip (gp_mcmc_group_prep, _decide, _step)
called directly, against the numpy restatement tests/_mcmc_group_ref.py (float64 and, as the
high-precision reference, longdouble; itself checked against the oracle chain in
test_mcmc_group_cpu.py).  ``ll_all`` is drawn by the test (current ll + N(0, 2)): gp_loglik is
never called, so a case is a few single-workgroup launches.

What is compared, and how:
  * exact, bit for bit with the float64 restatement: the Uniform-step candidates, the in-range
    flags, s = 1/lamUz and delta = 1/lamWs + 1/(lamWOs lam) wherever their inputs are Uniform-step
    candidates or state, the selection of beta rows, ll, the counters, and which elements change
    (the kernels are built without FMA contraction);
  * through exp / log / log1p (BetaRho candidates, dlp, lp, anything downstream of an accepted
    BetaRho candidate): |gpu - ref_longdouble| <= margin * e_ref + 4 ulp(ref), with
    e_ref = max |ref_float64 - ref_longdouble| of that quantity in that case: the rounding a
    correct fp64 implementation shows at this conditioning.  An indexing or parameter mix-up
    moves these values by 1e-3 or more;
  * every buffer sits between guard bands of a NaN with a payload, compared bit for bit, and
    every element the header does not name as written must keep its bits.

Conditions on the inputs are asserted on the restatement alone (``_input_conditions``), never on
the kernels' output: every decision margin >= 1e-8, every bound and rho-range margin >= 1e-9,
the two precisions take the same decisions.  Then every flag, decision and counter must match
exactly.  A failure of such a condition says "pick another seed".

Largest |gpu - ref_longdouble| / e_ref seen on an MI355X over all cases of this file, per
quantity (MEASURED below): candidates, state, beta, s and delta 1.0 .. 1.96, dlp 9.66, lp 88.1.
The margin starts at 16 and is kept at no less than 4 times the measured ratio, so dlp has 40 and
lp 360.  lp is one number per case, so its e_ref is a single sample of the rounding of a sum of
(d + 4) P terms: in shapes[65-32-3] the float64 restatement happens to land 0.023 ulp from the
longdouble one, and a kernel that is 2 ulp away shows a ratio of 88 (the restatement's own e_ref
over the cases of this file spans 0.023 .. 84 ulp).  At 360 the lp bound is still below 4e-12
absolute in every case.
"""
import ctypes

import numpy as np
import pytest
import torch

import _mcmc_group_ref as ref
from gladsgp_amd import _capi, kernels

pytestmark = pytest.mark.gpu

MARGIN = 16.0                      # of every quantity but:
MARGINS = {"dlp": 40.0, "lp": 360.0}
MEASURED = {"beta": 1.33, "cand betaU": 1.96, "cand lamUz": 1.0, "cand lamWs": 1.0,
            "cand lamWOs": 1.24, "s": 1.0, "delta": 1.2, "dlp": 9.66, "lp": 88.1,
            "state betaU": 1.69, "state lamUz": 1.0, "state lamWs": 1.0, "state lamWOs": 1.24}
assert all(MARGINS.get(k, MARGIN) >= 4.0 * v for k, v in MEASURED.items())
GUARD = 32                         # doubles before and after every buffer
GUARD_BITS = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.int64)[0]
F64, LD = np.float64, np.longdouble


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    """Largest |gpu - ref_longdouble| / e_ref per quantity over the module, printed at the end."""
    seen = {}
    yield seen
    print("\nmcmc group kernels, max |gpu - ref_longdouble| / e_ref: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(seen.items())))


# ----------------------------------------------------------------------------------- helpers
def _bits(a):
    return np.ascontiguousarray(a, dtype=F64).reshape(-1).view(np.int64)


def _same_bits(name, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, name
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{name}: {bad.size} of {g.size} elements differ, first at {bad[0]}: "
                           f"{np.asarray(got).reshape(-1)[bad[0]]!r} != "
                           f"{np.asarray(want).reshape(-1)[bad[0]]!r}")


def _close(name, got, r64, rld, ratios):
    """|got - rld| <= margin e_ref + 4 ulp(r64) on the finite elements (the others: the bits of
    r64), e_ref = max |r64 - rld| over them."""
    got, r64 = np.asarray(got, F64).reshape(-1), np.asarray(r64, F64).reshape(-1)
    rld = np.asarray(rld, LD).reshape(-1)
    assert got.shape == r64.shape == rld.shape, name
    fin = np.isfinite(r64)
    _same_bits(name + " (non-finite)", got[~fin], r64[~fin])
    if not fin.any():
        return
    e_ref = float(np.max(np.abs(r64[fin] - rld[fin])))
    err = np.abs(got[fin].astype(LD) - rld[fin])
    bound = MARGINS.get(name, MARGIN) * e_ref + 4.0 * np.spacing(np.abs(r64[fin]))
    if e_ref > 0:
        ratios[name] = max(ratios.get(name, 0.0), float(np.max(err) / e_ref))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{name}: {bad.size} of {err.size} outside the bound, first at "
                           f"{bad[0]}: gpu {got[fin][bad[0]]!r} ref {r64[fin][bad[0]]!r} "
                           f"err {float(err[bad[0]]):.3e} e_ref {e_ref:.3e}")


def _guarded(a, dev):
    full = np.empty(np.size(a) + 2 * GUARD, dtype=F64)
    full.view(np.int64)[:] = GUARD_BITS
    full[GUARD:GUARD + np.size(a)] = np.asarray(a, dtype=F64).reshape(-1)
    return torch.from_numpy(full).to(dev)


class DeviceState:
    """gp_mcmc_state over guarded device buffers, with ll_all and the beta / s / delta outputs
    of a group of ``g`` (all guard pattern before the first launch)."""

    def __init__(self, st, dev, ll_all=None, g_out=None, _tensors=None):
        self.st, self.dev = st, dev
        P, d = st["P"], st["d"]
        if _tensors is None:
            self.t = {nm: _guarded(st[nm], dev) for nm in ref.ARRAYS}
            if ll_all is not None:
                self.t["ll_all"] = _guarded(ll_all, dev)
            self.new_outputs(g_out)
        else:
            self.t = _tensors
        S = self.S = _capi.McmcState()
        for nm in ref.ARRAYS:
            setattr(S, nm, self.ptr(nm))
        S.P, S.d = P, d
        for i in range(4):
            S.dist[i], S.steptype[i] = st["dist"][i], st["steptype"][i]
            S.pa[i], S.pb[i], S.lo[i], S.hi[i] = (st[k][i] for k in ("pa", "pb", "lo", "hi"))

    def ptr(self, nm):
        return self.t[nm].data_ptr() + 8 * GUARD

    def clone(self):
        return DeviceState(self.st, self.dev, _tensors={k: v.clone() for k, v in self.t.items()})

    def new_outputs(self, g):
        """beta / s / delta of a group of g, all guard pattern."""
        P, d, nset = self.st["P"], self.st["d"], 2 ** g - 1
        for nm, n in (("beta", nset * P * d), ("s", nset * P), ("delta", nset * P)):
            self.t[nm] = _guarded(np.zeros(n), self.dev)
            self.t[nm].view(torch.int64).fill_(int(GUARD_BITS))

    def host(self):
        """Every buffer, guards included, as numpy (synchronises)."""
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def _kinds(self, kinds):
        return (ctypes.c_int * len(kinds))(*kinds)

    def prep(self, kinds, first):
        k = self._kinds(kinds)
        _capi.call("gp_mcmc_group_prep", ctypes.addressof(self.S), ctypes.addressof(k),
                   len(kinds), int(first), self.ptr("beta"), self.ptr("s"), self.ptr("delta"),
                   kernels._stream(self.dev))

    def decide(self, kinds, last):
        k = self._kinds(kinds)
        _capi.call("gp_mcmc_group_decide", ctypes.addressof(self.S), ctypes.addressof(k),
                   len(kinds), int(last), self.ptr("ll_all"), kernels._stream(self.dev))

    def step(self, kinds, last, kinds_next, first):
        k, kn = self._kinds(kinds), self._kinds(kinds_next)
        _capi.call("gp_mcmc_group_step", ctypes.addressof(self.S), ctypes.addressof(k),
                   len(kinds), int(last), self.ptr("ll_all"), ctypes.addressof(self.S),
                   ctypes.addressof(kn), len(kinds_next), int(first), self.ptr("beta"),
                   self.ptr("s"), self.ptr("delta"), kernels._stream(self.dev))


def _core(h, nm, shape=-1):
    return h[nm][GUARD:-GUARD].reshape(shape)


def _guards_intact(h):
    for nm, a in h.items():
        b = a.view(np.int64)
        assert np.all(b[:GUARD] == GUARD_BITS), f"guard before {nm} overwritten"
        assert np.all(b[-GUARD:] == GUARD_BITS), f"guard after {nm} overwritten"


# ------------------------------------------------------------------------- reference + inputs
def _case(st, kinds, first, last, seed=0, shift=None):
    kinds = [int(c) for c in kinds]
    return dict(st=st, kinds=kinds, first=int(first), last=int(last),
                ll_all=ref.draw_ll_all(st, len(kinds), seed, shift))


def _wos_shift(kinds, d, P, sign):
    """ll_all shift per state set that steers the shared lamWOs decision: +-6 per GP on the sets
    of the lamWOs update.  The N(0, 2) draws sum to O(2 sqrt(P)), and every earlier accepted
    update of the group raised its GP's ll by about 1.5 (accepted draws are the favourable
    ones), at most 3 updates: 6 per GP outweighs both for P >= 1.  The sets of later updates
    that follow an accepted lamWOs carry the same shift, so they stay "current ll + N(0, 2)"."""
    g = len(kinds)
    shift = np.zeros(2 ** g - 1)
    if d + 3 in kinds:
        i = list(kinds).index(d + 3)
        shift[2 ** i - 1:2 ** (i + 1) - 1] = sign * 6.0
        for later in range(i + 1, g):
            for pat in range(2 ** later):
                if (pat >> i) & 1:
                    shift[2 ** later - 1 + pat] = sign * 6.0
    return shift


def _reference(case):
    """The restatement in both precisions: prep outputs, the state after prep (mid) and after
    decide (end), decide's record; the input conditions asserted."""
    out = {}
    for T in (F64, LD):
        st = ref.cast(case["st"], T)
        p = ref.prep(st, case["kinds"], case["first"], T)
        mid = ref.cast(st, T)
        dec = ref.decide(st, case["kinds"], case["last"], case["ll_all"], T)
        out[T] = dict(prep=p, mid=mid, dec=dec, end=st)
    _input_conditions(out)
    return out


def _input_conditions(R):
    for T in (F64, LD):
        m = R[T]["prep"]["margins"]
        dm = [R[T]["dec"]["margin"]] + ([m["row0"]["decision"]] if "row0" in m else [])
        assert min(float(np.min(x)) for x in dm) >= 1e-8, "decision margin: pick another seed"
        bm = m["bound"] + m["rho"] + ([m["row0"]["bound"], m["row0"]["rho"]] if "row0" in m
                                      else [])
        assert min(float(np.min(x)) for x in bm) >= 1e-9, "range margin: pick another seed"
    a, b = R[F64], R[LD]
    assert np.array_equal(a["prep"]["ok"], b["prep"]["ok"])
    assert np.array_equal(a["dec"]["accept"], b["dec"]["accept"])
    assert np.array_equal(a["dec"]["slots"], b["dec"]["slots"])
    assert np.array_equal(a["end"]["acc"], b["end"]["acc"])


# ----------------------------------------------------------------------------- the comparison
def _check_prep(case, R, h0, hA, ratios):
    st0, kinds, first = case["st"], case["kinds"], case["first"]
    P, d, g = st0["P"], st0["d"], len(kinds)
    r64, rld = R[F64], R[LD]
    exact = [t == ref.STEP_UNIFORM for t in st0["steptype"]]
    _guards_intact(hA)
    for nm in ("lam", "u", "step_betaU", "step_lamUz", "step_lamWs", "step_lamWOs", "lamUz",
               "lamWs", "lamWOs", "ll", "lp", "ll_all"):
        _same_bits(f"prep must not write {nm}", hA[nm], h0[nm])
    # betaU: only row 0, only when first, only its accepted elements
    b, b0 = _core(hA, "betaU", (d + 1, P)), _core(h0, "betaU", (d + 1, P))
    _same_bits("prep must not write betaU rows 1..d", b[1:], b0[1:])
    if first:
        row0 = r64["prep"]["margins"]["row0"]
        _same_bits("betaU row 0, rejected", b[0][~row0["accept"]], b0[0][~row0["accept"]])
        if exact[0]:
            _same_bits("betaU row 0", b[0], r64["mid"]["betaU"][0])
        else:
            _close("cand betaU", b[0], r64["mid"]["betaU"][0], rld["mid"]["betaU"][0], ratios)
    else:
        _same_bits("betaU row 0 (first == 0)", b[0], b0[0])
        _same_bits("acc (first == 0)", hA["acc"], h0["acc"])
    _same_bits("acc after prep", _core(hA, "acc"), r64["mid"]["acc"])
    # scratch: element 0 only for lamWOs, rows >= g untouched
    scr = _core(hA, "scratch", (3, ref.MAX_GROUP, P))
    scr0 = _core(h0, "scratch", (3, ref.MAX_GROUP, P))
    s64, sld = r64["mid"]["scratch"], rld["mid"]["scratch"]
    written = np.zeros((ref.MAX_GROUP, P), bool)
    for i, code in enumerate(kinds):
        written[i, :1 if code == d + 3 else P] = True
    for k, nm in enumerate(("cand", "ok", "dlp")):
        _same_bits(f"scratch {nm}, unwritten part", scr[k][~written], scr0[k][~written])
    _same_bits("ok flags", scr[1][written], s64[1][written])
    for i, code in enumerate(kinds):
        p = 0 if code <= d else code - d
        w = written[i]
        if exact[p]:
            _same_bits(f"cand of update {i} (code {code})", scr[0, i][w], s64[0, i][w])
        else:
            _close("cand " + ref.PARAMS[p], scr[0, i][w], s64[0, i][w], sld[0, i][w], ratios)
        n = 1 if code == d + 3 else P
        rej = s64[1, i, :n] == 0
        _same_bits(f"cand of update {i}, out of range: the current value", scr[0, i, :n][rej],
                   _update_values(st0, code)[rej])
    _close("dlp", scr[2][written], s64[2][written], sld[2][written], ratios)
    # the Gram inputs of the 2^g - 1 state sets
    nset = 2 ** g - 1
    p64, pld = r64["prep"], rld["prep"]
    beta = _core(hA, "beta", (nset * P, d))
    kept = _bits(p64["beta"]) == _bits(np.tile(st0["betaU"][1:].T, (nset, 1)))
    _same_bits("beta rows taken from the state", beta.reshape(-1)[kept],
               p64["beta"].reshape(-1)[kept])
    for nm, codes, got in (("beta", range(1, d + 1), beta), ("s", (d + 1,), _core(hA, "s")),
                           ("delta", (d + 2, d + 3), _core(hA, "delta"))):
        if all(exact[0 if c <= d else c - d] for c in kinds if c in codes):
            _same_bits(nm, got, p64[nm])
        else:
            _close(nm, got, p64[nm], pld[nm], ratios)


def _update_values(st, code):
    d = st["d"]
    if code <= d:
        return st["betaU"][code]
    return st[("lamUz", "lamWs", "lamWOs")[code - d - 1]]


def _check_decide(case, R, hA, hB, ratios):
    st0, last = case["st"], case["last"]
    r64, rld = R[F64], R[LD]
    exact = [t == ref.STEP_UNIFORM for t in st0["steptype"]]
    _guards_intact(hB)
    for nm in ("lam", "u", "step_betaU", "step_lamUz", "step_lamWs", "step_lamWOs", "scratch",
               "beta", "s", "delta", "ll_all"):
        _same_bits(f"decide must not write {nm}", hB[nm], hA[nm])
    for p, nm in enumerate(ref.PARAMS):
        got, before = _core(hB, nm), _core(hA, nm)
        e64, eld = r64["end"][nm].reshape(-1), rld["end"][nm].reshape(-1)
        unchanged = _bits(e64) == _bits(r64["mid"][nm])
        _same_bits(f"{nm}, elements not accepted", got[unchanged], before[unchanged])
        if exact[p]:
            _same_bits(nm, got, e64)
        else:
            _close("state " + nm, got, e64, eld, ratios)
    _same_bits("ll", _core(hB, "ll"), r64["end"]["ll"])
    _same_bits("acc", _core(hB, "acc"), r64["end"]["acc"])
    if last:
        _close("lp", _core(hB, "lp"), r64["dec"]["lp"], rld["dec"]["lp"], ratios)
    else:
        _same_bits("lp (last == 0)", hB["lp"], hA["lp"])


def _run(dev, case):
    """prep then decide on fresh guarded buffers: the host images before, between and after."""
    D = DeviceState(case["st"], dev, case["ll_all"], len(case["kinds"]))
    h0 = D.host()
    D.prep(case["kinds"], case["first"])
    hA = D.host()
    D.decide(case["kinds"], case["last"])
    return h0, hA, D.host()


def _run_and_check(dev, case, ratios):
    R = _reference(case)
    h0, hA, hB = _run(dev, case)
    _check_prep(case, R, h0, hA, ratios)
    _check_decide(case, R, hA, hB, ratios)
    return R, (h0, hA, hB)


# ------------------------------------------------------------------------------------- cases
def shape_case(P, d, g):
    """g distinct update codes in a drawn order (not the sampler's), first / last covering all
    four combinations over g = 1..4 for every (P, d)."""
    rng = np.random.default_rng([P, d, g])
    kinds = rng.permutation(np.arange(1, d + 4))[:g]
    return _case(ref.default_state(P, d, seed=g), kinds, (g + P) % 2, (g // 2 + d) % 2)


@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("d", [1, 5, 32])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 200, 1024])
def test_shapes(dev, ratios, P, d, g):
    """One to sixteen waves, P on and beside the wave size, the largest P and d."""
    _run_and_check(dev, shape_case(P, d, g), ratios)


CP, CD = 200, 5                                        # compositions: 4 waves, d + 3 = 8 codes
COMPOSITIONS = {
    "wos_at_0": [CD + 3, 4, CD + 2, 2], "wos_at_1": [4, CD + 3, CD + 2, 2],
    "wos_at_2": [4, CD + 2, CD + 3, 2], "wos_at_3": [4, CD + 2, 2, CD + 3],
    "no_wos": [1, CD + 1, 3, CD + 2], "betaU_descending": [5, 4, 2, 1],
    "wos_alone": [CD + 3], "wos_first_of_2": [CD + 3, CD + 1],
}


def composition_case(name, wos):
    kinds = COMPOSITIONS[name]
    sign = {"accept": 1.0, "reject": -1.0}[wos]
    return _case(ref.default_state(CP, CD, seed=len(name)), kinds, 0, 1,
                 shift=_wos_shift(kinds, CD, CP, sign))


@pytest.mark.parametrize("wos", ["accept", "reject"])
@pytest.mark.parametrize("name", list(COMPOSITIONS))
def test_compositions(dev, ratios, name, wos):
    """Groups the sampler never forms.  The shared lamWOs decision is steered both ways by a
    shift of its state sets' ll_all; every later update must then read the other state set."""
    case = composition_case(name, wos)
    R = _reference(case)
    composition_conditions(case, R, wos)
    h0, hA, hB = _run(dev, case)
    _check_prep(case, R, h0, hA, ratios)
    _check_decide(case, R, hA, hB, ratios)


def composition_conditions(case, R, wos):
    kinds, g = case["kinds"], len(case["kinds"])
    dec = R[F64]["dec"]
    pats = set((dec["accept"].astype(int) << np.arange(g)[:, None]).sum(0).tolist())
    if CD + 3 in kinds:
        q = kinds.index(CD + 3)
        took = bool(dec["accept"][q, 0])
        assert took == (wos == "accept"), "the shift did not steer lamWOs: pick another seed"
        assert np.all(dec["accept"][q] == took)
        want = {p for p in range(2 ** g) if ((p >> q) & 1) == took}
        for i in range(q + 1, g):                      # later updates: the set lamWOs selects
            assert np.all(((dec["slots"][i] - (2 ** i - 1)) >> q) & 1 == took)
    else:
        want = set(range(2 ** g))
    assert pats == want, f"outcome patterns {sorted(want - pats)} never occur: pick another seed"


LP_CASES = [(5, 256), (5, 257), (32, 1024), (1, 1)]


def lp_case(d, P):
    return _case(ref.default_state(P, d, seed=9), [d + 2, 1], 1, 1)


@pytest.mark.parametrize("d,P", LP_CASES, ids=[f"nt{(d + 3) * P}" for d, P in LP_CASES])
def test_log_posterior_branches(dev, ratios, d, P):
    """(d + 3) P = 2048 is the last size whose prior terms are computed one per thread, 2056 the
    first on the per-GP serial path; the largest and the smallest problem."""
    _run_and_check(dev, lp_case(d, P), ratios)


FAMILIES = {ref.GAMMA: "Gamma", ref.BETA: "Beta", ref.NORMAL: "Normal", ref.UNIFORM: "Uniform"}
STEPS = {ref.STEP_UNIFORM: "uni", ref.STEP_BETARHO: "rho"}


def latin(k):
    """Row k of a Latin square: parameter p gets family (p + k) % 4 and a step type that takes
    both values per parameter and per family over k = 0..3."""
    dist = [(p + k) % 4 for p in range(4)]
    step = [(f // 2 + p) % 2 for p, f in enumerate(dist)]
    return dist, step


def _latin_id(k):
    dist, step = latin(k)
    return "-".join(f"{nm}:{FAMILIES[f]}/{STEPS[s]}" for nm, f, s in zip(ref.PARAMS, dist, step))


def prior_case(k):
    dist, step = latin(k)
    d = CD
    kinds = [2, d + 1, d + 2, d + 3]
    st = ref.unit_state(CP, d, seed=k, dist=dist, steptype=step)
    st["lamWOs"][:] = 2.0                              # the one lamWOs proposal: a small move
    st["u"][2 * CP * (d + 3)] = 0.55                   # inside the bounds, so its prior counts
    case = _case(st, kinds, 1, 1, shift=_wos_shift(kinds, d, CP, 1.0 if k % 2 == 0 else -1.0))
    case["wos_accepted"] = k % 2 == 0
    return case


@pytest.mark.parametrize("k", range(4), ids=[_latin_id(k) for k in range(4)])
def test_priors_steps_and_bounds(dev, ratios, k):
    """Every family on every parameter and both step types on each, with bounds tight enough
    that each per-GP update has accepted and bound-rejected proposals (5 % .. 95 % rejected) and
    every BetaRho update leaves (0, 1] on both sides."""
    case = prior_case(k)
    R = _reference(case)
    prior_conditions(case, R)
    h0, hA, hB = _run(dev, case)
    _check_prep(case, R, h0, hA, ratios)
    _check_decide(case, R, hA, hB, ratios)


def prior_conditions(case, R):
    st, kinds, d = case["st"], case["kinds"], case["st"]["d"]
    p, dec = R[F64]["prep"], R[F64]["dec"]
    m = p["margins"]
    # (parameter, in-range flags, decisions, side of rho's range) of each per-GP update
    rows = [(0, m["row0"]["ok"], m["row0"]["accept"], m["row0"]["side"])]
    rows += [(0 if c <= d else c - d, p["ok"][i] != 0, dec["accept"][i], m["side"][i])
             for i, c in enumerate(kinds) if c != d + 3]
    assert sorted(r[0] for r in rows) == [0, 0, 1, 2]
    for par, ok, acc, side in rows:
        share = 1.0 - float(np.mean(ok))
        assert 0.05 <= share <= 0.95, f"rejected share {share:.3f}: tune steps and bounds"
        assert acc.any() and not ok.all()       # accepted and bound-rejected proposals
        if st["steptype"][par] == ref.STEP_BETARHO:
            assert (side < 0).any() and (side > 0).any(), "rho leaves (0, 1] on one side only"
    q = kinds.index(d + 3)                             # lamWOs: in range, steered by k
    assert p["ok"][q, 0] != 0 and (p["dlp"][q, 0] != 0) == (st["dist"][3] != ref.UNIFORM)
    assert dec["accept"][q, 0] == case["wos_accepted"]
    # the prior differences are O(1): neither negligible nor dominant
    moved = np.abs(p["dlp"][p["ok"] != 0])
    moved = moved[moved > 0]
    assert moved.size == 0 or 0.05 < np.median(moved) < 20.0


WOS_BOUNDS = {                     # lamWOs value, step, proposal uniform, step type, in range
    "uniform_in": (2.0, 2.0, 0.6, ref.STEP_UNIFORM, True),
    "uniform_above_hi": (3.5, 2.0, 0.9, ref.STEP_UNIFORM, False),
    "uniform_below_lo": (0.8, 2.0, 0.1, ref.STEP_UNIFORM, False),
    "rho_in": (2.0, 0.8, 0.55, ref.STEP_BETARHO, True),
    "rho_le_0": (3.5, 1.0, 0.02, ref.STEP_BETARHO, False),
    "rho_gt_1": (0.8, 1.0, 0.95, ref.STEP_BETARHO, False),
    "rho_in_range_below_lo": (0.8, 0.8, 0.7, ref.STEP_BETARHO, False),
}


def wos_bounds_case(name):
    x, step, up, stype, _ = WOS_BOUNDS[name]
    d, P = 5, 65
    st = ref.unit_state(P, d, seed=3, dist=[ref.BETA, ref.GAMMA, ref.NORMAL, ref.GAMMA],
                        steptype=[ref.STEP_BETARHO, ref.STEP_UNIFORM, ref.STEP_UNIFORM, stype])
    st["lamWOs"][:], st["step_lamWOs"][:] = x, step
    st["u"][2 * P * (d + 3)] = up
    kinds = [d + 1, d + 3, 3]
    return _case(st, kinds, 0, 1, shift=_wos_shift(kinds, d, P, 1.0))


@pytest.mark.parametrize("name", list(WOS_BOUNDS))
def test_lamwos_bounds(dev, ratios, name):
    """The single lamWOs proposal inside its bounds (then accepted: ll_all favours it) and
    rejected by each bound and by each end of rho's range, whatever ll_all says."""
    case = wos_bounds_case(name)
    R = _reference(case)
    inside = WOS_BOUNDS[name][4]
    assert bool(R[F64]["prep"]["ok"][1, 0]) == inside
    assert bool(R[F64]["dec"]["accept"][1, 0]) == inside
    side = R[F64]["prep"]["margins"]["side"][1][0]
    assert side == {"rho_le_0": -1, "rho_gt_1": 1}.get(name, 0)
    h0, hA, hB = _run(dev, case)
    _check_prep(case, R, h0, hA, ratios)
    _check_decide(case, R, hA, hB, ratios)
    if not inside:
        _same_bits("lamWOs", hB["lamWOs"], h0["lamWOs"])
        _same_bits("lamWOs counter", _core(hB, "acc", (5 + 4, 65))[5 + 3],
                   _core(h0, "acc", (5 + 4, 65))[5 + 3])


NONFINITE = ["per_gp", "wos_nan", "wos_minus_inf", "wos_current_minus_inf"]


def nonfinite_case(name):
    """Entries of ll_all that must reject whatever else holds.  per_gp: GP 7 has ll = -inf and
    only -inf proposals (NaN differences); GPs 20..24 get -inf for update 0, 30..34 NaN for
    update 1, 40..44 NaN for update 2, in every state set of that update.  wos_*: one bad entry
    among the lamWOs update's state sets, which ll_all otherwise favours by 6 per GP."""
    d, P = 5, 200
    st = ref.default_state(P, d, seed=21)
    if name == "per_gp":
        kinds, hit = [1, d + 1, 3], {}
        st["ll"][7] = -np.inf
        case = _case(st, kinds, 1, 1)
        ll = case["ll_all"].reshape(7, P)
        ll[:, 7] = -np.inf
        for i, (gps, v) in enumerate(((range(20, 25), -np.inf), (range(30, 35), np.nan),
                                      (range(40, 45), np.nan))):
            ll[2 ** i - 1:2 ** (i + 1) - 1, list(gps)] = v
            hit[i] = [7] + list(gps)
        case["hit"] = hit
        return case
    kinds = [2, d + 3, d + 1]
    if name == "wos_current_minus_inf":
        st["ll"][7] = -np.inf
    case = _case(st, kinds, 0, 1, shift=_wos_shift(kinds, d, P, 1.0))
    ll = case["ll_all"].reshape(7, P)
    if name == "wos_current_minus_inf":
        ll[:, 7] = -np.inf
    else:
        ll[1:3, 5] = np.nan if name == "wos_nan" else -np.inf
    case["hit"] = {1: list(range(P))}
    return case


@pytest.mark.parametrize("name", NONFINITE)
def test_nonfinite_likelihoods_reject(dev, ratios, name):
    case = nonfinite_case(name)
    R = _reference(case)
    d, P, kinds = case["st"]["d"], case["st"]["P"], case["kinds"]
    for i, gps in case["hit"].items():
        assert not R[F64]["dec"]["accept"][i, gps].any()
        assert np.any(R[F64]["prep"]["ok"][i, :1 if kinds[i] == d + 3 else P] != 0)
    h0, hA, hB = _run(dev, case)
    _check_prep(case, R, h0, hA, ratios)
    _check_decide(case, R, hA, hB, ratios)
    acc0, acc1 = _core(hA, "acc", (d + 4, P)), _core(hB, "acc", (d + 4, P))
    for i, gps in case["hit"].items():
        code = kinds[i]
        if code == d + 3:
            _same_bits("lamWOs", hB["lamWOs"], h0["lamWOs"])
            _same_bits("lamWOs counter", acc1[code], acc0[code])
            continue
        nm = "betaU" if code <= d else ("lamUz", "lamWs")[code - d - 1]
        shape = (d + 1, P) if code <= d else (1, P)
        row = code if code <= d else 0
        _same_bits(f"{nm} of the hit GPs", _core(hB, nm, shape)[row, gps],
                   _core(h0, nm, shape)[row, gps])
        _same_bits("counters of the hit GPs", acc1[code, gps], acc0[code, gps])
    if name == "per_gp":                               # GP 7 never leaves ll = -inf
        assert _core(hB, "ll")[7] == -np.inf
    if name == "wos_current_minus_inf":
        _same_bits("ll after a rejected lamWOs", _core(hB, "ll")[7], -np.inf)


def merged_case(P, last):
    d = 5
    kinds, kinds_next = [2, d + 3, d + 1], [d + 2, 1, 3, 4]
    case = _case(ref.default_state(P, d, seed=31 + last), kinds, 1, last,
                 shift=_wos_shift(kinds, d, P, 1.0 if last else -1.0))
    case["kinds_next"] = kinds_next
    return case


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("P", [65, 200, 1024])
def test_merged_step_equals_decide_then_prep(dev, P, last):
    """gp_mcmc_group_step against gp_mcmc_group_decide + gp_mcmc_group_prep on a copy of the
    same buffers, every buffer bit for bit (last != 0, first != 0: a sweep's last group and the
    next sweep's first in one launch, which the sampler never issues)."""
    case = merged_case(P, last)
    kinds, nxt, first = case["kinds"], case["kinds_next"], last
    D = DeviceState(case["st"], dev, case["ll_all"], len(kinds))
    D.prep(kinds, 1)
    D.new_outputs(len(nxt))
    E = D.clone()
    before = D.host()
    D.decide(kinds, last)
    D.prep(nxt, first)
    E.step(kinds, last, nxt, first)
    two, one = D.host(), E.host()
    _guards_intact(one)
    for nm in two:
        _same_bits(nm, one[nm], two[nm])
    # the launches did something: decisions taken, proposals and Gram inputs written
    for nm in ("acc", "scratch", "beta", "s", "delta", "ll"):
        assert np.any(_bits(two[nm]) != _bits(before[nm])), nm
    assert np.any(_bits(two["lp"]) != _bits(before["lp"])) == bool(last)


@pytest.mark.parametrize("P,d,g", [(65, 5, 3), (1024, 32, 4)])
def test_same_inputs_same_bits(dev, P, d, g):
    case = shape_case(P, d, g)
    case["first"] = case["last"] = 1
    a, b = _run(dev, case), _run(dev, case)
    for ha, hb in zip(a, b):
        for nm in ha:
            _same_bits(nm, ha[nm], hb[nm])
