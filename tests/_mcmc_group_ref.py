"""numpy restatement of the Metropolis group steps (gp_mcmc_group_prep / gp_mcmc_group_decide)
from their contract in include/gpfit.h (the gp_mcmc_state comment), and the inputs their tests
share.  Nothing here imports gladsgp_amd.mcmc or follows csrc/mcmc.hip's thread layout: every
quantity is a whole-array numpy expression over the P GPs, and the sums are in index order.

A state is a dict of numpy arrays named as the fields of gp_mcmc_state (betaU (d+1, P), lamUz,
lamWs, ll, lam, step_lamUz, step_lamWs (P,), lamWOs, step_lamWOs, lp (1,), step_betaU (d+1, P),
acc (d+4, P), u (nuniforms(d, P),), scratch (3, MAX_GROUP, P): planes cand, ok, dlp) plus the
plain entries P, d, dist, steptype, pa, pb, lo, hi.  ``prep`` and ``decide`` run in the dtype of
the state (``cast``): np.float64 states what a correct fp64 implementation computes,
np.longdouble is the high-precision reference, and their difference is how ill-conditioned a
quantity is.

Margins.  Every decision and range test is returned with the margin it was taken with, so a
test can require its inputs to be far from every threshold (and then expect every flag,
decision and counter to match exactly):
  decision  |log(ua) - rhs| (inf where the bounds or a non-finite rhs decide instead);
  bound     min over lo, hi of |x' - bound| / max(|x'|, |bound|) (inf for an infinite bound, or
            where rho's range already rejected);
  rho       min(|rho'|, |rho' - 1|) of a BetaRho move (inf for a Uniform move), with the side
            rho' fell on (-1: rho' <= 0, +1: rho' > 1, 0: in range).
"""
import numpy as np

GAMMA, BETA, NORMAL, UNIFORM = 0, 1, 2, 3          # GPFIT_MCMC_GAMMA ...
STEP_UNIFORM, STEP_BETARHO = 0, 1                  # GPFIT_MCMC_STEP_UNIFORM ...
MAX_GROUP = 4                                      # GPFIT_MCMC_MAX_GROUP
RHO_MAX = 0.999                                    # rho clipped in the Beta prior
ARRAYS = ("betaU", "lamUz", "lamWs", "lamWOs", "ll", "lam", "u", "step_betaU", "step_lamUz",
          "step_lamWs", "step_lamWOs", "acc", "lp", "scratch")
PARAMS = ("betaU", "lamUz", "lamWs", "lamWOs")


def nuniforms(d, P):
    return 2 * ((d + 1) * P + 2 * P + 1)


def cast(state, dtype):
    """A deep copy of ``state`` with its arrays in ``dtype`` (exact from float64)."""
    out = dict(state)
    for k in ARRAYS:
        out[k] = np.array(state[k], dtype=dtype, copy=True)
    return out


def _log_prior(st, p, x):
    T = x.dtype.type
    a, b = T(st["pa"][p]), T(st["pb"][p])
    fam = st["dist"][p]
    if fam == GAMMA:
        return (a - T(1)) * np.log(x) - b * x
    if fam == BETA:
        rho = np.minimum(np.exp(-x / T(4)), T(RHO_MAX))
        return (a - T(1)) * np.log(rho) + (b - T(1)) * np.log1p(-rho)
    if fam == NORMAL:
        t = (x - a) / b
        return T(-0.5) * (t * t)
    assert fam == UNIFORM
    return np.zeros_like(x)


def _update(st, code):
    """(current values (a view), step, proposal uniforms, acceptance uniforms, parameter index)
    of update ``code``: 0..d betaU row, d+1 lamUz, d+2 lamWs, d+3 lamWOs (one element)."""
    P, d = st["P"], st["d"]
    off = 2 * P * code                      # every earlier update took 2 P uniforms
    if code <= d:
        cur, step, p = st["betaU"][code], st["step_betaU"][code], 0
    elif code == d + 1:
        cur, step, p = st["lamUz"], st["step_lamUz"], 1
    elif code == d + 2:
        cur, step, p = st["lamWs"], st["step_lamWs"], 2
    else:
        assert code == d + 3
        cur, step, p = st["lamWOs"], st["step_lamWOs"], 3
    m = cur.shape[0]
    return cur, step, st["u"][off:off + m], st["u"][off + m:off + 2 * m], p


def _rel(x, bound):
    if not np.isfinite(bound):
        return np.full(x.shape, np.inf)
    den = np.maximum(np.abs(x), abs(bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, np.abs(x - bound) / den, 0.0).astype(np.float64)


def _propose(st, p, x, step, up):
    """Candidate (x where the move is rejected by rho's range or the bounds), in-range flag,
    prior difference and the margins of the range tests."""
    T = x.dtype.type
    lo, hi = T(st["lo"][p]), T(st["hi"][p])
    if st["steptype"][p] == STEP_BETARHO:
        rho = np.exp(-x / T(4)) + step * (up - T(0.5))
        ok_rho = (rho > 0) & (rho <= 1)
        raw = T(-4) * np.log(np.where(ok_rho, rho, T(1)))
        m_rho = np.minimum(np.abs(rho), np.abs(rho - T(1))).astype(np.float64)
        side = np.where(rho > 1, 1, np.where(rho <= 0, -1, 0))
    else:
        assert st["steptype"][p] == STEP_UNIFORM
        raw = x + step * (up - T(0.5))
        ok_rho = np.ones(x.shape, bool)
        m_rho = np.full(x.shape, np.inf)
        side = np.zeros(x.shape, int)
    ok = ok_rho & (raw >= lo) & (raw <= hi)
    m_bnd = np.where(ok_rho, np.minimum(_rel(raw, float(lo)), _rel(raw, float(hi))), np.inf)
    cand = np.where(ok, raw, x)
    dlp = _log_prior(st, p, cand) - _log_prior(st, p, x)
    return cand, ok, dlp, dict(rho=m_rho, bound=m_bnd, side=side)


def _decision(ok, ua, rhs):
    with np.errstate(invalid="ignore", divide="ignore"):
        lua = np.log(ua)
        acc = ok & (lua < rhs)                  # NaN compares false: rejected
        margin = np.where(ok & np.isfinite(rhs), np.abs(lua - rhs), np.inf).astype(np.float64)
    return acc, margin


def prep(st, kinds, first, dtype=np.float64):
    """gp_mcmc_group_prep.  ``first``: the prior-only move of betaU row 0 (state and counter in
    place).  Writes the group's candidates, flags and prior differences to the scratch planes
    and returns dict(beta ((2^g - 1) P, d), s, delta ((2^g - 1) P,), cand, ok, dlp ((g, P) views
    of the planes; lamWOs uses element 0 only), margins)."""
    assert st["betaU"].dtype == dtype
    T = np.dtype(dtype).type
    P, d, g = st["P"], st["d"], len(kinds)
    assert 1 <= g <= MAX_GROUP and len(set(kinds)) == g
    margins = dict(bound=[], rho=[], side=[])
    if first:
        cur, step, up, ua, p = _update(st, 0)
        cand, ok, dlp, m = _propose(st, p, cur, step, up)
        acc, md = _decision(ok, ua, dlp)
        cur[acc] = cand[acc]
        st["acc"][0] += acc
        margins["row0"] = dict(decision=md, accept=acc, ok=ok, **m)
    scr = st["scratch"]
    assert scr.shape == (3, MAX_GROUP, P)
    for i, code in enumerate(kinds):
        assert 1 <= code <= d + 3
        cur, step, up, ua, p = _update(st, code)
        cand, ok, dlp, m = _propose(st, p, cur, step, up)
        n = cur.shape[0]
        scr[0, i, :n], scr[1, i, :n], scr[2, i, :n] = cand, ok, dlp
        for k in ("bound", "rho", "side"):
            margins[k].append(m[k])
    nset = 2 ** g - 1
    beta = np.empty((nset * P, d), dtype)
    s = np.empty(nset * P, dtype)
    delta = np.empty(nset * P, dtype)
    for i in range(g):
        for pat in range(2 ** i):
            b = st["betaU"][1:].copy()
            lUz, lWs, lWO = st["lamUz"], st["lamWs"], st["lamWOs"][0]
            for q in range(i + 1):
                if q != i and not (pat >> q) & 1:
                    continue
                code = kinds[q]
                if code <= d:
                    b[code - 1] = scr[0, q]
                elif code == d + 1:
                    lUz = scr[0, q]
                elif code == d + 2:
                    lWs = scr[0, q]
                else:
                    lWO = scr[0, q, 0]
            rows = slice((2 ** i - 1 + pat) * P, (2 ** i + pat) * P)
            beta[rows] = b.T
            s[rows] = T(1) / lUz
            delta[rows] = T(1) / lWs + T(1) / (lWO * st["lam"])
    return dict(beta=beta, s=s, delta=delta, cand=scr[0, :g], ok=scr[1, :g], dlp=scr[2, :g],
                margins=margins)


def decide(st, kinds, last, ll_all, dtype=np.float64):
    """gp_mcmc_group_decide from the scratch planes ``prep`` left and ``ll_all``
    ((2^g - 1) P,): state, ll and counters in place; returns dict(lp (None unless ``last``; also
    stored in st["lp"]), accept (g, P) bool, slots (g, P) state set read per GP, margin (g, P))."""
    assert st["betaU"].dtype == dtype
    P, d, g = st["P"], st["d"], len(kinds)
    ll_all = np.asarray(ll_all, dtype=dtype).reshape(2 ** g - 1, P)
    scr = st["scratch"]
    gp = np.arange(P)
    pat = np.zeros(P, dtype=np.int64)
    accept = np.zeros((g, P), bool)
    slots = np.zeros((g, P), np.int64)
    margin = np.full((g, P), np.inf)
    for i, code in enumerate(kinds):
        cur, step, up, ua, p = _update(st, code)
        slots[i] = 2 ** i - 1 + pat
        lln = ll_all[slots[i], gp]
        with np.errstate(invalid="ignore"):
            diff = lln - st["ll"]
        if code == d + 3:                       # one decision on the in-order sum over the GPs
            tot = np.zeros(1, dtype)
            for v in diff:
                with np.errstate(invalid="ignore"):
                    tot = tot + v
            acc, md = _decision(scr[1, i, :1] != 0, ua, tot + scr[2, i, :1])
            if acc[0]:
                cur[0] = scr[0, i, 0]
                st["ll"][:] = lln
            st["acc"][code, 0] += acc[0]
            accept[i], margin[i] = acc[0], md[0]
        else:
            with np.errstate(invalid="ignore"):
                rhs = diff + scr[2, i]
            acc, md = _decision(scr[1, i] != 0, ua, rhs)
            cur[acc] = scr[0, i][acc]
            st["ll"][acc] = lln[acc]
            st["acc"][code] += acc
            accept[i], margin[i] = acc, md
        pat = pat | (accept[i].astype(np.int64) << i)
    lp = None
    if last:
        per_gp = st["ll"].copy()
        for r in range(d + 1):
            per_gp = per_gp + _log_prior(st, 0, st["betaU"][r])
        per_gp = per_gp + _log_prior(st, 1, st["lamUz"])
        per_gp = per_gp + _log_prior(st, 2, st["lamWs"])
        tot = np.zeros(1, dtype)
        for v in per_gp:
            tot = tot + v
        lp = tot + _log_prior(st, 3, st["lamWOs"])
        st["lp"][:] = lp
    return dict(lp=lp, accept=accept, slots=slots, margin=margin)


# ------------------------------------------------------------------------------------ inputs
DEFAULT_PRIORS = dict(dist=[BETA, GAMMA, GAMMA, GAMMA],
                      steptype=[STEP_BETARHO, STEP_UNIFORM, STEP_UNIFORM, STEP_UNIFORM],
                      pa=[1.0, 5.0, 3.0, 5.0], pb=[0.1, 5.0, 0.003, 0.005],
                      lo=[0.0, 0.3, 60.0, 60.0], hi=[np.inf, np.inf, 1e5, 1e5])


def default_state(P, d, seed):
    """A float64 state under the sampler's default priors: betaU ~ U(0.2, 5), lamUz ~ U(0.5, 3),
    lamWs ~ U(100, 5000), lamWOs 300, steps the defaults times U(0.5, 1.5), ll ~ N(-50, 10),
    counters small integers, lp and scratch recognisable finite values."""
    rng = np.random.default_rng([P, d, seed])
    st = dict(P=P, d=d, **{k: list(v) for k, v in DEFAULT_PRIORS.items()})
    st["betaU"] = rng.uniform(0.2, 5.0, (d + 1, P))
    st["lamUz"] = rng.uniform(0.5, 3.0, P)
    st["lamWs"] = rng.uniform(100.0, 5000.0, P)
    st["lamWOs"] = np.array([300.0])
    st["step_betaU"] = 0.1 * rng.uniform(0.5, 1.5, (d + 1, P))
    st["step_lamUz"] = 5.0 * rng.uniform(0.5, 1.5, P)
    st["step_lamWs"] = 100.0 * rng.uniform(0.5, 1.5, P)
    st["step_lamWOs"] = np.array([100.0 * rng.uniform(0.5, 1.5)])
    _common(st, rng)
    return st


def unit_state(P, d, seed, dist, steptype):
    """A float64 state whose four parameters all live in U(0.7, 3.7) with bounds [0.6, 3.8] (so
    both bounds reject), under the given families and step types: Gamma(3, 2), Beta(2, 3),
    Normal(2, 1) (prior differences O(1)); Uniform steps 2 U(0.5, 1.5), BetaRho steps
    1.6 U(0.5, 1.5) (rho = exp(-x / 4) in (0.39, 0.84), so rho' leaves (0, 1] both ways)."""
    rng = np.random.default_rng([P, d, seed, 7])
    pa = {GAMMA: 3.0, BETA: 2.0, NORMAL: 2.0, UNIFORM: 0.0}
    pb = {GAMMA: 2.0, BETA: 3.0, NORMAL: 1.0, UNIFORM: 1.0}
    st = dict(P=P, d=d, dist=list(dist), steptype=list(steptype),
              pa=[pa[f] for f in dist], pb=[pb[f] for f in dist], lo=[0.6] * 4, hi=[3.8] * 4)
    shapes = dict(betaU=(d + 1, P), lamUz=(P,), lamWs=(P,), lamWOs=(1,))
    for p, nm in enumerate(PARAMS):
        st[nm] = rng.uniform(0.7, 3.7, shapes[nm])
        scale = 1.6 if steptype[p] == STEP_BETARHO else 2.0
        st["step_" + nm] = scale * rng.uniform(0.5, 1.5, shapes[nm])
    _common(st, rng)
    return st


def _common(st, rng):
    P, d = st["P"], st["d"]
    st["lam"] = rng.uniform(1.0, 10.0, P)
    st["ll"] = -50.0 + 10.0 * rng.standard_normal(P)
    st["u"] = rng.random(nuniforms(d, P))
    st["acc"] = rng.integers(0, 5, (d + 4, P)).astype(np.float64)
    st["lp"] = np.array([-12345.678])
    st["scratch"] = 7000.0 + np.arange(3 * MAX_GROUP * P, dtype=np.float64).reshape(
        3, MAX_GROUP, P)


def draw_ll_all(st, g, seed, shift=None):
    """ll_all ((2^g - 1) P,): the current ll plus N(0, 2) per state set and GP; ``shift``
    (2^g - 1,) is added per state set (to steer the shared lamWOs decision)."""
    P = st["P"]
    rng = np.random.default_rng([P, st["d"], g, seed, 11])
    out = st["ll"][None, :] + 2.0 * rng.standard_normal((2 ** g - 1, P))
    if shift is not None:
        out = out + np.asarray(shift, dtype=np.float64)[:, None]
    return out.reshape(-1)
