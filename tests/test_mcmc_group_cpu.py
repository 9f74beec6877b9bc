"""CPU: the numpy restatement of the group steps (tests/_mcmc_group_ref.py), chained over whole
sweeps, against the oracle chain (oracle/mcmc_ref.py, one update at a time) fed the same
uniforms.  The likelihood is test_mcmc_spec_cpu's CPU stand-in for gp_loglik, so this checks the
restatement the GPU tests (tests/test_gpu_mcmc_group.py) compare the kernels with: the uniform
layout, the state sets, the per-GP and shared decisions, the counters and the log posterior."""
import numpy as np
import pytest
import torch

import _mcmc_group_ref as ref
from oracle import mcmc_ref
from test_mcmc_spec_cpu import _cpu_loglik, _problem

FAMILY = {"Gamma": ref.GAMMA, "Beta": ref.BETA, "Normal": ref.NORMAL, "Uniform": ref.UNIFORM}
STEP = {"Uniform": ref.STEP_UNIFORM, "BetaRho": ref.STEP_BETARHO}

SPECS = {
    "default": {"betaU": ("Beta", (1.0, 0.1), (0.0, np.inf), "BetaRho"),
                "lamUz": ("Gamma", (5.0, 5.0), (0.3, np.inf), "Uniform"),
                "lamWs": ("Gamma", (3.0, 0.003), (60.0, 1e5), "Uniform"),
                "lamWOs": ("Gamma", (5.0, 0.005), (60.0, 1e5), "Uniform")},
    "mixed": {"betaU": ("Beta", (1.0, 0.1), (0.0, np.inf), "BetaRho"),
              "lamUz": ("Normal", (1.5, 1.0), (0.3, np.inf), "Uniform"),
              "lamWs": ("Uniform", (0.0, 1.0), (60.0, 1e5), "Uniform"),
              "lamWOs": ("Gamma", (5.0, 0.005), (60.0, 1e5), "Uniform")},
}


def _loglik(X, w, lam, betaU, lamUz, lamWs, lamWOs):
    t = torch.as_tensor
    return _cpu_loglik(t(X), t(np.ascontiguousarray(betaU[1:].T)), t(1.0 / lamUz),
                       t(1.0 / lamWs + 1.0 / (lamWOs * lam)), t(w), None).numpy()


@pytest.mark.parametrize("priors", ["default", "mixed"])
@pytest.mark.parametrize("spec", [1, 2, 3, 4])
def test_chained_groups_match_oracle_chain(spec, priors):
    n, d, P, nsw = 20, 3, 3, 30
    X, w, lam = _problem(n, d, P, seed=4)
    sp = SPECS[priors]
    start = {"betaU": np.full((d + 1, P), 0.1), "lamUz": np.full(P, 1.0),
             "lamWs": np.full(P, 1000.0), "lamWOs": 1000.0}
    steps = {"betaU": np.full((d + 1, P), 0.1), "lamUz": np.full(P, 5.0),
             "lamWs": np.full(P, 100.0), "lamWOs": np.full(1, 100.0)}
    U = np.random.default_rng(5).random((nsw, ref.nuniforms(d, P)))
    _, want, acc = mcmc_ref.run_chain(X, w, lam, sp, start, steps, U)

    rows = [sp[nm] for nm in ref.PARAMS]
    st = dict(P=P, d=d, dist=[FAMILY[r[0]] for r in rows], steptype=[STEP[r[3]] for r in rows],
              pa=[r[1][0] for r in rows], pb=[r[1][1] for r in rows],
              lo=[r[2][0] for r in rows], hi=[r[2][1] for r in rows])
    for nm in ref.PARAMS:
        st[nm] = np.array(start[nm], dtype=np.float64).reshape((d + 1, P) if nm == "betaU" else -1)
        st["step_" + nm] = steps[nm].copy()
    st["lam"] = lam.copy()
    st["ll"] = _loglik(X, w, lam, st["betaU"], st["lamUz"], st["lamWs"], st["lamWOs"][0])
    st["acc"] = np.zeros((d + 4, P))
    st["lp"] = np.zeros(1)
    st["scratch"] = np.zeros((3, ref.MAX_GROUP, P))
    codes = list(range(1, d + 4))
    groups = [codes[i:i + spec] for i in range(0, len(codes), spec)]
    tw = torch.as_tensor(w)
    got = {k: [] for k in ref.PARAMS}
    patterns = set()
    for u in U:
        st["u"] = u.copy()
        for gi, kinds in enumerate(groups):
            out = ref.prep(st, kinds, first=gi == 0)
            ll_all = _cpu_loglik(torch.as_tensor(X), torch.as_tensor(out["beta"]),
                                 torch.as_tensor(out["s"]), torch.as_tensor(out["delta"]),
                                 tw.repeat(2 ** len(kinds) - 1, 1), None).numpy()
            dec = ref.decide(st, kinds, gi == len(groups) - 1, ll_all)
            if len(kinds) == spec and d + 3 not in kinds:
                patterns |= set((dec["accept"] << np.arange(spec)[:, None]).sum(0).tolist())
        for k in ref.PARAMS:
            got[k].append(st[k].reshape(-1).copy())
        # the log posterior of the state reached, from the oracle's own pieces
        lp = np.sum(_loglik(X, w, lam, st["betaU"], st["lamUz"], st["lamWs"], st["lamWOs"][0]))
        for nm in ref.PARAMS:
            lp += np.sum(mcmc_ref.log_prior(sp[nm][0], sp[nm][1], st[nm]))
        assert abs(dec["lp"][0] - lp) <= 1e-9 * abs(lp)
        assert st["lp"][0] == dec["lp"][0]
    for k in ref.PARAMS:
        np.testing.assert_allclose(np.array(got[k]), want[k], rtol=1e-9, atol=1e-12, err_msg=k)
    np.testing.assert_array_equal(st["acc"][:d + 1], acc["betaU"])
    np.testing.assert_array_equal(st["acc"][d + 1], acc["lamUz"])
    np.testing.assert_array_equal(st["acc"][d + 2], acc["lamWs"])
    assert st["acc"][d + 3, 0] == acc["lamWOs"] and not st["acc"][d + 3, 1:].any()
    # both outcomes occurred inside the groups, so the state-set selection was exercised
    if spec > 1:
        assert len(patterns) > 2


def test_longdouble_run_takes_the_same_decisions():
    """The two precisions differ only by rounding: the same flags, decisions and state sets, and
    values apart by a few ulp of the quantity's conditioning."""
    P, d, kinds = 65, 5, [2, 8, 6, 4]
    st64 = ref.default_state(P, d, seed=0)
    ll_all = ref.draw_ll_all(st64, len(kinds), seed=0)
    stld = ref.cast(st64, np.longdouble)
    p64, pld = ref.prep(st64, kinds, True), ref.prep(stld, kinds, True, np.longdouble)
    d64 = ref.decide(st64, kinds, True, ll_all)
    dld = ref.decide(stld, kinds, True, ll_all, np.longdouble)
    assert p64["beta"].dtype == np.float64 and pld["beta"].dtype == np.longdouble
    np.testing.assert_array_equal(p64["ok"], pld["ok"])
    np.testing.assert_array_equal(d64["accept"], dld["accept"])
    np.testing.assert_array_equal(d64["slots"], dld["slots"])
    np.testing.assert_array_equal(st64["acc"], stld["acc"])
    for k in ("beta", "s", "delta", "dlp"):
        assert np.max(np.abs(p64[k] - pld[k])) < 1e-12, k
    assert 0 < abs(d64["lp"][0] - dld["lp"][0]) < 1e-9
    assert d64["margin"][np.isfinite(d64["margin"])].min() > 1e-8


def test_documented_slot_and_uniform_layout():
    """Hand-checkable case: P = 2, d = 1, group (lamWOs, betaU row 1): set 0 proposes lamWOs,
    sets 1 and 2 propose row 1 after lamWOs was rejected / accepted."""
    P, d = 2, 1
    st = ref.default_state(P, d, seed=3)
    st["u"] = np.arange(ref.nuniforms(d, P)) / 100.0 + 0.3
    b1, wos, lam = st["betaU"][1].copy(), st["lamWOs"][0], st["lam"]
    out = ref.prep(st, [4, 1], first=False)
    # lamWOs is update d + 3 = 4: uniforms 2 P 4 = 16 (proposal) and 17 (acceptance)
    wos_c = wos + st["step_lamWOs"][0] * (st["u"][16] - 0.5)
    rho = np.exp(-b1 / 4.0) + st["step_betaU"][1] * (st["u"][4:6] - 0.5)
    b1_c = -4.0 * np.log(rho)
    np.testing.assert_array_equal(out["cand"][0, 0], wos_c)
    np.testing.assert_array_equal(out["cand"][1], b1_c)
    np.testing.assert_array_equal(out["beta"][:, 0], np.concatenate([b1, b1_c, b1_c]))
    d0 = 1.0 / st["lamWs"] + 1.0 / (wos * lam)
    d1 = 1.0 / st["lamWs"] + 1.0 / (wos_c * lam)
    np.testing.assert_array_equal(out["delta"], np.concatenate([d1, d0, d1]))
    np.testing.assert_array_equal(out["s"], np.tile(1.0 / st["lamUz"], 3))
    # scratch: the lamWOs row holds one element, the rest of it stays as it was
    assert st["scratch"][0, 0, 1] == 7001.0 and st["scratch"][0, 2, 0] == 7000.0 + 2 * P
