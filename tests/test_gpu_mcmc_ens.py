"""GPU: mcmc.EnsembleSampler (C chains per batched sweep), tune_step_sizes_ensemble,
emulator.fit_ensemble and EmulatorModel.do_mcmc_chains.  Every chain of an ensemble must be the
chain a lone GPUSampler produces from the same generator (1e-12: the tolerance
test_speculative_groups_same_chain holds across batch compositions) and the oracle's chain
(oracle/mcmc_ref.py, 1e-9 as in test_chain_matches_oracle)."""
import numpy as np
import pytest
import torch

from gladsgp_amd import emulator, mcmc
from oracle import mcmc_ref
from test_gpu_mcmc import _problem, _spec, _t

pytestmark = pytest.mark.gpu
KEYS = ("betaU", "lamUz", "lamWs", "lamWOs", "logPost")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ensemble_problem(n, d, P, C, seed):
    """One design, C different sets of PC weights and LamSim."""
    X, w0, lam0 = _problem(n, d, P, seed)
    ws, lams = [w0], [lam0]
    for c in range(1, C):
        _, w, lam = _problem(n, d, P, seed + 1000 * c)
        ws.append(w)
        lams.append(lam)
    return X, np.stack(ws), np.stack(lams)


def _params(d, P, C, scale=1.0):
    """C ModelParams with the shared default priors and chain-specific starts and steps."""
    out = []
    for c in range(C):
        pr = mcmc.ModelParams(d, P)
        for k in pr.names:
            p = getattr(pr, k)
            p.mcmcStepParam = p.mcmcStepParam * scale * (1.0 + 0.1 * c)
        pr["lamUz"] = pr.lamUz.val * (1.0 + 0.2 * c)
        pr["betaU"] = pr.betaU.val * (1.0 + 0.5 * c)
        out.append(pr)
    return out


def _lone(dev, X, w, lam, pr, seed, nsw, **kw):
    s = mcmc.GPUSampler(_t(X, dev), _t(w, dev), _t(lam, dev), pr, **kw)
    return s, s.run(nsw, np.random.default_rng(seed))


# one lone run and one oracle run per (shape, chain), shared by the spec / graph cases
_REFS = {}


def _references(dev, n, d, P, C, scale, nsw):
    key = (n, d, P, C)
    if key not in _REFS:
        X, w, lam = _ensemble_problem(n, d, P, C, seed=11 + n)
        lone, oracle = [], []
        for c, pr in enumerate(_params(d, P, C, scale)):
            state = {"betaU": pr.betaU.val.copy(), "lamUz": pr.lamUz.val[0].copy(),
                     "lamWs": pr.lamWs.val[0].copy(), "lamWOs": pr.lamWOs.val[0, 0]}
            steps = {k: getattr(pr, k).mcmcStepParam for k in pr.names}
            U = np.random.default_rng(50 + c).random((nsw, mcmc.uniforms_per_sweep(d, P)))
            _, chain, acc = mcmc_ref.run_chain(X, w[c], lam[c], _spec(pr), state, steps, U)
            oracle.append((chain, acc))
            s, rec = _lone(dev, X, w[c], lam[c], pr, 50 + c, nsw, use_graph=False)
            lone.append((rec, s.counts()))
        _REFS[key] = (X, w, lam, lone, oracle)
    return _REFS[key]


@pytest.mark.parametrize("spec,graph", [(1, False), (2, True), (3, False), (3, True)])
@pytest.mark.parametrize("n,d,P,C,scale", [(48, 2, 3, 3, 1.0), (48, 2, 1, 5, 1.0),
                                           (130, 3, 2, 2, 0.3), (48, 2, 3, 1, 1.0)])
def test_chain_equals_lone_sampler_and_oracle(dev, n, d, P, C, scale, spec, graph):
    nsw = 25
    X, w, lam, lone, oracle = _references(dev, n, d, P, C, scale, nsw)
    ens = mcmc.EnsembleSampler(_t(X, dev), _t(w, dev), _t(lam, dev), _params(d, P, C, scale),
                               use_graph=graph, spec=spec)
    rec = ens.run(nsw, [np.random.default_rng(50 + c) for c in range(C)])
    cnt = ens.counts()
    exact = True
    for c in range(C):
        lrec, lcnt = lone[c]
        chain, acc = oracle[c]
        for k in KEYS:
            assert rec[k].shape == (C,) + lrec[k].shape
            np.testing.assert_allclose(rec[k][c], lrec[k], rtol=1e-12, atol=1e-12,
                                       err_msg=f"chain {c} {k} vs the lone sampler")
            exact = exact and np.array_equal(rec[k][c], lrec[k])
        for k in KEYS[:4]:
            np.testing.assert_allclose(rec[k][c], chain[k], rtol=1e-9, atol=1e-12,
                                       err_msg=f"chain {c} {k} vs the oracle")
        for k in lcnt:
            np.testing.assert_array_equal(cnt[c][k], lcnt[k], err_msg=f"chain {c} {k}")
        np.testing.assert_array_equal(np.stack([cnt[c][("betaU", r)] for r in range(d + 1)]),
                                      acc["betaU"])
        np.testing.assert_array_equal(cnt[c]["lamUz"], acc["lamUz"])
        np.testing.assert_array_equal(cnt[c]["lamWs"], acc["lamWs"])
        assert cnt[c]["lamWOs"][0] == acc["lamWOs"]
        assert acc["betaU"][1:].sum() > 0 and cnt[c]["lamUz"].sum() > 0
    if C == 1:
        # an ensemble of one and the lone sampler at the same spec issue the same calls
        s, lrec = _lone(dev, X, w[0], lam[0], _params(d, P, C, scale)[0], 50, nsw,
                        use_graph=graph, spec=spec)
        for k in KEYS:
            np.testing.assert_array_equal(rec[k][0], lrec[k], err_msg=k)
        for k, v in s.counts().items():
            np.testing.assert_array_equal(cnt[0][k], v, err_msg=str(k))
    else:
        # chains differ from each other (different w_hat, starts and uniforms)
        assert not np.allclose(rec["lamUz"][0], rec["lamUz"][1])
    print(f"\nensemble vs lone sampler n={n} P={P} C={C} spec={spec} graph={graph}: "
          f"{'bit-exact' if exact else 'within 1e-12, not bit-exact'}")


def test_slices_of_whole_chains(dev):
    """C = 5 with max_batch holding two chains of the largest group: slices of 2, 2, 1 chains
    give the chains of one slice bit for bit."""
    n, d, P, C, spec, nsw = 48, 2, 3, 5, 2, 12
    X, w, lam = _ensemble_problem(n, d, P, C, seed=7)
    recs, cnts = [], []
    for max_batch in (None, 2 * (2 ** spec - 1) * P + 1):
        ens = mcmc.EnsembleSampler(_t(X, dev), _t(w, dev), _t(lam, dev), _params(d, P, C),
                                   use_graph=False, spec=spec, max_batch=max_batch)
        chunks = {sets: b["chunk"] for sets, b in ens._gbuf.items()}
        recs.append(ens.run(nsw, [np.random.default_rng(c) for c in range(C)]))
        cnts.append(ens.counts())
    # groups (1, 2), (3, 4), (5): three state sets x P = 9 rows per chain, 19 // 9 = 2 chains per
    # slice (batches 18, 18, 9); the single-set group and init_state: all 5 chains (15) at once
    assert chunks == {2 ** spec - 1: 2, 1: 6} and sorted(ens._ws) == [9, 15, 18]
    for k in KEYS:
        np.testing.assert_array_equal(recs[1][k], recs[0][k], err_msg=k)
    for a, b in zip(*cnts):
        for k in a:
            np.testing.assert_array_equal(b[k], a[k])


def test_group_size_follows_the_batch_limit(dev):
    n, d, P, C = 48, 2, 3, 2
    X, w, lam = _ensemble_problem(n, d, P, C, seed=7)
    args = (_t(X, dev), _t(w, dev), _t(lam, dev))
    ens = mcmc.EnsembleSampler(*args, _params(d, P, C), max_batch=10)
    assert ens.spec == 2 and all(b["chunk"] >= 1 for b in ens._gbuf.values())   # 3 P <= 10 < 7 P
    with pytest.raises(ValueError, match="max_batch"):
        mcmc.EnsembleSampler(*args, _params(d, P, C), max_batch=P - 1)
    with pytest.raises(ValueError, match="spec 3"):
        mcmc.EnsembleSampler(*args, _params(d, P, C), spec=3, max_batch=10)
    bad = _params(d, P, C)
    bad[1].lamWs.bounds = (1.0, np.inf)
    with pytest.raises(ValueError, match=r"lamWs\.bounds"):
        mcmc.EnsembleSampler(*args, bad)
    # the default limit is the persistent factorisation's range on this stream
    lim = mcmc.loglik_max_batch(n, dev)
    assert lim is not None and lim >= 8
    assert mcmc.EnsembleSampler(*args, _params(d, P, C)).max_batch == lim


def test_block_graph_equals_eager(dev):
    """2 block + 7 sweeps: whole blocks replayed as one graph, the rest one sweep at a time; the
    chains, records and counters equal the eager sweep's bit for bit."""
    n, d, P, C, block = 64, 3, 4, 2, 5
    X, w, lam = _ensemble_problem(n, d, P, C, seed=51)
    recs, cnts = [], []
    for graph in (False, True):
        ens = mcmc.EnsembleSampler(_t(X, dev), _t(w, dev), _t(lam, dev), _params(d, P, C),
                                   use_graph=graph)
        ens.block = block
        rngs = [np.random.default_rng(17 + c) for c in range(C)]
        ens.run(block + 3, rngs, record=False)
        recs.append(ens.run(2 * block + 7, rngs, block=block + 4))
        cnts.append(ens.counts())
    assert recs[1]["lamUz"].shape == (C, 2 * block + 7, P)
    for k in KEYS:
        np.testing.assert_array_equal(recs[1][k], recs[0][k], err_msg=k)
    for a, b in zip(*cnts):
        for k in a:
            np.testing.assert_array_equal(b[k], a[k])


def test_tune_step_sizes_ensemble(dev):
    n, d, P, C, n_burn, n_levels = 48, 2, 3, 2, 15, 3
    X, w, lam = _ensemble_problem(n, d, P, C, seed=21)
    plist = _params(d, P, C)
    ens = mcmc.EnsembleSampler(_t(X, dev), _t(w, dev), _t(lam, dev), plist)
    mcmc.tune_step_sizes_ensemble(ens, n_burn, n_levels,
                                  [np.random.default_rng(c) for c in range(C)])
    ens.write_back()
    for c, pr in enumerate(_params(d, P, C)):
        s = mcmc.GPUSampler(_t(X, dev), _t(w[c], dev), _t(lam[c], dev), pr)
        mcmc.tune_step_sizes(s, n_burn, n_levels, np.random.default_rng(c))
        s.write_back()
        for k in pr.names:
            np.testing.assert_allclose(getattr(plist[c], k).mcmcStepParam,
                                       getattr(pr, k).mcmcStepParam, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(getattr(plist[c], k).val, getattr(pr, k).val,
                                       rtol=1e-12, atol=1e-12)
            np.testing.assert_array_equal(ens.last_tune[c]["accepts"][k],
                                          s.last_tune["accepts"][k])
        assert np.any(plist[c].betaU.mcmcStepParam != mcmc.ModelParams(d, P).betaU.mcmcStepParam)


def _scalar_models(dev, n, d, C, seed):
    """C scalar (P = 1) emulators on one design, as fit_scalar_models.py builds them."""
    rng = np.random.default_rng(seed)
    t = rng.random((n, d))
    models = []
    for c in range(C):
        y = np.sin(2 * np.pi * t @ rng.uniform(0, 1, d) + c)[:, None] * rng.uniform(1, 2, (1, 6))
        y = y + 1e-2 * rng.standard_normal(y.shape)
        data = emulator.EmulatorData(t, y, device=dev)
        data.standardize_y()
        K = np.linalg.svd(data.sim_data.y_std.cpu().numpy(), full_matrices=False)[2][:1]
        data.create_K_basis(K)
        m = emulator.EmulatorModel(data)
        m.rng = np.random.default_rng(100 + c)
        models.append(m)
    return models


def test_fit_ensemble_equals_fitting_alone(dev):
    n, d, C = 40, 2, 3
    together = emulator.fit_ensemble(_scalar_models(dev, n, d, C, seed=3), 12, 3, 20)
    alone = _scalar_models(dev, n, d, C, seed=3)
    for a, b in zip(alone, together):
        a.tune_step_sizes(12, 3)
        a.do_mcmc(20)
        for k in KEYS:
            assert b.samples[k].shape == a.samples[k].shape
            np.testing.assert_allclose(b.samples[k], a.samples[k], rtol=1e-12, atol=1e-12,
                                       err_msg=k)
        for k in a.params.names:
            np.testing.assert_allclose(getattr(b.params, k).mcmcStepParam,
                                       getattr(a.params, k).mcmcStepParam, rtol=1e-12, atol=0)
            np.testing.assert_allclose(getattr(b.params, k).val, getattr(a.params, k).val,
                                       rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(b.tune_info["accepts"]["lamUz"],
                                      a.tune_info["accepts"]["lamUz"])
    # a second call appends, as do_mcmc does
    emulator.fit_ensemble(together, 0, 0, 5, tune=False)
    assert together[0].samples["lamUz"].shape == (25, 1)
    bad = _scalar_models(dev, n, d, 2, seed=3)
    bad[1].params.lamUz.params = [4.0, 5.0]
    with pytest.raises(ValueError, match=r"lamUz\.params"):
        emulator.fit_ensemble(bad, 12, 3, 20)


def test_do_mcmc_chains(dev):
    n, d, C, N, seed = 40, 2, 3, 18, 123
    m = _scalar_models(dev, n, d, 1, seed=5)[0]
    m.do_mcmc(4)
    before = {k: v.copy() for k, v in m.samples.items()}
    vals = m.params.values()
    chains = m.do_mcmc_chains(N, C, seeds=[seed, 1, 2])
    assert chains is m.chains
    P = m.P
    assert {k: v.shape for k, v in chains.items()} == {
        "betaU": (C, N, (d + 1) * P), "lamUz": (C, N, P), "lamWs": (C, N, P),
        "lamWOs": (C, N, 1), "logPost": (C, N, 1)}
    for k in before:                                   # samples and values untouched
        np.testing.assert_array_equal(m.samples[k], before[k])
    for k, v in vals.items():
        np.testing.assert_array_equal(m.params[k], v)
    # chains 1, 2 start dispersed: they differ from chain 0 and from each other
    assert not np.allclose(chains["lamUz"][1], chains["lamUz"][0])
    assert not np.allclose(chains["lamUz"][2], chains["lamUz"][1])
    diag = m.chain_diagnostics(nburn=2)
    assert set(diag) == {"rhat", "ess"} and diag["rhat"]["betaU"].shape == ((d + 1) * P,)
    assert diag["ess"]["lamWOs"].shape == (1,)
    # chain 0 is do_mcmc's chain under the same generator
    m.rng = np.random.default_rng(seed)
    m.samples = None
    m.do_mcmc(N)
    for k in KEYS:
        np.testing.assert_allclose(chains[k][0], m.samples[k], rtol=1e-12, atol=1e-12,
                                   err_msg=k)
    # given starts are used as they are; default seeds are spawned from model.rng
    start = {k: v.copy() for k, v in vals.items()}
    start["lamUz"] = np.full((1, P), 2.5)
    given = m.do_mcmc_chains(3, 2, starts=[None, start], seeds=[seed, 9])
    assert abs(given["lamUz"][1, 0, 0] - 2.5) <= 5.0 / 2 + 1e-12       # one Uniform step of 5
    assert given["lamUz"].shape == (2, 3, P)
    m.rng = np.random.default_rng(4)
    a = m.do_mcmc_chains(3, 2)
    m.rng = np.random.default_rng(4)
    b = m.do_mcmc_chains(3, 2)
    np.testing.assert_array_equal(a["betaU"], b["betaU"])
    assert not np.array_equal(a["betaU"][0], a["betaU"][1])
