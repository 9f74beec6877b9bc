"""GPU: the device emits exactly the task list tests/test_pp_sched_cpu.py proved safe, this
device's launches are safe by the same model, and the factorisation does not depend on what its
scratch held.

gp_pp_schedule launches pp_schedule_kernel alone (through the launch helper the factorisation
uses), so N = 240 tile rows costs a few milliseconds and no 15360 x 15360 matrix.
"""
import ctypes

import numpy as np
import pytest
import torch

import _pp_sched_ref as ref
from oracle import gp_ref

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gladsgp_amd import kernels  # noqa: F401 (loads libgpfit.so)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from gladsgp_amd import _capi
    return _capi.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _plan_stream(lib, dev, n, batch, inv, lead=-1):
    from gladsgp_amd import _capi
    out = (ctypes.c_longlong * len(_capi.PP_PLAN))()
    assert lib.gp_pp_plan_stream(n, batch, inv, lead, out, _stream(dev)) == 0
    p = dict(zip(_capi.PP_PLAN, out))
    # the same report as the host form gives for that residency
    out2 = (ctypes.c_longlong * len(_capi.PP_PLAN))()
    assert lib.gp_pp_plan(n, batch, inv, p["resident"], lead, out2) == 0
    assert list(out) == list(out2)
    return p


def _host_list(lib, n, inv, lead):
    count = lib.gp_pp_schedule_host(n, inv, lead, None, 0)
    assert count >= 0
    buf = np.zeros((max(count, 1), 3), dtype=np.int32)
    assert lib.gp_pp_schedule_host(n, inv, lead, buf.ctypes.data, count) == count
    return buf[:count].astype(np.int64)


def _align256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 33, 64, 239, 240])
def test_device_list_equals_host_list(dev, lib, N, inv):
    """Scratch prefilled with 0xFF: afterwards the task list is the host's, word for word, the
    header and every flag word are 0, and no other byte changed -- the list's and the flags'
    padding, and a guard region past the scratch size."""
    W = _plan_stream(lib, dev, 64, 1, inv)["kPPLead"]
    for lead, n in ((0, 64 * N), (W, 64 * N - 63)):
        one = _host_list(lib, n, inv, lead)
        for batch in (1, 3, 8) + ((257,) if N <= 12 else ()):   # 257 > the 256 schedule blocks
            size = lib.gp_pp_schedule_ws_bytes(n, batch, inv)
            total = batch * (len(one) + 1)
            task_bytes = _align256(total * 8)
            fstride = (2 * N * N + 2 * N + 1 + 31) // 32 * 32
            flag_end = task_bytes + 256 + batch * fstride * 4
            assert size == task_bytes + _align256(256 + batch * fstride * 4)
            buf = torch.full((size + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 256 == 0
            assert lib.gp_pp_schedule(n, batch, inv, lead, buf.data_ptr(), size, _stream(dev)) == 0
            torch.cuda.synchronize()
            raw = buf.cpu().numpy()
            got = raw[:total * 8].view(np.int32).reshape(-1, 2)
            want = ref.encode(ref.batched(one, batch))
            assert np.array_equal(got, want), (N, inv, lead, batch)
            assert np.all(raw[total * 8:task_bytes] == 0xFF)
            assert not raw[task_bytes:flag_end].any(), "header and flag words must be 0"
            assert np.all(raw[flag_end:] == 0xFF), "bytes past the flag words were written"


@pytest.mark.parametrize("n,batch", [(4096, 1), (1024, 32), (512, 24), (512, 128), (512, 256),
                                     (1000, 6), (1000, 16), (256, 8)])
def test_this_device_plan_is_safe(dev, lib, n, batch):
    """The shapes the suite and the benchmark factorise, with this device's residency: where
    the persistent kernel runs, its grid, queues and lead cannot deadlock on the real list."""
    for inv in (0, 1):
        p = _plan_stream(lib, dev, n, batch, inv)
        print(f"n={n} batch={batch} inv={inv}: {p}")
        assert p["resident"] >= 1 and p["N"] == -(-n // 64)
        if not p["eligible"]:
            assert 2 * batch > p["resident"]
            continue
        e = ref.batched(_host_list(lib, n, inv, p["lead"]), batch)
        assert len(e) == batch * (p["tasks"] + 1)
        assert ref.layout_errors(e, batch, p["groups"]) == []
        profs = ref.queue_profiles(e, p["N"], p["groups"])
        G, B = p["grid"] // p["groups"], batch // p["groups"]
        assert p["grid"] % p["groups"] == 0
        for q in profs:
            assert q.final_blocked == 0 and not q.deadlocks(G), (p, q.max_blocked)
            if p["grid"] < len(e):
                assert q.max_stuck < G - B, (p, q.max_stuck)


def _spd_batch(n, B, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, 8))
    return np.stack([gp_ref.gram_ardse(X, rng.uniform(0.5, 5, 8), 1.0, 1e-4) for _ in range(B)])


@pytest.mark.parametrize("n,B", [(200, 3), (1000, 8)])
def test_scratch_contents_do_not_matter(dev, lib, n, B):
    """gp_potrf_inv_ws and gp_potrf_ws on a workspace prefilled with 0xFF and on a zero-filled
    one: info 0 and the same bits of L, L^-1 and logdet, which meet test_gpu_kernels.py's bounds
    against LAPACK."""
    from gladsgp_amd import _capi, kernels
    assert _plan_stream(lib, dev, n, B, 1)["eligible"] and _plan_stream(lib, dev, n, B, 0)["eligible"]
    G = _spd_batch(n, B, 1000 + n)
    npad = kernels.padded_n(n)
    Lref = np.linalg.cholesky(G)

    def run(name, fill):
        A = torch.as_tensor(G, device=dev).contiguous()
        info = torch.full((B,), 77, dtype=torch.int32, device=dev)
        logdet = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
        if name == "gp_potrf_inv_ws":
            ws = torch.full((int(lib.gp_potrf_inv_ws_bytes(n, B)),), fill, dtype=torch.uint8,
                            device=dev)
            Linv = torch.zeros((B, npad, npad), dtype=torch.float64, device=dev)
            _capi.call(name, A.data_ptr(), n, n, n * n, Linv.data_ptr(), npad, npad * npad, B,
                       info.data_ptr(), logdet.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        else:
            ws = torch.full((int(lib.gp_potrf_ws_bytes(n, B)),), fill, dtype=torch.uint8,
                            device=dev)
            Linv = None
            _capi.call(name, A.data_ptr(), n, n, n * n, B, info.data_ptr(), logdet.data_ptr(),
                       ws.data_ptr(), ws.numel(), _stream(dev))
        torch.cuda.synchronize()
        assert ws.data_ptr() % 256 == 0
        assert info.cpu().tolist() == [0] * B
        L = np.tril(A.transpose(1, 2).cpu().numpy())              # [b][row][col]
        X = None if Linv is None else Linv.transpose(1, 2).cpu().numpy()
        return L, X, logdet.cpu().numpy()

    for name in ("gp_potrf_inv_ws", "gp_potrf_ws"):
        L, X, logdet = run(name, 0xFF)
        L0, X0, logdet0 = run(name, 0)
        assert np.array_equal(L, L0) and np.array_equal(logdet, logdet0), name
        for b in range(B):
            assert np.linalg.norm(L[b] @ L[b].T - G[b]) / np.linalg.norm(G[b]) <= 1e-13
            assert np.max(np.abs(L[b] - Lref[b])) <= 1e-10 * np.max(np.abs(Lref[b]))
            np.testing.assert_allclose(logdet[b], 2 * np.sum(np.log(np.diag(Lref[b]))), rtol=0,
                                       atol=1e-9 * n)
        if X is not None:
            assert np.array_equal(X, X0), name
            for b in range(B):
                assert np.max(np.abs(X[b][:n, :n] @ L[b] - np.eye(n))) <= 1e-9
                assert np.all(np.triu(X[b], 1) == 0)
                assert np.all(X[b][n:, :] == 0) and np.all(X[b][:, n:] == 0)
