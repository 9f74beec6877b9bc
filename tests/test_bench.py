"""bench.py's own options: ``--dump-outputs`` (the last timed step's answers as .npy files) and
the split between a plain run (set-up, warm-up, the timed steps, the line) and ``--full`` (the
auxiliary rooflines and the CPU baseline with its parity check beside them).

The GPU test runs the benchmark itself, as a child process, at a small C3 (n = 600, past the
column-resident kernel's 512 and no multiple of the tile, so the headline's Gram / factorisation
/ cross-covariance / pair-TRMM path; m = 3000: two chunks of 2048 test points, the second
partial); the oracle runs once for both runs.
Tolerances are SURVEY §8c's for C3 (max|dmean| <= 1e-8 max(1, |mean|), max|dvar| <= 1e-8 s),
which the full-size parity test (tests/test_gpu_c3.py) uses at n = 4096."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, D = 600, 3000, 8


def _bench():
    import bench
    return bench


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    """dump_outputs keeps float32 / float64, widens anything else to float64, and past its byte
    limit cuts every array by the same factor to the same sorted sample on every call."""
    bench = _bench()
    a = torch.arange(4000, dtype=torch.float64).reshape(40, 100)
    b = torch.arange(1000, dtype=torch.float32)
    c = torch.arange(10)
    bench.dump_outputs(str(tmp_path / "all"), {"a": a, "b": b, "c": c})
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in "abc"}
    assert got["a"].dtype == np.float64 and got["a"].shape == (40, 100)
    assert got["b"].dtype == np.float32 and got["c"].dtype == np.float64
    np.testing.assert_array_equal(got["a"], a.numpy())
    np.testing.assert_array_equal(got["c"], np.arange(10.0))
    total = a.numel() * 8 + b.numel() * 4
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", total // 4)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    s1 = {k: np.load(tmp_path / "s1" / f"{k}.npy") for k in "ab"}
    s2 = {k: np.load(tmp_path / "s2" / f"{k}.npy") for k in "ab"}
    assert s1["a"].shape == (1000,) and s1["b"].shape == (250,)
    assert s1["a"].nbytes + s1["b"].nbytes <= total // 4
    for k in "ab":
        np.testing.assert_array_equal(s1[k], s2[k])
        assert np.all(np.diff(s1[k]) >= 0)          # values = indices here: a sorted sample
    assert set(s1["a"]) <= set(a.reshape(-1).numpy())


def _run_bench(*extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--n", str(N), "--m", str(M), "--d", str(D), "--m-chunk", "2048"]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_and_full_runs(tmp_path):
    """A plain run prints the headline line without the figures that take runs of their own and,
    with --dump-outputs, writes the last timed step's mean and variance (float64, all m points),
    which match the oracle; --full reports the auxiliary rooflines and the CPU baseline with its
    parity, and dumps the same inputs' answers again."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from oracle import gp_ref
    bench = _bench()
    X, y, beta, Xs, s, delta = bench.c3_inputs(N, M, D)
    mean_ref, var_ref = gp_ref.predict(X, Xs, y, beta, s, delta)

    def check_dump(d):
        assert sorted(os.listdir(d)) == ["mean.npy", "var.npy"]
        mean, var = np.load(d / "mean.npy"), np.load(d / "var.npy")
        assert mean.dtype == np.float64 and var.dtype == np.float64
        assert mean.shape == (M,) and var.shape == (M,)
        dm = float(np.max(np.abs(mean - mean_ref)))
        dv = float(np.max(np.abs(var - var_ref)))
        print(f"dump vs oracle: max|dmean|={dm:.3e} max|dvar|={dv:.3e}")
        assert dm <= 1e-8 * max(1.0, float(np.max(np.abs(mean_ref))))
        assert dv <= 1e-8 * s
        return mean, var

    plain = _run_bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["n_gpus"] == 1
    assert plain["unit"] == "predictions/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f64" and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(M / (plain["ms_per_step"] * 1e-3), rel=1e-9)
    assert plain["roofline"]["launches"] > 0
    assert plain["roofline_aux"] is None and plain["cpu_baseline"] is None
    mean_p, var_p = check_dump(tmp_path / "plain")

    full = _run_bench("--full", "--cpu-sample", "2000", "--cpu-faithful-batches", "1",
                      "--dump-outputs", str(tmp_path / "full"))
    assert full["metric"] == plain["metric"] and full["steps"] == 2
    for k in ("gram", "potrf_inv", "cross"):
        assert full["roofline_aux"][k]["achieved"] > 0
    par = full["cpu_baseline"]["parity_vs_gpu"]
    assert par["points"] == 2000
    assert par["max_abs_dmean"] <= 1e-8 * max(1.0, float(np.max(np.abs(mean_ref))))
    assert par["max_abs_dvar"] <= 1e-8 * s
    mean_f, var_f = check_dump(tmp_path / "full")
    # the same inputs from run to run: two runs of one build agree far inside the tolerance
    assert float(np.max(np.abs(mean_f - mean_p))) <= 1e-12 * max(1.0,
                                                                 float(np.max(np.abs(mean_ref))))
    assert float(np.max(np.abs(var_f - var_p))) <= 1e-12
