"""bench.py --dump-outputs and the plain / --full split.

* dump_outputs (CPU): dtypes, the byte budget, and a sample that is the same
  from call to call.
* A plain run on the GPU writes the last timed step's answer, equal to the true
  order statistic of the same generated keys, and carries none of the --full
  legs; --full adds them.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, true_kth


def _bench():
    spec = importlib.util.spec_from_file_location("kth_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * 8 * 1000)  # 1000 float64 per array
    big = torch.arange(5000, dtype=torch.int64) * (1 << 40)  # beyond float32's integers
    arrays = {"i32": torch.tensor([[-2 ** 31, 2 ** 31 - 1]], dtype=torch.int32),
              "f32": torch.linspace(-1, 1, 2000, dtype=torch.float32).reshape(40, 50),
              "i64": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in arrays}
    assert a["i32"].dtype == np.float64 and a["i32"].tolist() == [[-2.0 ** 31, 2.0 ** 31 - 1]]
    # under its share (2000 float32 <= 8000 B / 4): whole, shape kept
    assert a["f32"].dtype == np.float32 and np.array_equal(a["f32"], arrays["f32"].numpy())
    # over its share: 1000 elements at sorted positions, exact, the same both times
    assert a["i64"].dtype == np.float64 and a["i64"].shape == (1000,)
    assert np.all(np.diff(a["i64"]) >= 0) and set(a["i64"].tolist()) <= set(big.double().tolist())
    assert len(set(a["i64"].tolist())) > 500
    assert all(np.array_equal(a[n], b[n]) for n in arrays)
    assert sum(x.nbytes for x in a.values()) <= 3 * 8 * 1000


def _run(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "KTH_RDV_FILE")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--log2n", "20", *args],
                       capture_output=True, text=True, timeout=240, env=env, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_dumps_last_answer(gpu, oracle, tmp_path):
    import torch
    plain = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    n = 1 << 20
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.fill(keys, n, "uniform_half", 0x5EED0001, offset=0, n_total=n)  # bench.py's defaults
    gpu.sync()
    want = true_kth(oracle, keys.cpu().numpy(), n // 2)
    assert os.listdir(tmp_path / "a") == ["kth.npy"]
    got = np.load(tmp_path / "a" / "kth.npy")
    assert got.dtype == np.float64 and got.shape == (1,)
    assert got[0] == want and plain["answer"] == want
    assert plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["full"] is False and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(n / (plain["ms_per_step"] * 1e-3) / 1e9)
    for key in ("verified", "roofline", "cpu_baseline", "cpu_baseline_cgm", "ms_per_step_events"):
        assert key not in plain, key


@pytest.mark.gpu
def test_full_run_adds_its_legs():
    line = _run(["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert line["full"] is True and line["verified"] is True
    assert line["roofline"]["avg_launch_ms"] > 0 and line["ms_per_step_events"] > 0
