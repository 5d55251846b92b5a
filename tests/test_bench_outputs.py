"""bench.py --dump-outputs: the last timed step's outputs as .npy files (float32 / float64, 64 MB at most, fixed samples of what is
larger), and the plain run's line: `steps` timed steps, `ms_per_step`, no --full legs."""
import importlib.util
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fake_path(n, gathered=None, latent=None):
    g = torch.Generator().manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4096, 512), torch.nn.Linear(512, 64))
    return SimpleNamespace(losses=[torch.tensor(9.0), torch.tensor(1.5), torch.tensor(2.5)], my_voters=[0, 1],
                           mean=torch.rand(4096, dtype=torch.float64, generator=g), scale=torch.rand(4096, dtype=torch.float64, generator=g),
                           feats=torch.rand((4, n, 4096), generator=g), last_model=SimpleNamespace(net=net), gathered=gathered, latent=latent)


def test_dump_outputs_cpu(tmp_path):
    """On CPU tensors: every output is written, in float32 / float64, within the budget; the store is sampled by rows with the fixed
    seed (the same rows every time), what fits is written whole, the losses are the last step's."""
    bench = _bench()
    n = 1200                                                      # [4, 1200, 4096] float32 = 75 MB: sampled
    hp = _fake_path(n, gathered=torch.randint(0, 20, (8, 3000), dtype=torch.int32))
    bench.dump_outputs(hp, str(tmp_path / "a"))
    bench.dump_outputs(hp, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["epoch_loss.npy", "scaler_mean.npy", "scaler_scale.npy", "features.npy", "assignments.npy", "net_0_weight.npy",
                            "net_0_bias.npy", "net_1_weight.npy", "net_1_bias.npy"]), names
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    f = np.load(tmp_path / "a" / "features.npy")
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, f.shape[1], replace=False))
    assert f.shape[0] == 4 and 0 < f.shape[1] < n and np.array_equal(f, hp.feats.numpy()[:, rows])
    assert np.array_equal(np.load(tmp_path / "a" / "epoch_loss.npy"), [1.5, 2.5])
    assert np.array_equal(np.load(tmp_path / "a" / "scaler_mean.npy"), hp.mean.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "net_0_weight.npy"), hp.last_model.net[0].weight.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "assignments.npy"), hp.gathered.numpy().astype(np.float32))


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_outputs(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` on a small synthetic batch: one line with `steps` == 2 and `ms_per_step`,
    none of the --full legs, and the outputs of its last timed step -- identical inputs on a second run, so the feature store and
    the scaler come out the same."""
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "5000", "--steps", "2",
                            "--warmup", "1", "--dump-outputs", str(tmp_path / d)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(line) == 1, r.stdout[-2000:]
        lines.append(json.loads(line[0]))
    j = lines[0]
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "sequences/sec" and j["dtype"] == "f32"
    for leg in ("cpu_baseline", "t_e2e", "fixed_job_8_voters", "k_sweep", "fp32_step_form", "cfg5_one_gpu", "exchange_ms"):
        assert leg not in j, leg
    total = 0
    for name in os.listdir(tmp_path / "a"):
        a = np.load(tmp_path / "a" / name)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), name
        total += a.nbytes
    assert total <= 64 << 20
    f = np.load(tmp_path / "a" / "features.npy")
    assert f.shape[0] == 4 and 0 < f.shape[1] <= 5000 and f.shape[2] == 4096 and np.allclose(f.astype(np.float64).sum(2), 1.0, atol=1e-5)
    assert np.load(tmp_path / "a" / "epoch_loss.npy").shape == (1,)
    assert np.array_equal(f, np.load(tmp_path / "b" / "features.npy"))
    for name in ("scaler_mean.npy", "scaler_scale.npy"):
        np.testing.assert_allclose(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name), rtol=1e-12, atol=0, err_msg=name)
