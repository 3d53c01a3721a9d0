"""bench.py must be runnable as `python bench.py --gpus N`: without a launcher's
environment it starts the N ranks itself and relays rank 0's JSON line (no GPU needed
to check that: the child process is faked)."""

import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KSP_BENCH_FORCE_LAUNCH"):
        monkeypatch.delenv(var, raising=False)
    import bench as module

    return module


def test_self_launch_command_and_relay(bench, monkeypatch, capsys):
    seen = {}

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"] = cmd
        seen["env"] = env
        line = json.dumps({"metric": "m", "value": 1.0, "n_gpus": 4})
        return types.SimpleNamespace(returncode=0, stdout="NCCL banner\n" + line + "\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    assert bench.main() == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1 :] == ["--gpus", "4", "--steps", "5", "--warmup", "2"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    lines = [x for x in out.out.splitlines() if x.strip()]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 4  # exactly one JSON line
    assert "NCCL banner" in out.err


def test_self_launch_propagates_failure(bench, monkeypatch, capsys):
    monkeypatch.setattr(
        subprocess, "run",
        lambda cmd, env=None, stdout=None, text=None: types.SimpleNamespace(returncode=3, stdout=""),
    )
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    assert bench.main() == 3
    assert capsys.readouterr().out == ""


def test_rank_mismatch_is_an_error(bench, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit):
        bench.main()


def test_inject_rfi_is_deterministic_and_sparse(bench):
    import numpy as np

    a = bench.inject_rfi(bench.synth_block(64, 512, 1), seed=3)
    b = bench.inject_rfi(bench.synth_block(64, 512, 1), seed=3)
    assert np.array_equal(a, b)
    strong = np.abs(a) > 40
    assert 0.04 < strong.mean() < 0.09


def test_dump_outputs_whole_when_it_fits(bench, tmp_path):
    import numpy as np

    flags = (np.arange(6 * 10).reshape(6, 10) % 3 == 0).astype(np.uint8)
    noise = np.linspace(0.5, 1.5, 10, dtype=np.float32)
    bench.dump_outputs(str(tmp_path), {"flags": flags, "noise": noise}, 1 << 20, "_rank1")
    got = np.load(tmp_path / "flags_rank1.npy")
    assert got.dtype == np.float32 and np.array_equal(got, flags)
    assert np.array_equal(np.load(tmp_path / "noise_rank1.npy"), noise)


def test_dump_outputs_samples_the_same_baselines_within_budget(bench, tmp_path):
    import numpy as np

    channels, baselines, budget = 64, 5000, 300_000
    rs = np.random.RandomState(5)
    flags = (rs.random_sample((channels, baselines)) < 0.1).astype(np.uint8)
    noise = rs.random_sample(baselines).astype(np.float32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"flags": flags, "noise": noise}, budget)
    files = sorted((tmp_path / "a").iterdir())
    assert [f.name for f in files] == ["flags.npy", "noise.npy"]
    assert sum(f.stat().st_size for f in files) <= budget
    got_flags, got_noise = (np.load(f) for f in files)
    assert got_flags.dtype == got_noise.dtype == np.float32
    assert got_flags.shape[0] == channels and 0 < got_flags.shape[1] == got_noise.shape[0] < baselines
    # the same columns of both outputs, and the same sample from run to run
    cols = np.flatnonzero(np.isin(noise, got_noise))
    assert np.array_equal(noise[cols], got_noise) and np.array_equal(flags[:, cols], got_flags)
    for name in ("flags.npy", "noise.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))


def test_steps_must_be_positive(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.main()
