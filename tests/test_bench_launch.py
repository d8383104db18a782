"""Host logic of bench.py's launcher (no GPU): `--gpus N` without WORLD_SIZE re-executes through
torch.distributed.run with N ranks on 127.0.0.1; with WORLD_SIZE set it must equal --gpus."""
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_spawn_command(monkeypatch):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=0)

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert bench.spawn_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"]
    assert cmd[-7] == os.path.join(ROOT, "bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and seen["env"]["MASTER_ADDR"] == "127.0.0.1"


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "--gpus 8 but WORLD_SIZE=1" in out.stderr


def test_full_is_off_by_default_and_dumps_are_float_arrays(tmp_path):
    """A plain run does only what the headline needs (--full opts in to the rest); --dump-outputs writes float arrays:
    the losses by name and the same seeded sample of the parameters and of their gradients on every run."""
    import numpy as np
    import torch

    bench = _load_bench()
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs is None
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True
    torch.manual_seed(0)
    lin = torch.nn.Linear(1500, 1000)
    lin(torch.randn(4, 1500)).square().sum().backward()
    params = list(lin.parameters())
    a = bench.step_outputs(torch.tensor(2.5), {"loss_ce": torch.tensor(0.5)}, params)
    b = bench.step_outputs(torch.tensor(2.5), {"loss_ce": torch.tensor(0.5)}, params)
    assert a["params_sample"].shape == (bench.DUMP_SAMPLE,) and torch.equal(a["params_sample"], b["params_sample"])
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([p.grad.reshape(-1) for p in params])
    idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(flat_p.numel(), bench.DUMP_SAMPLE, replace=False)))
    assert torch.equal(a["params_sample"], flat_p[idx]) and torch.equal(a["grads_sample"], flat_g[idx])
    bench.dump_outputs(str(tmp_path), a)
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(got) == {"loss.npy", "loss_ce.npy", "params_sample.npy", "grads_sample.npy"}
    assert all(v.dtype == np.float32 for v in got.values()) and float(got["loss.npy"]) == 2.5
