"""`usc_adamw_step_scaled`, the bucket-triggered optimizer and `trainer.TrainLoop` on the device.

The loop tests run in child processes (tests/train_loop_child.py), each with its own timeout; runs that several tests
look at are made once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "train_loop_child.py")


# ---------------------------------------------------------------------------------------------------------- 4. kernel
@pytest.mark.parametrize("write_back", [0, 1])
@pytest.mark.parametrize("n", [4096 + 1024, 4099, 3])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_scaled_adamw_equals_div_then_adamw_bit_for_bit(device, world, n, write_back):
    """`flat.div_(world)` + `usc_adamw_step` against `usc_adamw_step_scaled(grad_scale = f32(1) / f32(world))` on the
    sum: three consecutive steps under OneCycleLR (lr and beta1 change every step).  Zero tolerance: torch divides by a
    host scalar as a multiplication with its f32 reciprocal, which is the scale the kernel is given — world 3 included."""
    from unscene3d_amd._lib import check, lib
    from unscene3d_amd.ops import _ptr, _stream

    g = torch.Generator().manual_seed(100 * world + n)
    p0 = torch.randn(n, generator=g)
    pa, pb = p0.to(device), p0.to(device)
    ma, va = torch.zeros(n, device=device), torch.zeros(n, device=device)
    mb, vb = torch.zeros(n, device=device), torch.zeros(n, device=device)
    knob = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(knob, max_lr=1e-3, total_steps=10)
    scale = float(np.float32(1.0) / np.float32(world))
    for step in (1, 2, 3):
        grp = knob.param_groups[0]
        lr, (b1, b2), eps, wd = float(grp["lr"]), grp["betas"], float(grp["eps"]), float(grp["weight_decay"])
        total = (torch.randn(n, generator=g) * world).to(device)          # what the all-reduce leaves: the ranks' sum
        ga, gb = total.clone(), total.clone()
        ga.div_(world)
        check(lib.usc_adamw_step(_ptr(pa), _ptr(ga), _ptr(ma), _ptr(va), n, lr, float(b1), float(b2), eps, wd, step,
                                 _stream()), "usc_adamw_step")
        check(lib.usc_adamw_step_scaled(_ptr(pb), _ptr(gb), _ptr(mb), _ptr(vb), n, scale, write_back, lr, float(b1),
                                        float(b2), eps, wd, step, _stream()), "usc_adamw_step_scaled")
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), (world, n, step)
        assert torch.equal(gb, ga if write_back else total), (world, n, step, write_back)
        knob.step()
        sched.step()
    assert bool(torch.isfinite(pb).all()) and not torch.equal(pb.cpu(), p0)


def test_scaled_adamw_checks_its_arguments(device):
    from unscene3d_amd._lib import last_error, lib
    from unscene3d_amd.ops import _ptr, _stream
    t = torch.zeros(16, device=device)
    assert lib.usc_adamw_step_scaled(_ptr(t), _ptr(t), _ptr(t), _ptr(t), 8, 1.0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0,
                                     _stream()) != 0                    # step counts from 1
    assert "usc_adamw_step_scaled" in last_error()
    assert lib.usc_adamw_step_scaled(_ptr(t[1:]), _ptr(t), _ptr(t), _ptr(t), 8, 1.0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1,
                                     _stream()) != 0                    # 16-byte alignment
    assert "aligned" in last_error()


def test_early_modes_exclude_each_other_and_a_span_is_stepped_once(device):
    from unscene3d_amd.ddp import BucketedGradReducer, flatten_grads
    from unscene3d_amd.optim import FlatAdamW
    params = [torch.nn.Parameter(torch.randn(64, device=device)) for _ in range(3)]
    flat = flatten_grads(params)
    opt = FlatAdamW(params, flat_grad=flat)
    red = BucketedGradReducer(params, flat, 2, average=False)
    try:
        opt.enable_early_reduced(red)
        with pytest.raises(RuntimeError):
            opt.enable_early(torch.cuda.Stream())
        opt._on_reduced(0, 64, torch.cuda.current_stream())
        with pytest.raises(RuntimeError, match="already stepped"):
            opt._on_reduced(32, 96, torch.cuda.current_stream())
        opt.step()
        assert opt.callback_ranges == 1
        opt.disable_early()
        assert red.average and red.on_reduced is None
        opt.enable_early(torch.cuda.Stream())
        with pytest.raises(RuntimeError):
            opt.enable_early_reduced(BucketedGradReducer(params, flat, 2, average=False))
        # the views are checked before the first early launch of a step, not only in step()
        params[1].grad = torch.zeros(64, device=device)
        with pytest.raises(RuntimeError, match="no longer aliases"):
            opt._on_final([params[0]])
    finally:
        opt.disable_early()
        for h in red._hooks:
            h.remove()


# ---------------------------------------------------------------------------------------------------------- children
def _child(args, timeout=300, env=None):
    return subprocess.Popen([sys.executable, CHILD, *[str(x) for x in args]], cwd=ROOT, env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), timeout


def _wait(procs):
    for p, timeout in procs:
        try:
            _, err = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q, _ in procs:
                q.kill()
            raise
        assert p.returncode == 0, err[-3000:]


def _load(d, rank=0):
    return dict(np.load(os.path.join(d, f"rank{rank}.npz")))


def _same(a, b, names):
    for k in names:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """Four steps of the world-1 loop on bench.py's scene (`--rotate 0 --voxels 40000`)."""
    d = str(tmp_path_factory.mktemp("plain"))
    _wait([_child(["loop", "--out", d, "--steps", 4])])
    return d


def test_the_loop_is_the_bench_loop(plain, tmp_path):
    """bench.py --warmup 1 --steps 3 --dump-outputs against TrainLoop over the same scene, seed, overrides and
    schedule for the same four steps: every dumped array bit for bit.  Aligned, not tolerated: bench.py prepares the
    steady state after its first warm-up step when --warmup is 1, so the loop runs with steady_after=1."""
    out_dir = tmp_path / "bench"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--voxels", "40000", "--rotate", "0", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    mine = _load(plain)
    keys = json.load(open(os.path.join(plain, "keys0.json")))
    assert keys["early"] == "final"
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".npy"))
    assert {"loss.npy", "params_sample.npy", "grads_sample.npy", "loss_ce.npy", "loss_dice_11.npy"} <= set(files)
    assert np.array_equal(np.load(out_dir / "loss.npy"), mine["totals"][-1])
    assert np.array_equal(np.load(out_dir / "params_sample.npy"), mine["params_sample"])
    assert np.array_equal(np.load(out_dir / "grads_sample.npy"), mine["grads_sample"])
    loss_files = [f for f in files if f.startswith("loss_")]
    assert sorted(loss_files) == sorted(f"{k}.npy" for k in keys["keys"])
    for j, k in enumerate(keys["keys"]):
        assert np.array_equal(np.load(out_dir / f"{k}.npy"), mine["losses"][-1][j]), k
    # and what the loop reports through its pinned ring after a synchronise is the last step's vector
    assert int(mine["reported_step"]) == 4 and np.array_equal(mine["reported"], mine["losses"][-1])


STATE = ["params", "exp_avg", "exp_avg_sq", "losses", "totals"]


def test_one_rank_group_runs_the_same_program_and_changes_no_bit(plain, tmp_path):
    """force_dist over a one-rank RCCL group: reducer with average=False + bucket-triggered AdamW on the sum."""
    d = str(tmp_path / "forced")
    _wait([_child(["loop", "--out", d, "--steps", 4, "--force-dist", "--port", free_port()])])
    a, b = _load(plain), _load(d)
    assert json.load(open(os.path.join(d, "keys0.json")))["early"] == "reduced"
    _same(a, b, STATE)
    assert (b["callback_ranges"] >= 1).all(), b["callback_ranges"]
    assert (b["early_buckets"][1:] >= 1).all() and b["early_buckets"][0] == 0, b["early_buckets"]


def test_two_ranks_end_equal_with_and_without_the_bucket_triggered_optimizer(tmp_path):
    """Two gloo ranks on the one device: sum x 0.5 is exact, so the bucket-triggered optimizer on the sum ends with the
    bits of reducer-averages-then-one-launch, on both ranks."""
    res = {}
    for early in (1, 0):
        d, port = str(tmp_path / f"early{early}"), free_port()
        _wait([_child(["loop", "--out", d, "--steps", 4, "--world", 2, "--rank", r, "--port", port, "--backend", "gloo",
                       "--early", early]) for r in (0, 1)])
        res[early] = [_load(d, 0), _load(d, 1)]
        _same(res[early][0], res[early][1], ["params", "exp_avg", "exp_avg_sq"])
    _same(res[1][0], res[0][0], ["params", "exp_avg", "exp_avg_sq"])
    assert (res[1][0]["callback_ranges"] >= 1).all() and (res[0][0]["callback_ranges"] == 0).all()


def test_resume_continues_to_the_bit(tmp_path):
    """Six steps over two rotating scenes, against three steps -> save_checkpoint -> a fresh process -> resume -> three
    steps.  Leans on the step being run-to-run deterministic (tests/test_gpu_determinism.py)."""
    full, head, tail, ckpt = (str(tmp_path / n) for n in ("full", "head", "tail", "three.ckpt"))
    _wait([_child(["loop", "--out", full, "--steps", 6, "--scenes", 2])])
    _wait([_child(["loop", "--out", head, "--steps", 3, "--scenes", 2, "--save-at", 3, "--ckpt", ckpt])])
    _wait([_child(["loop", "--out", tail, "--steps", 3, "--scenes", 2, "--resume", ckpt])])
    a, h, t = _load(full), _load(head), _load(tail)
    _same(a, t, ["params", "exp_avg", "exp_avg_sq", "sched_last_epoch", "sched_lr", "opt_steps", "global_step", "epoch",
                 "position"])
    assert np.array_equal(a["losses"], np.concatenate([h["losses"], t["losses"]]))
    assert np.array_equal(a["totals"], np.concatenate([h["totals"], t["totals"]]))
    assert int(a["global_step"]) == 6 and int(a["epoch"]) == 3


@pytest.fixture(scope="module")
def misc(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("misc"))
    _wait([_child(["misc", "--out", d])])
    return json.load(open(os.path.join(d, "misc.json")))


def test_skipped_batch_and_clean_up(misc):
    s = misc["skip"]
    assert s["error"] is None and s["stepped"] == [True, False, True]
    assert s["batches"] == 3 and s["global_step"] == 2 and s["opt_steps"] == 2 and s["sched"] == 2 and s["skipped"] == 1
    assert s["early"] == "final"
    assert misc["hooks_after_close"] == [True, True]
    assert misc["losses"]["late_step"] == 3              # the second loop of the process ran its steps


def test_losses_without_a_wait(misc):
    m = misc["losses"]
    assert m["first_step"] == 2
    assert m["early_step"] == 2 and m["early_seconds"] < 0.05, m      # the compute stream was held back for 0.4 s
    assert m["late_step"] == 3 and m["late_equal"] and m["n_losses"] == 52


def test_validation_cadence(misc):
    v = misc["val"]
    assert v["files"] == ["best.ckpt", "last-epoch.ckpt"]
    assert "val_mean_ap_50" in v["metrics_keys"] and v["best"] is not None
    assert v["epoch"] == 2 and v["steps"] == 4 and v["training"] is True
    assert v["step_after"] and v["replays_after"] >= 1, v            # the captured decoder passes are still replayed
