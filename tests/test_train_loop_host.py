"""CPU, world size 2 over gloo on host tensors: the reducer's `average=False` / `on_reduced` contract, its unchanged
defaults, and `configure_optimizers`' unchanged default."""
import copy
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import free_port


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unscene3d_amd.ddp import BucketedGradReducer, flatten_grads
        torch.manual_seed(1)
        net = torch.nn.Sequential(*[torch.nn.Linear(12, 12) for _ in range(6)])
        twin = copy.deepcopy(net)                    # same weights, the default reducer: what `flat` holds today
        params, tparams = list(net.parameters()), list(twin.parameters())
        flat, tflat = flatten_grads(params), flatten_grads(tparams)
        calls = []
        red = BucketedGradReducer(params, flat, world, bucket_bytes=1200, average=False,
                                  on_reduced=lambda lo, hi, stream: calls.append((lo, hi, stream, flat[lo:hi].clone())))
        ref = BucketedGradReducer(tparams, tflat, world, bucket_bytes=1200)
        assert ref.average and ref.on_reduced is None and len(red.bounds) >= 3
        per_step = []
        for it in range(3):
            xin = torch.full((4, 12), float(rank + 1 + it))
            twin.zero_grad(set_to_none=False)
            ref.begin_step()
            twin(xin).square().sum().backward()
            ref.finish()
            net.zero_grad(set_to_none=False)
            red.begin_step()
            del calls[:]
            net(xin).square().sum().backward()
            during = len(calls)
            red.finish()
            # once per bucket, the ranges tile the flat buffer exactly
            assert len(calls) == len(red.bounds), (it, len(calls))
            assert sorted((lo, hi) for lo, hi, _, _ in calls) == sorted(red.bounds)
            assert sorted(red.bounds)[0][0] == 0 and sorted(red.bounds)[-1][1] == flat.numel()
            assert all(a[1] == b[0] for a, b in zip(sorted(red.bounds), sorted(red.bounds)[1:]))
            assert all(st is None for _, _, st, _ in calls)              # host tensors: the call is synchronous
            # what the callback saw in its range is the finished sum, and sum / world is the default reducer's mean
            for lo, hi, _, seen in calls:
                assert torch.equal(seen, flat[lo:hi])
            assert torch.equal(flat / world, tflat), it
            assert (during == 0) if it == 0 else (during >= len(red.bounds) - 1), (it, during)
            per_step.append([(lo, hi) for lo, hi, _, _ in calls])
        got = [None] * world
        dist.all_gather_object(got, per_step)
        assert got[0] == got[1]                                          # the same call order on every rank
        out[rank] = per_step
    finally:
        dist.destroy_process_group()


def test_reducer_reports_reduced_buckets_and_leaves_the_sum():
    world, port = 2, free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    assert set(res) == {0, 1} and res[0] == res[1]
    # eligible buckets report from the last to the first (the order backward finishes them) from the second step on
    assert res[0][1] == sorted(res[0][1], reverse=True)


def _default_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unscene3d_amd.ddp import BucketedGradReducer, flatten_grads
        torch.manual_seed(3)
        net = torch.nn.Sequential(*[torch.nn.Linear(8, 8) for _ in range(3)])
        twin = copy.deepcopy(net)
        params = list(net.parameters())
        flat, tflat = flatten_grads(params), flatten_grads(list(twin.parameters()))
        red = BucketedGradReducer(params, flat, world, bucket_bytes=300)
        for it in range(2):
            xin = torch.full((2, 8), float(rank + 1 + it))
            twin.zero_grad(set_to_none=False)
            twin(xin).sum().backward()
            local = tflat.clone()
            net.zero_grad(set_to_none=False)
            red.begin_step()
            net(xin).sum().backward()
            red.finish()
            gathered = [torch.zeros_like(local) for _ in range(world)]
            dist.all_gather(gathered, local)
            assert torch.equal(flat, (gathered[0] + gathered[1]) / world), it       # still divides
        assert red.on_reduced is None and red.average is True
        out[rank] = True
    finally:
        dist.destroy_process_group()


def test_default_reducer_still_divides_and_never_calls_back():
    world, port = 2, free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_default_worker, args=(world, port, out), nprocs=world, join=True)
        assert dict(out) == {0: True, 1: True}


def test_configure_optimizers_default_is_torch_adamw_over_all_parameters():
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.trainer import InstanceSegmentation, TrainLoop, fit  # noqa: F401  (the loop is exported)

    cfg = apply_overrides(default_config(), ["general.num_targets=3"])
    torch.manual_seed(0)
    module = InstanceSegmentation(cfg)
    opt, sched = module.configure_optimizers(steps_per_epoch=10, epochs=2)
    assert type(opt) is torch.optim.AdamW
    held = {id(p) for g in opt.param_groups for p in g["params"]}
    assert held == {id(p) for p in module.parameters()}
    assert any(".backbone.final." in n for n, _ in module.named_parameters())
    assert isinstance(sched, torch.optim.lr_scheduler.OneCycleLR) and sched.total_steps == 20
    _, sched2 = module.configure_optimizers(10, 2, total_steps=77)
    assert sched2.total_steps == 77
