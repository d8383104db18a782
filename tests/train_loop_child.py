"""Child process of tests/test_gpu_train_loop.py (not collected: no test_ prefix): builds a `TrainLoop` the way
`bench.py --mode mask3d` builds its step (same config overrides, seed, scenes, schedule) and writes what it computed.

    python train_loop_child.py loop --out DIR --steps K [--scenes S] [--voxels V] [--force-dist] [--world W --rank R
                                    --port P --backend gloo] [--early 0|1] [--steady-after N] [--save-at K --ckpt PATH]
                                    [--resume PATH]
    python train_loop_child.py misc --out DIR        skipped batch + clean-up, losses without a wait, validation cadence
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DUMP_SAMPLE = 1 << 20


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["loop", "misc"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--scenes", type=int, default=1)
    ap.add_argument("--voxels", type=int, default=40000)
    ap.add_argument("--force-dist", action="store_true")
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--early", type=int, default=1)
    ap.add_argument("--steady-after", type=int, default=1)
    ap.add_argument("--save-at", type=int, default=0)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--resume", default=None)
    return ap.parse_args()


def build(world=1):
    """bench.make_mask3d_step's config, seed and module."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.trainer import InstanceSegmentation
    cfg = apply_overrides(default_config(), ["general.num_targets=3", f"data.batch_size={world}"])
    torch.manual_seed(1234)
    module = InstanceSegmentation(cfg).to("cuda:0").train()
    return cfg, module


def scene_list(n, voxels, base=2000):
    """Scene j: bench.py's rotation slot j (seed 2000 + 16 j; slot 0 is the scene of `--rotate 0`)."""
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    return [SyntheticFreeMaskDataset(n_scenes=1, target_voxels=voxels, seed=base + 16 * j)[0] for j in range(n)]


def sample_like_bench(params):
    """bench.step_outputs: the fixed seeded sample of the concatenated parameters and of their gradients."""
    with torch.no_grad():
        p = torch.cat([q.detach().reshape(-1) for q in params])
        g = torch.cat([q.grad.detach().reshape(-1) for q in params])
        n = p.numel()
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(n, min(n, DUMP_SAMPLE), replace=False))).to(p.device)
        return p[idx].cpu().numpy(), g[idx].cpu().numpy()


def run_loop(a):
    from unscene3d_amd.trainer import TrainLoop
    dist_on = a.world > 1 or a.force_dist
    if a.world > 1:                                  # ranks share the one device: second streams off, like bench.py does
        os.environ.setdefault("USC3D_WGRAD_LANE_MAX_ROWS", "0")
        os.environ.setdefault("USC3D_KV_SIDE_STREAM", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if dist_on:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(a.port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(a.backend, rank=a.rank, world_size=a.world,
                                **({"device_id": dev} if a.backend == "nccl" else {}))
    cfg, module = build(a.world)
    scenes = scene_list(max(a.scenes, a.world), a.voxels)
    kw = dict(device=dev, world=a.world, rank=a.rank, force_dist=a.force_dist, early_optimizer=bool(a.early),
              total_steps=100000, steady_after=a.steady_after, resident=True, seed=7)
    loop = TrainLoop.resume(a.resume, module, cfg, scenes, **kw) if a.resume else TrainLoop(module, cfg, scenes, **kw)
    totals, vecs, cb, early_buckets = [], [], [], []
    for k in range(a.steps):
        total = loop.step()
        assert total is not None
        totals.append(total.clone())
        vecs.append(loop.last_losses.clone())
        cb.append(loop.optimizer.callback_ranges)
        early_buckets.append(loop.reducer.started_during_backward if loop.reducer is not None else 0)
        if a.save_at and k + 1 == a.save_at:
            loop.save_checkpoint(a.ckpt)
    torch.cuda.synchronize()
    rep = loop.losses()
    ps, gs = sample_like_bench(loop.params)
    os.makedirs(a.out, exist_ok=True)
    sched = loop.scheduler.state_dict()
    np.savez(os.path.join(a.out, f"rank{a.rank}.npz"),
             params=loop.optimizer.flat_param.cpu().numpy(), exp_avg=loop.optimizer.exp_avg.cpu().numpy(),
             exp_avg_sq=loop.optimizer.exp_avg_sq.cpu().numpy(), totals=torch.stack(totals).cpu().numpy(),
             losses=torch.stack(vecs).cpu().numpy(), params_sample=ps, grads_sample=gs,
             callback_ranges=np.asarray(cb), early_buckets=np.asarray(early_buckets),
             reported=np.asarray([rep["losses"][k] for k in loop._loss_keys], dtype=np.float32),
             reported_step=rep["step"], sched_last_epoch=sched["last_epoch"], sched_lr=np.float64(sched["_last_lr"][0]),
             opt_steps=loop.optimizer.steps, global_step=loop.global_step, epoch=loop.epoch, position=loop.pos)
    with open(os.path.join(a.out, f"keys{a.rank}.json"), "w") as f:
        json.dump({"keys": loop._loss_keys, "early": loop.early}, f)
    loop.close()
    if dist_on:
        torch.distributed.destroy_process_group()


def run_misc(a):
    from unscene3d_amd import graphs, ops
    from unscene3d_amd._lib import check, lib
    from unscene3d_amd.trainer import TrainLoop
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg, module = build()
    out = {}

    # ---- a target-less scene between two normal ones; clean-up; a second loop in the same process
    s = scene_list(2, 40000)
    empty = list(s[1])
    table = empty[2].copy()
    table[:, 1:-1] = 0
    empty[2] = table
    scenes = [s[0], tuple(empty), s[1]]
    err = None
    loop = TrainLoop(module, cfg, scenes, device=dev, total_steps=1000, shuffle=False, steady_after=0)
    try:
        got = [loop.step() is not None for _ in range(3)]
    except RuntimeError as e:       # (zero_grad's early-range guard would land here)
        err, got = str(e), []
    torch.cuda.synchronize()
    out["skip"] = {"stepped": got, "batches": loop.batches, "global_step": loop.global_step, "skipped": loop.skipped,
                   "opt_steps": loop.optimizer.steps, "sched": loop.scheduler.state_dict()["last_epoch"], "error": err,
                   "early": loop.early}
    loop.close()
    out["hooks_after_close"] = [ops.PARAMS_FINAL_HOOK is None, ops.GRAD_WRITTEN_HOOK is None]

    # ---- second loop: losses without a wait
    loop = TrainLoop(module, cfg, [s[0]], device=dev, total_steps=1000, steady_after=0)
    loop.step()
    loop.step()
    torch.cuda.synchronize()
    first = loop.losses()
    for _ in range(4):                            # holds the compute stream back for 0.4 s (100 ms per launch at most)
        check(lib.usc_spin(100_000, 1, torch.cuda.current_stream().cuda_stream), "usc_spin")
    loop.step()                                   # issued behind the spin
    want = loop.last_losses
    t0 = time.perf_counter()
    early = loop.losses()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    late = loop.losses()
    out["losses"] = {"first_step": first["step"], "early_step": early["step"], "early_seconds": dt,
                     "late_step": late["step"],
                     "late_equal": bool(np.array_equal(np.asarray([late["losses"][k] for k in loop._loss_keys], np.float32),
                                                       want.cpu().numpy())),
                     "n_losses": len(late["losses"])}
    loop.close()

    # ---- validation cadence: two epochs of two small scenes, validation after each
    cfg.trainer.check_val_every_n_epoch = 1
    cfg.general.filter_out_instances = True
    cfg.general.topk_per_image = 30
    cfg.general.scores_threshold = 0.0
    val = scene_list(2, 8000, base=6100)
    gt = {}
    for xyz, _, table, name, *_ in val:               # GT: the first synthetic mask column of each point
        cols = table[:, 1:-1] != 0
        gt[name] = np.where(cols.any(1), 1000 + cols.argmax(1) + 1, 0).astype(np.int64)
    ckpt_dir = os.path.join(a.out, "ckpt")
    loop = TrainLoop(module, cfg, s, device=dev, total_steps=1000, steady_after=0, val_scenes=val, val_gt_ids=gt,
                     out_dir=ckpt_dir)
    res = loop.run(epochs=2)
    before = graphs.STATS["grad_buffer_hits"] + graphs.STATS["grad_out_copies"]
    after_val = loop.step() is not None
    torch.cuda.synchronize()
    replays = graphs.STATS["grad_buffer_hits"] + graphs.STATS["grad_out_copies"] - before
    out["val"] = {"metrics_keys": sorted(res["metrics"]), "monitor": res["metrics"].get("val_mean_ap_50"),
                  "best": res["best"], "files": sorted(os.listdir(ckpt_dir)), "training": module.training,
                  "step_after": after_val, "replays_after": replays, "epoch": res["epoch"], "steps": res["steps"],
                  "passes": module.model.num_levels * module.model.num_decoders}
    loop.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "misc.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    args = parse()
    (run_loop if args.mode == "loop" else run_misc)(args)
