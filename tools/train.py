"""Run the training loop (`unscene3d_amd.trainer.TrainLoop`) on synthetic scenes and print one JSON line.

    python tools/train.py --synthetic 8 --voxels 150000 --steps 40 [--force-dist] [--no-early-optimizer]
                          [--resume PATH] [--out DIR] [--no-shuffle] [--supervised]

--synthetic N: the N rotated scenes of `bench.py`'s default workload (sizes spread over +-2 % of --voxels, the largest
first).  One rank per process: under a launcher (RANK / WORLD_SIZE / LOCAL_RANK set) every process is one rank; this
tool does not spawn ranks.  ms_per_step is measured over the steps after the loop prepared its steady state, between
two device synchronisations.  --supervised: the same scenes with ground-truth label tables (`SyntheticLabelledDataset`)
through `VoxelizeCollate` (filter_out_classes=[0, 1], label_offset=2), num_targets=19, loss.device_max_targets=128."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=8, metavar="N")
    ap.add_argument("--voxels", type=int, default=150_000)
    ap.add_argument("--spread", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--steady-after", type=int, default=2)
    ap.add_argument("--settle", type=int, default=1, help="steps between the steady-state preparation and the timed ones")
    ap.add_argument("--force-dist", action="store_true", help="one rank: still run the gradient exchange (one-rank group)")
    ap.add_argument("--no-early-optimizer", action="store_true")
    ap.add_argument("--write-back-grad", action="store_true")
    ap.add_argument("--no-shuffle", action="store_true")
    ap.add_argument("--dist-backend", default="nccl")
    ap.add_argument("--resume", default=None, metavar="PATH")
    ap.add_argument("--supervised", action="store_true", help="ground-truth label tables through VoxelizeCollate")
    ap.add_argument("--train-precision", default="f32", choices=("f32", "bf16x2", "bf16x3"),
                    help="general.train_precision: the trunk's stride-1 convolutions in f32 or split bf16")
    ap.add_argument("--out", default=None, metavar="DIR", help="write DIR/last.ckpt at the end")
    a = ap.parse_args()

    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset, SyntheticLabelledDataset
    from unscene3d_amd.datasets.utils import VoxelizeCollate
    from unscene3d_amd.trainer import InstanceSegmentation, TrainLoop
    from unscene3d_amd.trainer.loop import pin_to_device_numa

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pin_to_device_numa(dev)
    if world > 1 or a.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(a.dist_backend, rank=rank, world_size=world,
                                **({"device_id": dev} if a.dist_backend == "nccl" else {}))

    overrides = ["general.num_targets=19", "loss.device_max_targets=128"] if a.supervised else ["general.num_targets=3"]
    cfg = apply_overrides(default_config(), overrides + [f"data.batch_size={world}", f"general.train_precision={a.train_precision}"])
    dataset = SyntheticLabelledDataset if a.supervised else SyntheticFreeMaskDataset
    torch.manual_seed(1234)
    module = InstanceSegmentation(cfg).to(dev).train()
    n = max(1, a.synthetic) * world
    scenes = []
    for j in range(n):
        scale = 1.0 if n == 1 else 1.0 + a.spread - 2 * a.spread * ((j * 5) % n) / max(1, n - 1)
        seed = 2000 if j == 0 else 2000 + 16 * j
        scenes.append(dataset(n_scenes=1, target_voxels=int(a.voxels * scale), seed=seed)[0])
    kw = dict(device=dev, world=world, rank=rank, force_dist=a.force_dist, early_optimizer=not a.no_early_optimizer,
              write_back_grad=a.write_back_grad, total_steps=100000, steady_after=a.steady_after, resident=True,
              shuffle=not a.no_shuffle, seed=2000)
    if a.supervised:
        kw["collate"] = VoxelizeCollate(ignore_label=255, voxel_size=cfg.data.voxel_size, mode="train",
                                        filter_out_classes=[0, 1], label_offset=2, device=str(dev))
    loop = TrainLoop.resume(a.resume, module, cfg, scenes, **kw) if a.resume else TrainLoop(module, cfg, scenes, **kw)
    with loop:
        first = loop.global_step
        head = min(a.steps, a.steady_after + a.settle)
        for _ in range(head):
            loop.step()
        torch.cuda.synchronize()
        timed = a.steps - head
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(timed + 1)] if timed > 0 else []
        t0 = time.perf_counter()
        if marks:
            marks[0].record()
        for k in range(timed):
            loop.step()
            marks[k + 1].record()              # device-side step boundaries, no host wait inside the timed loop
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(timed))
        rep = loop.losses()
        if a.out:
            loop.save_checkpoint(os.path.join(a.out, "last.ckpt"))
        from unscene3d_amd import _lib
        line = {"steps": loop.global_step - first, "skipped": loop.skipped, "timed_steps": timed,
                "ms_per_step": (1e3 * dt / timed) if timed > 0 else None,
                "ms_per_step_p10_p50_p90": ([round(float(np.percentile(per, q)), 3) for q in (10, 50, 90)] if per else None),
                "early_optimizer": loop.early, "supervised": bool(a.supervised), "world": world,
                "train_precision": a.train_precision,
                "force_dist": bool(a.force_dist),
                "buckets_started_during_backward": loop.reducer.started_during_backward if loop.reducer else None,
                "losses_step": rep["step"] if rep else None, "losses": rep["losses"] if rep else None,
                "library": _lib.lib.usc_build_info().decode()}
    if rank == 0:
        print(json.dumps(line))
    if world > 1 or a.force_dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
