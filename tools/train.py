"""Run the training loop (`unscene3d_amd.trainer.TrainLoop`) on synthetic scenes or on a dataset directory and print
one JSON line.

    python tools/train.py --synthetic 8 --voxels 150000 --steps 40 [--force-dist] [--no-early-optimizer]
                          [--resume PATH] [--out DIR] [--no-shuffle] [--supervised]
    python tools/train.py --data-dir DATA --steps 1000 --out RUN [--self-train-dir DIR] [--host-tables]

--data-dir DIR: the dataset tools/dataset_from_scans.py wrote.  The train scenes come from `FreeMaskSceneReader`
(mode="train", the shipped volume and colour augmentations, add_normals=False, add_raw_coordinates=True, the written
colour statistics) over train_database.yaml, mask tables built on the device; --host-tables builds them with numpy on
the host instead (same tables, same steps; for A/B).  validation_database.yaml + instance_gt/validation, when both
exist, switch the validation pass on (every cfg.trainer.check_val_every_n_epoch epochs).  --self-train-dir DIR merges
the previous round's export (tools/export_round.py: DIR/freemasks/scene*_cloud.npy and _masks.npy, or the bit rows
_masks_bits.npy, which are preferred when both exist) into every scene's masks.  The line then holds
`losses_per_step`, the weighted loss vector of every step taken.  --seed seeds numpy's, python's and torch's generators
(the reader's augmentations draw from the first two).

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
    ap.add_argument("--data-dir", default=None, metavar="DIR", help="train on a dataset of tools/dataset_from_scans.py")
    ap.add_argument("--self-train-dir", default=None, metavar="DIR", help="with --data-dir: load_self_train_data=True")
    ap.add_argument("--host-tables", action="store_true", help="with --data-dir: the reader's numpy mask tables")
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    if a.data_dir and (a.supervised or a.resume):
        ap.error("--data-dir goes with neither --supervised nor --resume")

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
    if a.data_dir:
        overrides.append("loss.device_max_targets=128")          # real scenes carry 20-50 pseudo masks
    cfg = apply_overrides(default_config(), overrides + [f"data.batch_size={world}", f"general.train_precision={a.train_precision}"])
    dataset = SyntheticLabelledDataset if a.supervised else SyntheticFreeMaskDataset
    torch.manual_seed(a.seed)
    module = InstanceSegmentation(cfg).to(dev).train()
    if a.data_dir:
        line = train_on_data_dir(a, cfg, module, dev, world, rank)
        if rank == 0:
            print(json.dumps(line, default=float))
        if world > 1 or a.force_dist:
            torch.distributed.destroy_process_group()
        return
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


def train_on_data_dir(a, cfg, module, dev, world, rank):
    """--data-dir: readers over the written databases -> TrainLoop, `a.steps` batches, epoch ends (validation,
    checkpoints) as `TrainLoop.run` handles them.  -> the JSON line."""
    import random

    from unscene3d_amd.datasets.augment import ColorAugmentations, VolumeAugmentations
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader, entries_from_database, load_color_mean_std
    from unscene3d_amd.evaluation.instance_ap import load_gt_ids
    from unscene3d_amd.trainer import TrainLoop

    d = a.data_dir
    stats = load_color_mean_std(os.path.join(d, "color_mean_std.yaml"))
    common = dict(color_mean_std=stats, add_normals=False, add_raw_coordinates=True, device=str(dev),
                  device_tables=not a.host_tables, load_self_train_data=bool(a.self_train_dir),
                  self_train_data_dir=a.self_train_dir)
    entries = entries_from_database(os.path.join(d, "train_database.yaml"))
    train = FreeMaskSceneReader(entries, mode="train", volume_augmentations=VolumeAugmentations(),
                                image_augmentations=ColorAugmentations(), **common)
    val = val_ids = None
    val_db, gt_dir = os.path.join(d, "validation_database.yaml"), os.path.join(d, "instance_gt", "validation")
    if os.path.exists(val_db) and os.path.isdir(gt_dir):
        val = FreeMaskSceneReader(entries_from_database(val_db), mode="validation",
                                  resegment_mesh=bool(getattr(cfg.data, "resegment_mesh", False)),
                                  segment_min_vert_num=getattr(cfg.data, "segment_min_vert_num", 20), **common)
        names = [val._scene_name(i) for i in range(len(val))]
        val_ids = {n: load_gt_ids(os.path.join(gt_dir, f"{n}.txt")) for n in names}
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    np.random.seed(a.seed)
    random.seed(a.seed)
    loop = TrainLoop(module, cfg, train, device=dev, world=world, rank=rank, force_dist=a.force_dist,
                     early_optimizer=not a.no_early_optimizer, write_back_grad=a.write_back_grad, total_steps=100000,
                     steady_after=a.steady_after, shuffle=not a.no_shuffle, seed=2000,
                     sizes=[int(e.get("file_len", 1)) for e in entries], val_scenes=val, val_gt_ids=val_ids,
                     out_dir=a.out)
    per_step, metrics = [], {}
    with loop:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            before = loop.epoch
            if loop.step() is not None:
                per_step.append(loop.last_losses.clone())          # device tensors: read after the last step
            if loop.epoch != before:
                metrics = loop.end_epoch() or metrics
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if a.out:
            loop.save_checkpoint(os.path.join(a.out, "last.ckpt"))
        from unscene3d_amd import _lib
        return {"steps": loop.global_step, "skipped": loop.skipped, "epoch": loop.epoch, "scenes": len(train),
                "validation_scenes": len(val) if val is not None else 0, "metrics": metrics,
                "device_tables": not a.host_tables, "ms_per_step_wall": 1e3 * dt / max(1, a.steps),
                "loss_names": list(loop._loss_keys or []), "losses_per_step": [v.tolist() for v in per_step],
                "library": _lib.lib.usc_build_info().decode()}


if __name__ == "__main__":
    main()
