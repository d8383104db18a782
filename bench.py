#!/usr/bin/env python
"""bench.py — training scenes/sec of UnScene3D's self-training hot path on MI355X.

`python bench.py --gpus N --steps K --warmup W`.  N>1 needs one process per GPU over RCCL: either the caller
launches the ranks (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`; RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment) or, when WORLD_SIZE is not set, this script
re-executes itself through torch.distributed.run with N ranks on 127.0.0.1.  In both cases the world size must
equal --gpus (checked), the backend is nccl (= RCCL) and every rank owns one device.

One "step" (default --mode mask3d, BASELINE.json configs[2]) = one full self-training step over one synthetic
ScanNet-shaped 150k-voxel scene per GPU: device collate (2 cm voxelisation, hash unique, targets) -> coordinate /
kernel maps -> Res16UNet34C -> 3x4 decoder passes -> 13 cost matrices -> Hungarian (device: usc_lsap_batch, scipy's
algorithm and tie-breaking) -> 52 losses -> backward -> (N>1: gradient all-reduce) -> AdamW + OneCycleLR.  The raw scene arrays are resident in HBM before the
timed region.  Rank 0 prints ONE JSON line (DESIGN.md §5 defines `roofline` and `cpu_baseline`).

A plain run sets up, warms up, times the K steps and prints the line; `ms_per_step` is the wall time of one timed step.
`--full` adds what the headline figure does not need (CPU baseline, the second row order, the roofline); `--dump-outputs
DIR` writes what the last timed step computed as .npy files, so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

VOXELS = 150_000
MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
HBM_PEAK_GBS = 8000.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voxels", type=int, default=VOXELS)
    ap.add_argument("--mode", choices=["mask3d", "backbone", "ncut"], default="mask3d",
                    help="mask3d: BASELINE.json configs[2] full self-train step (the metric's config); "
                         "backbone: configs[1] Res16UNet34C fwd+bwd only; "
                         "ncut: configs[4] masked-NCut pseudo-mask loop on a 625-segment scene (secondary metric)")
    ap.add_argument("--scenes", type=int, default=16,
                    help="--mode ncut: scenes in flight on one GPU (one HIP stream each, one host thread for all)")
    ap.add_argument("--no-graphs", action="store_true", help="do not capture the decoder passes as HIP graphs")
    ap.add_argument("--torch-adamw", action="store_true", help="torch.optim.AdamW(fused=True) instead of the flat-buffer kernel")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="voxelise and build the coordinate maps at the start of the step on the compute stream "
                         "instead of ahead of time on a side stream")
    ap.add_argument("--prefetch-depth", type=int, default=2, metavar="D",
                    help="batches the scene prefetcher keeps in flight (the reference's DataLoader: prefetch_factor = 2)")
    ap.add_argument("--prefetch-ahead", type=int, default=0, metavar="N",
                    help="DIAGNOSTIC (not the metric: the collate leaves the timed region): prepare N batches before the "
                         "timed loop and consume them without issuing new ones — the step without the prefetch stream's "
                         "kernels running beside it")
    ap.add_argument("--spatial-sort", type=int, default=0, metavar="SHIFT",
                    help="row order of `value`.  0 (default) = the reference's first-occurrence order "
                         "(ME.utils.sparse_quantize, datasets/utils.py:403-408): FPS and key sampling pick the rows the "
                         "reference would pick.  SHIFT > 0: voxel rows grouped into z-ordered cells of (2^SHIFT)^3 voxels by "
                         "the collate (a consistent row permutation; sparse_quantize itself stays bit-exact)")
    ap.add_argument("--zorder-shift", type=int, default=5, metavar="SHIFT",
                    help="the second timed loop (`value_zorder`) runs the same steps with the rows in z-ordered cells of "
                         "(2^SHIFT)^3 voxels: 5 = 64 cm cells, 2.3x instead of 6.9x the algorithmic bytes fetched by the "
                         "dominant conv kernel at the same step time (profiles/r02_spatial_sort_sweep.txt)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-reference-order", "--no-zorder", dest="no_second_order", action="store_true",
                    help="skip the second timed loop in the other row order (`value_zorder`)")
    ap.add_argument("--dist-backend", default="nccl",
                    help="nccl (= RCCL, the measured configuration); gloo only to smoke-test the N>1 code path on a box "
                         "with fewer GPUs than ranks (ranks then share devices)")
    ap.add_argument("--scenes-per-gpu", type=int, default=1, metavar="B",
                    help="scenes per rank and step (the reference trains with batch_size 5-8 per GPU, conf/data/indoor.yaml:25; "
                         "the headline metric is quoted at 1): B distinct synthetic scenes collated into one sparse batch, "
                         "decoder passes captured for batch B")
    ap.add_argument("--rotate", type=int, default=8, metavar="N",
                    help="rotate N distinct scene sets through the steps (per-step times p10/p50/p90 are added to the "
                         "line); 0 or 1 = replay one scene")
    ap.add_argument("--rotate-spread", type=float, default=0.02, metavar="F",
                    help="voxel counts of the rotated scenes spread over +-F of --voxels: 0.02 = SURVEY.md 8(d)'s "
                         "tolerance for a `150 k-voxel` scene (the metric's scene size); 0.2 = ScanNet-like size spread "
                         "(what the N-rank sampler / skew report is exercised with)")
    ap.add_argument("--bucket-window", type=int, default=8, metavar="K",
                    help="with --rotate on N > 1 ranks the scenes are drawn through datasets/sampler.py "
                         "(DistributedSampler semantics): K steps' worth of scenes are sorted by size and dealt so that "
                         "the ranks of a step hold scenes of similar size; 1 = plain DistributedSampler order")
    ap.add_argument("--voxels-by-rank", default=None, metavar="N0,N1,...",
                    help="scene size per rank (uneven ranks: the step of a small scene is host-bound, that of a large one "
                         "device-bound; the collectives must line up all the same); default: --voxels on every rank")
    ap.add_argument("--eager-ranks", default="", metavar="R0,R1,...",
                    help="ranks that do NOT capture the decoder passes as HIP graphs (mixed eager / graphed ranks)")
    ap.add_argument("--force-dist", action="store_true",
                    help="with --gpus 1: still create a (one-rank) process group and run the bucketed gradient reducer and "
                         "the criterion's all-reduce through it — what RCCL's own streams cost next to the step's four")
    ap.add_argument("--dry-collectives", action="store_true",
                    help="N ranks: run ONLY the collectives of a training step — the criterion's 13 scalar `num_masks` "
                         "all-reduces (models/criterion.py:258-260) and the gradient exchange in the reducer's bucket "
                         "schedule, next to one flat all-reduce — timed per bucket, without building a scene: what the "
                         "exchange costs when nothing hides it, to be read beside `ms_per_step` on an N-GPU node")
    ap.add_argument("--cpu-sample-voxels", type=int, default=10_000,
                    help="scene size of the cpu_baseline legs (3 warm-up + up to 10 timed passes of the CPU restatement each)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the CPU baseline, the second timed loop in "
                         "the other row order (`value_zorder`), the dominant kernel's roofline (in-step launch marks + one "
                         "instrumented step) and, with --mode ncut, the eigen-solve timing and its CPU baseline.  Without "
                         "it the line holds `roofline: null` and `cpu_baseline: null`")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32): "
                         "mask3d / backbone: the total loss, every weighted loss, and a fixed seeded sample of the updated "
                         "parameters and of their gradients; ncut: the masks of every scene of the last round")
    return ap.parse_args(argv)


DUMP_SAMPLE = 1 << 20     # --dump-outputs: parameters / gradients sampled (4 MB each in float32)


def dump_outputs(dirname, arrays):
    """arrays: {name: tensor or array} -> DIR/<name>.npy, float32 (float64 kept)."""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.dtype != np.float64:
            a = a.astype(np.float32)
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def step_outputs(loss, losses, params):
    """What a caller of the training step holds after the last timed step: the total loss, the weighted losses by name,
    and the parameters after the optimizer step with the gradients that moved them — the last two as the same fixed,
    seeded sample of DUMP_SAMPLE positions in the concatenated parameter vector (all of it when it is smaller)."""
    out = {"loss": loss.reshape(())}
    out.update({k: v.reshape(()) for k, v in (losses or {}).items()})
    with torch.no_grad():
        p = torch.cat([q.detach().reshape(-1) for q in params])
        g = torch.cat([q.grad.detach().reshape(-1) for q in params])
        n = p.numel()
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(n, min(n, DUMP_SAMPLE), replace=False))).to(p.device)
        out["params_sample"] = p[idx]
        out["grads_sample"] = g[idx]
    return out


def build_model(device):
    from unscene3d_amd.models.res16unet import Res16UNet34C

    torch.manual_seed(1234)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    return Res16UNet34C(3, 20, cfg, out_fpn=True).to(device).train()


def train_step(model, opt, xyz, colors, flat, world):
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import ops

    # V1: voxelise on the device (reference: ME.utils.sparse_quantize in the collate, datasets/utils.py:403-408)
    c3, umap, _ = ME.utils.sparse_quantize(xyz, quantization_size=0.02, return_index=True, return_inverse=True,
                                           device=str(xyz.device))
    coords = torch.cat([torch.zeros((c3.shape[0], 1), dtype=torch.int32, device=xyz.device), c3], 1).contiguous()
    # (z-order row sorting — ops.spatial_order — was measured to make the gather convs ~12 % slower:
    #  scan-order rows spread the gathers over all HBM channels; kept off)
    feats = ops.gather_rows(colors, umap)
    x = ME.SparseTensor(features=feats, coordinates=coords, device=xyz.device)   # V3
    out, fmaps = model(x)
    loss = out.F.square().mean()
    for f in fmaps[:-1]:
        loss = loss + f.F.square().mean()
    opt.zero_grad(set_to_none=False)
    loss.backward()
    if world > 1:
        dist.all_reduce(flat)          # RCCL over xGMI: one flat 151 MB buffer
        flat.div_(world)
    opt.step()
    return loss, coords.shape[0]


WORKLOADS = {
    "backbone": "BASELINE.json configs[1]: Res16UNet34C backbone fwd+bwd+AdamW, one synthetic ScanNet-shaped scene "
                "per GPU, {nvox} voxels @2cm (voxelise + coordinate/kernel maps rebuilt every step), random-init weights",
    "mask3d": "BASELINE.json configs[2]: full Mask3D self-train step (device collate/voxelise -> Res16UNet34C -> "
              "100-query decoder 3x4 passes -> Hungarian (on the device) -> 52 losses -> backward -> AdamW + OneCycleLR), "
              "{spr} synthetic ScanNet-shaped scene(s) per GPU and step, {nvox} voxels @2cm each, pseudo-mask targets, "
              "random-init weights",
}


def _gil_switch_interval():
    """Two Python threads issue device work here: the step (main thread) and the next scenes' voxelisation + maps (the
    prefetcher's worker).  CPython hands the interpreter lock over every 5 ms by default — a fifth of the step: the main
    thread, whose launches the device is waiting for, then sits out whole slices of the worker's bookkeeping.
    USC3D_GIL_SWITCH_MS (default 0.5) shortens the slice."""
    import sys
    ms = float(os.environ.get("USC3D_GIL_SWITCH_MS", "0.5"))
    if ms > 0:
        sys.setswitchinterval(ms / 1e3)


def make_mask3d_step(args, dev, rank, world):
    """Full self-training step (reference trainer/trainer.py:99-163 + :953-966) on one scene per rank."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.ddp import flatten_grads
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    B = max(1, args.scenes_per_gpu)
    cfg = apply_overrides(default_config(), ["general.num_targets=3", f"data.batch_size={world * B}"])
    torch.manual_seed(1234)
    module = InstanceSegmentation(cfg).to(dev).train()
    params = [p for n, p in module.named_parameters() if ".backbone.final." not in n]    # unused in forward
    flat = flatten_grads(params)
    if args.torch_adamw:
        opt = torch.optim.AdamW(params, lr=cfg.optimizer.lr, fused=True)
    else:
        from unscene3d_amd.optim import FlatAdamW
        opt = FlatAdamW(params, lr=cfg.optimizer.lr, flat_grad=flat)     # same defaults as torch.optim.AdamW
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=cfg.optimizer.lr, total_steps=100000)
    voxels = args.voxels
    if args.voxels_by_rank:
        by_rank = [int(v) for v in args.voxels_by_rank.split(",")]
        voxels = by_rank[rank % len(by_rank)]
    eager = str(rank) in [r for r in args.eager_ranks.split(",") if r]
    def resident(sample):
        # raw scene arrays resident in HBM before the timed region (the collate reads them from there)
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) if isinstance(x, np.ndarray) and i in (0, 1, 2)
                     else x for i, x in enumerate(sample))
    # scene sets: one per rotation slot, B scenes each; slot 0 of B = 1 is the scene of rounds 1-2 (seed 2000 + rank)
    n_sets = max(1, args.rotate)
    sets, skew_info = [], None
    if world > 1 and args.rotate:
        # N ranks: ONE pool of world * rotate * B scenes (sizes spread over +-20 %), every rank draws its scenes of a
        # step through the sampler (DistributedSampler semantics + size bucketing, datasets/sampler.py) and keeps only
        # the scenes of its own plan resident
        from unscene3d_amd.datasets.sampler import BucketedDistributedSampler
        n_pool = world * n_sets * B
        sp = float(args.rotate_spread)
        scale = 1.0 - sp + 2 * sp * ((np.arange(n_pool) * 5) % n_pool) / max(1, n_pool - 1)
        sizes = (voxels * scale).astype(np.int64)
        sampler = BucketedDistributedSampler(sizes, world, rank, batch_size=B, window=max(1, args.bucket_window), seed=2000)
        plain = BucketedDistributedSampler(sizes, world, rank, batch_size=B, window=1, seed=2000)
        mine = sampler.plan()[:, rank, :]
        n_sets = mine.shape[0]
        cache = {}
        for step_ids in mine:
            for g in step_ids:
                if int(g) not in cache:
                    ds = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=int(sizes[g]), seed=5000 + 16 * int(g))
                    cache[int(g)] = resident(ds[0])
            sets.append([cache[int(g)] for g in step_ids])
        skew_info = {"sampler": "BucketedDistributedSampler", "bucket_window": sampler.window, "pool_scenes": n_pool,
                     "planned_voxel_max_over_mean": sampler.imbalance(), "unbucketed_voxel_max_over_mean": plain.imbalance()}
    else:
        for j in range(n_sets):
            sp = float(args.rotate_spread)
            # spread, not sorted — except that set 0 is the LARGEST scene: the warm-up steps then size the caching
            # allocator's blocks for everything that follows (a larger scene met for the first time inside the timed
            # loop costs a round of hipMalloc calls: one 52 ms step in ten)
            scale = 1.0 if n_sets == 1 else 1.0 + sp - 2 * sp * ((j * 5) % n_sets) / max(1, n_sets - 1)
            seed = 2000 + rank if (B == 1 and j == 0) else 2000 + 1000 * rank + 16 * j
            ds = SyntheticFreeMaskDataset(n_scenes=B, target_voxels=int(voxels * scale), seed=seed)
            sets.append([resident(ds[i]) for i in range(B)])
    if not (args.no_graphs or eager):
        module.model.enable_decoder_graphs(batch_size=B, device=dev)
    collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="train", device=str(dev),
                                      spatial_sort=args.spatial_sort)

    reducer = None
    if (world > 1 or getattr(args, "force_dist", False)) and os.environ.get("USC3D_OVERLAP_ALLREDUCE", "1") == "1":
        from unscene3d_amd.ddp import BucketedGradReducer
        reducer = BucketedGradReducer(params, flat, world).install()     # ~24 MB buckets, started during backward

    # optimizer in the backward pass (one rank, FlatAdamW): the trunk's parameters are stepped stage by stage, as their
    # gradients become final, on the stream that is idle during the backbone's backward pass (optim.FlatAdamW.enable_early)
    early_opt = None
    if (world == 1 and not getattr(args, "force_dist", False) and not args.torch_adamw
            and os.environ.get("USC3D_EARLY_OPTIMIZER", "1") == "1"):
        from unscene3d_amd.models import mask3d as _m3d
        if getattr(_m3d, "_KV_SIDE_STREAM", False):
            early_opt = module.model._side_stream(dev)
            opt.enable_early(early_opt)

    prefetch = None
    if not args.no_prefetch:
        from unscene3d_amd.datasets.prefetch import ScenePrefetcher
        prefetch = ScenePrefetcher(collate, add_raw_coordinates=cfg.data.add_raw_coordinates, device=dev,
                                   precompute=module.model.precompute_geometry,
                                   threaded=os.environ.get("USC3D_PREFETCH_THREAD", "1") == "1",
                                   bounded_lifetime=(int(os.environ.get("USC3D_STEPS_IN_FLIGHT", "2")) > 0
                                                     and os.environ.get("USC3D_BOUNDED_BATCHES", "1") == "1"))
        # the first batches, outside the timed region like the resident raw arrays.  Two in flight (the reference's
        # DataLoader default, prefetch_factor = 2): with one, every step began by waiting ~8 ms for the worker thread to
        # finish issuing the batch submitted a moment earlier — host time the 24 ms device step no longer hides
        depth = max(1, getattr(args, "prefetch_depth", 2))
        for j in range(depth):
            prefetch.submit(sets[j % n_sets])
    _gil_switch_interval()
    state = {"k": 0, "marks": None}
    ahead = []
    if prefetch is not None and getattr(args, "prefetch_ahead", 0) > 0:
        from unscene3d_amd.datasets.prefetch import _record_streams
        prefetch.drain()
        ahead = [prefetch._issue(sets[k % n_sets]) for k in range(args.prefetch_ahead)]
        torch.cuda.synchronize()

    from unscene3d_amd.trainer.trainer import StepsInFlight
    in_flight = StepsInFlight(int(os.environ.get("USC3D_STEPS_IN_FLIGHT", "2")))

    def step(w):
        state["k"] += 1
        in_flight.begin()              # at most two steps queued on the device (trainer.StepsInFlight)
        if ahead:
            batch, done, _ = ahead.pop(0)
            torch.cuda.current_stream().wait_event(done)
            _record_streams(batch, torch.cuda.current_stream(), set())
        elif prefetch is not None:
            batch = prefetch.take()
        else:
            batch = collate(sets[(state["k"] - 1) % n_sets])
        out = module.training_step(batch)
        if out is None:      # the trainer skips a batch without targets, like the reference (trainer/trainer.py:106-108)
            raise SystemExit("bench.py: training_step skipped the batch (no targets in the synthetic scene): "
                             "--voxels is too small for this benchmark")
        total, losses = out
        if args.dump_outputs:          # kept for --dump-outputs only (detached: no graph node outlives its step)
            state["losses"] = {k: v.detach() for k, v in losses.items()}
        opt.zero_grad(set_to_none=False)
        if reducer is not None:
            reducer.begin_step()
        total.backward()
        if state["marks"] is not None:                # device-side: this rank's own work of the step is queued up to here
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            state["marks"].append(ev)
        if reducer is not None:
            reducer.finish()           # RCCL over xGMI: what backward has not already started, then wait + average
        elif w > 1 or getattr(args, "force_dist", False):
            dist.all_reduce(flat)      # one flat ~158 MB gradient buffer (--force-dist: over the one-rank group too)
            flat.div_(w)
            nd = int(os.environ.get("USC3D_DUMMY_COLLECTIVES", "0"))      # diagnostic: does the NUMBER of collectives per step matter?
            if nd:
                if os.environ.get("USC3D_DUMMY_SYNC"):
                    for k in range(nd):
                        dist.all_reduce(flat[k * 1024:(k + 1) * 1024])
                else:
                    hs = [dist.all_reduce(flat[k * 1024:(k + 1) * 1024], async_op=True) for k in range(nd)]
                    for h in hs:
                        h.wait()
        opt.step()
        state["sched"].step()
        step_done = in_flight.end()
        if prefetch is not None and prefetch.bounded:
            prefetch.retire(step_done)     # the batch of this step may be released once the device is past this point
        if prefetch is not None and not ahead and not getattr(args, "prefetch_ahead", 0):
            # the voxelisation + coordinate maps of the step after the next (depth 2), on the prefetch stream
            prefetch.submit(sets[(state["k"] + max(1, getattr(args, "prefetch_depth", 2)) - 1) % n_sets])
        return total.detach(), batch[0].coordinates.shape[0]

    state["sched"] = sched
    def set_spatial_sort(shift):
        """Switch the collate's row order (0 = the reference's first-occurrence order, datasets/utils.py:403-408) and
        re-issue the prefetched batch in the new order."""
        collate.spatial_sort = int(shift) if shift else False
        if prefetch is not None:
            prefetch.drain()
            for j in range(max(1, getattr(args, "prefetch_depth", 2))):
                prefetch.submit(sets[(state["k"] + j) % n_sets])

    step.set_spatial_sort = set_spatial_sort
    def close():
        if early_opt is not None:
            opt.disable_early()            # (a module-level hook: the next step object of this process must not feed this optimizer)
        if prefetch is not None:
            prefetch.close()
    step.close = close
    step.prefetch = prefetch
    step.scenes_per_rank = B
    step.skew_info = skew_info
    step.state = state
    step.reducer = reducer
    step.module = module
    step.params = params
    step.opt = opt
    step.set_sched = lambda s: state.__setitem__("sched", s)      # tools/det_probe_mr.py restarts the schedule per trial
    return step


def _committed_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (profiles/pmc_traffic.json), or null
    with the reason when the figure cannot vouch for the code that just ran: the json records the sha256 of every
    kernel source at measurement time; a kernel whose defining .hip (or a shared header) changed since reports null."""
    import hashlib
    import re
    root = os.path.dirname(os.path.abspath(__file__))
    tpath = os.path.join(root, "profiles", "pmc_traffic.json")
    if not os.path.exists(tpath):
        return {"traffic": None, "traffic_source": "no profiles/pmc_traffic.json"}
    with open(tpath) as f:
        table = json.load(f)
    ent = table.get(kernel)
    if not ent:
        return {"traffic": None, "traffic_source": f"profiles/pmc_traffic.json has no entry for {kernel}"}
    shas = table.get("_source_sha256")
    if not shas:
        return {"traffic": None, "traffic_source": "profiles/pmc_traffic.json carries no source hashes (unverifiable)"}
    csrc = os.path.join(root, "unscene3d_amd", "csrc")
    base = re.sub(r"<.*$", "", kernel.replace("usc::", ""))
    need = [f for f in sorted(os.listdir(csrc)) if f.endswith(".h")]
    need += [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip")
             and re.search(r"\b" + re.escape(base) + r"\b", open(os.path.join(csrc, f)).read())]
    for fn in need:
        have = hashlib.sha256(open(os.path.join(csrc, fn), "rb").read()).hexdigest()
        if shas.get(fn) != have:
            return {"traffic": None, "traffic_source": f"stale: {fn} changed since profiles/pmc_traffic.json was measured"}
    return {"traffic": ent["bytes_per_launch"], "traffic_source": "profiles/pmc_traffic.json (source hashes match)"}


def _stream_report():
    """What unscene3d_amd/streams.py measured when it picked the prefetch / lane / key-preparation streams (two HIP streams
    may share a hardware queue; `shared_queue: true` = no candidate overlapped with the compute stream)."""
    try:
        from unscene3d_amd import streams
        return [{"role": r["role"], "shared_queue": r["shared_queue"], "tried": len(r["tried"]),
                 "ratios": r["tried"][-1]["ratios"] if r["tried"] else None,
                 **({"switched_off": r["switched_off"]} if "switched_off" in r else {})} for r in streams.REPORT]
    except Exception as err:      # noqa: BLE001 — a report, never a reason to lose the bench line
        return str(err)


def _allreduce_note(step, world):
    red = getattr(step, "reducer", None)
    if world == 1 and red is None:
        import torch.distributed as dist
        return "one flat buffer after backward (one-rank group)" if dist.is_available() and dist.is_initialized() else None
    if red is None:
        return "one flat buffer after backward"
    return (f"{len(red.bounds)} buckets of the flat buffer, {red.started_during_backward} started during backward "
            f"(last step)")


def _pin_to_device_numa(dev):
    """Bind this process to the CPUs of the NUMA node the device hangs off (sysfs: /sys/bus/pci/devices/<bdf>/local_cpulist) —
    what a launcher does for a rank on a two-socket box; every launch is a doorbell write across the fabric otherwise, and
    the scheduler is free to move the two Python threads between sockets.  Measured on one box, alternating, K = 20:
    22.78 / 22.50 / 22.49 ms pinned to the local node, 22.70 / 22.80 / 22.75 to the remote one, 22.67 / 22.80 / 22.82
    unpinned.  USC3D_NUMA_PIN=0 leaves the affinity alone.  -> the CPU list it bound to, or None."""
    if os.environ.get("USC3D_NUMA_PIN", "1") != "1" or not hasattr(os, "sched_setaffinity"):
        return None
    try:
        p = torch.cuda.get_device_properties(dev)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
            text = f.read().strip()
        cpus = set()
        for part in text.split(","):
            if part:
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        before = os.sched_getaffinity(0)
        cpus &= before
        if len(cpus) >= 8 and cpus != before:
            _set_affinity_all_threads(cpus)
            _pin_to_device_numa.before = before        # (the CPU baseline runs on the host's cores as it always did)
            return text
    except (OSError, ValueError, AttributeError):
        pass
    return None


def _set_affinity_all_threads(cpus):
    """sched_setaffinity works per THREAD: apply the mask to every thread the process has (the runtime's, the OpenMP pool's)."""
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cpus)
        except OSError:
            pass


def _unpinned(fn, *a):
    """fn(*a) with the process's original CPU affinity (the oracle's legs use up to half of the host's threads)."""
    before = getattr(_pin_to_device_numa, "before", None)
    if before is not None:
        _set_affinity_all_threads(before)
    return fn(*a)


def _device_id(dev):
    """A string that names the physical device behind `dev`: its uuid when the runtime reports one, else the PCI bus
    id, else the index (two ranks that print the same string share a device)."""
    prop = torch.cuda.get_device_properties(dev)
    for attr in ("uuid", "pci_bus_id"):
        v = getattr(prop, attr, None)
        if v not in (None, ""):
            extra = "".join(f":{getattr(prop, a)}" for a in ("pci_domain_id", "pci_device_id") if hasattr(prop, a)) \
                if attr == "pci_bus_id" else ""
            return f"{attr}={v}{extra}"
    return f"index={dev.index}"


def _ranks_seen(dev, rank, world, backend, params):
    """What the collectives really spanned (reference: pl.Trainer(gpus=N), main_instance_segmentation.py:86-92):
    `rccl_ranks_seen` = dist.get_world_size() when the backend is nccl (= RCCL) else 0, the physical device of every
    rank (all-gathered), and whether every rank holds the same weights after the run (data-parallel ranks that apply
    the same averaged gradients must agree to the bit)."""
    import socket
    ids = [None] * world
    dist.all_gather_object(ids, f"{socket.gethostname()}/{_device_id(dev)}")
    same = None
    if params:
        with torch.no_grad():
            tot = torch.zeros(world, dtype=torch.float64, device=dev)
            tot[rank] = sum(p.detach().double().abs().sum() for p in params)     # one checksum per rank
            dist.all_reduce(tot)
            same = bool((tot == tot[0]).all().item())
    return {"dist_backend": backend, "rccl_ranks_seen": dist.get_world_size() if backend == "nccl" else 0,
            "rank_devices": ids, "distinct_devices": len(set(ids)), "weights_equal_across_ranks": same}


def cpu_baseline(sample_voxels, mode="mask3d"):
    """Oracle (CPU restatement of the same fwd+bwd) on a bounded sample, rank 0 only."""
    if mode == "mask3d":
        return cpu_baseline_mask3d(sample_voxels)
    import oracle.res16unet_ref as M
    from oracle import sparse_ref as R
    from unscene3d_amd.synthetic import make_scene

    sc = make_scene(2999, target_voxels=sample_voxels, tol=0.05)
    t0 = time.perf_counter()
    ec = R.voxel_floor(sc["xyz"], 0.02)
    eu, _ = R.sparse_quantize(ec)
    coords4, feats = R.sparse_collate([ec[eu]], [sc["colors"][eu]])
    feats = torch.from_numpy(feats)
    from unscene3d_amd.models.res16unet import Res16UNet34C
    torch.manual_seed(1234)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point)
          for k, v in Res16UNet34C(3, 20, cfg, out_fpn=True).state_dict().items()}
    pyr = M.Pyramid(coords4)
    out, levels = M.res16unet_forward(sd, pyr, feats, (2, 3, 4, 6, 2, 2, 2, 2))
    loss = out.square().mean()
    for f in levels[:-1]:
        loss = loss + f.square().mean()
    loss.backward()
    dt = time.perf_counter() - t0
    nv = coords4.shape[0]
    return {
        "value": (nv / VOXELS) / dt, "unit": "scenes/s (150k-voxel-scene equivalents)",
        "cores": torch.get_num_threads(), "kind": "port",
        "sample": f"oracle Res16UNet34C fwd+bwd (voxelise+maps+conv/BN autograd, no optimizer) on one "
                  f"{nv}-voxel synthetic scene, {dt:.1f} s, scaled by voxels/150000",
    }


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_mask3d(sample_voxels, runs=10, warmup=3, leg_budget_s=25.0, full_size_voxels=VOXELS):
    """oracle/mask3d_ref.py forward + criterion + backward (through every parameter, backbone included) on one small
    scene (SURVEY.md §8d "Timing the reference CPU path": ME cannot run, so the baseline is the CPU restatement):
    `warmup` untimed + up to `runs` timed passes per leg — 3 threads (the reference's scripts export
    OMP_NUM_THREADS=3, scripts/unsupervised/train_unscene3d.sh:2) and all host threads; a leg stops early (never below
    3 timed passes) once it has used `leg_budget_s` seconds, so that the default bench run stays within minutes on a
    128-thread host where the restatement's many small torch ops are oversubscribed.  median / p10 / p90 / min / max;
    value scaled by voxels/150000."""
    import oracle.criterion_ref as OC
    import oracle.mask3d_ref as OM
    from oracle import sparse_ref as R
    from unscene3d_amd.config import apply_overrides, default_config, instantiate_model
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset

    cfg = apply_overrides(default_config(), ["general.num_targets=3"])
    sample = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=sample_voxels, seed=2999)[0]
    torch.manual_seed(1234)
    sd0 = {k: v.detach().clone() for k, v in instantiate_model(cfg).state_dict().items()}
    m = cfg.matcher
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0, "loss_noise_robust": 0.0}
    wd.update({f"{k}_{i}": v for i in range(12) for k, v in list(wd.items())})

    def one_pass():
        nonlocal sample
        sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd0.items()}
        t0 = time.perf_counter()
        ec = R.voxel_floor(sample[0], 0.02)
        eu, _ = R.sparse_quantize(ec)
        coords4, feats = R.sparse_collate([ec[eu]], [sample[1][eu]])
        table = torch.from_numpy(sample[2][eu].astype(np.int64))
        _, p2s = np.unique(table[:, -1].numpy(), return_inverse=True)
        p2s = torch.from_numpy(p2s.reshape(-1))
        S = int(p2s.max()) + 1
        masks = table[:, 1:-1].bool().T
        masks = masks[masks.sum(1) > 0]
        seg_mask = torch.zeros(masks.shape[0], S, dtype=torch.bool)
        for t in range(masks.shape[0]):
            seg_mask[t, p2s[masks[t]].unique()] = True
        target = [{"labels": torch.ones(masks.shape[0], dtype=torch.int64), "masks": masks, "segment_mask": seg_mask,
                   "point2segment": p2s}]
        feats = torch.from_numpy(feats)
        out = OM.mask3d_forward(sd, cfg, coords4, feats[:, :3], feats[:, 3:], [p2s], lambda n: torch.randperm(n),
                                keep_graph=True)     # gradients reach every parameter, backbone included
        losses = OC.set_criterion(out, target, "segment_mask", num_classes=3, eos_coef=0.1, cost_class=m.cost_class,
                                  cost_mask=m.cost_mask, cost_dice=m.cost_dice)
        sum(v * wd[k] for k, v in losses.items() if k in wd).backward()
        return time.perf_counter() - t0, coords4.shape[0]

    all_threads = torch.get_num_threads()
    legs = {}
    for name, nthr in (("omp3", 3), ("all_threads", all_threads)):
        torch.set_num_threads(nthr)
        leg_t0 = time.perf_counter()
        for _ in range(warmup):                      # allocator, thread pool, lazy imports
            one_pass()
            if time.perf_counter() - leg_t0 > leg_budget_s / 2:      # slow leg (oversubscribed host): one warm-up pass
                break
        ts = []
        # at least three timed passes — unless the leg is pathological: a pass that alone overruns twice the leg's budget
        # ends the leg (round 6: with the process bound to one NUMA node the 128-thread leg took 571 s PER PASS and the
        # default line 40 minutes; the binding is lifted for this function now, and no leg can do that again)
        while len(ts) < runs and (len(ts) < 3 or time.perf_counter() - leg_t0 < leg_budget_s):
            dt, nv = one_pass()
            ts.append(dt)
            if time.perf_counter() - leg_t0 > 2 * leg_budget_s and len(ts) >= 1 and dt > leg_budget_s / 2:
                break
        ts.sort()
        q = lambda f: ts[min(len(ts) - 1, int(round(f * (len(ts) - 1))))]
        legs[name] = {"threads": nthr, "timed_passes": len(ts), "median_s": q(0.5), "p10_s": q(0.1), "p90_s": q(0.9),
                      "min_s": ts[0], "max_s": ts[-1], "scenes_per_s_150k_equiv": (nv / VOXELS) / q(0.5)}
    # one UNSCALED pass at the metric's own size (round-3 verdict, weak #15: the legs above time a 10 k-voxel scene and
    # scale by the voxel ratio): a full 150 k-voxel scene with 16 threads — the thread count at which the restatement's
    # index kernels stop scaling on the hosts seen so far
    full = None
    if full_size_voxels:
        nthr = min(16, all_threads)
        torch.set_num_threads(nthr)
        small = sample
        sample = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=full_size_voxels, seed=2000)[0]
        dt, nv_full = one_pass()
        sample = small
        full = {"threads": nthr, "voxels": int(nv_full), "seconds": dt, "scenes_per_s": 1.0 / dt,
                "scenes_per_s_150k_equiv": (nv_full / VOXELS) / dt}
    torch.set_num_threads(all_threads)
    best = max(legs.values(), key=lambda l: l["scenes_per_s_150k_equiv"])
    a, o = legs["all_threads"], legs["omp3"]
    value, cores, unit = best["scenes_per_s_150k_equiv"], best["threads"], \
        "scenes/s in 150k-voxel-scene equivalents (measured on a smaller scene, scaled by voxels/150000)"
    if full is not None and full["scenes_per_s_150k_equiv"] >= value:
        value, cores, unit = full["scenes_per_s_150k_equiv"], full["threads"], \
            "scenes/s (one unscaled pass over a full-size scene; scaled by voxels/150000 only for the +-2 % size tolerance)"
    return {
        # the fastest leg is the baseline (oversubscribed hosts run the restatement's many small torch ops far slower
        # with all hardware threads than with a few); every leg is reported
        "value": value, "unit": unit,
        "cores": cores, "kind": "port", "cpu_model": _cpu_model(), "host_cpus": os.cpu_count(),
        "runs": best["timed_passes"], "legs": legs, "full_size_pass": full,
        "sample": f"oracle Mask3D self-train step (voxelise + maps + Res16UNet34C + decoder + Hungarian + losses, forward "
                  f"+ backward through all parameters, no optimizer; CPU restatement, not the reference binary: "
                  f"MinkowskiEngine cannot run here) on one {nv}-voxel synthetic scene; {warmup} warm-up + up to {runs} "
                  f"timed passes per leg (a leg stops after {leg_budget_s:.0f} s, >= 3 passes); "
                  f"3 threads (the reference's OMP_NUM_THREADS=3): {o['timed_passes']} passes, median {o['median_s']:.2f} s "
                  f"(p10 {o['p10_s']:.2f}, p90 {o['p90_s']:.2f}); {a['threads']} threads: {a['timed_passes']} passes, "
                  f"median {a['median_s']:.2f} s (p10 {a['p10_s']:.2f}, p90 {a['p90_s']:.2f})"
                  + ("" if full is None else f"; plus ONE unscaled pass over a {full['voxels']}-voxel scene with "
                                             f"{full['threads']} threads: {full['seconds']:.1f} s"),
    }


def run_ncut(args, dev):
    """Secondary measurement (BASELINE.json configs[4]): the masked-NCut loop — 20 iterations of
    affinity -> generalized Fiedler vector -> bipartition — over one 625-segment, two-modality scene."""
    from unscene3d_amd.pseudo_masks import ncut
    from unscene3d_amd.synthetic import make_segment_scene

    from unscene3d_amd.pseudo_masks.driver import PseudoMaskDriver

    K = max(1, args.scenes)
    feats, conn, _ = make_segment_scene(75, side=25, dims=(384, 96), n_objects=16)
    S = feats[0].shape[0]
    uniq = torch.arange(S)
    conn_t = torch.from_numpy(conn)
    dfe = tuple(torch.from_numpy(f).to(dev) for f in feats)
    # a step = one round of K scenes (the same synthetic scene K times: identical work per slot); K = 1 is the
    # single chain of round 1
    scenes = [{"features": (dfe[0].clone(), dfe[1].clone()), "unique_segments": uniq, "seg_connectivity": conn_t}
              for _ in range(K)]
    driver = PseudoMaskDriver(device=dev, concurrent=K)

    def run():
        for sc in scenes:
            sc["features"] = (dfe[0].clone(), dfe[1].clone())
        return driver.run(scenes)
    for _ in range(args.warmup):
        res = run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps / K          # seconds per scene
    masks = res[0]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {f"masks_{i}": torch.as_tensor(m) for i, m in sorted(res.items())})
    flops = 4.0 / 3.0 * S ** 3
    roof = None
    if args.full:
        # eigensolver alone (device time of one usc_ncut_fiedler call)
        A, D = ncut.get_affinity_matrix((dfe[0].clone(), dfe[1].clone()), tau=0.6)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ncut.second_smallest_eigenvector(A, D)
        e0.record()
        for _ in range(5):
            ncut.second_smallest_eigenvector(A, D)
        e1.record()
        torch.cuda.synchronize()
        eig_ms = e0.elapsed_time(e1) / 5
        # a chain of S-1 dependent Householder steps, one grid-wide exchange each: neither HBM nor the matrix cores bound
        # it.  What it is priced against is the exchange: the guide's ~4 us for one all-workgroup hand-over
        # (MI355X_MICROARCH.md, grid barrier 4-7 us) — `frac` = that floor / the measured time per step of the solve
        # (1 = nothing but exchanges)
        roof = {"bound": "latency", "kernel": "usc_ncut_fiedler (tridiagonalisation + bisection + inverse iteration)",
                "chain_steps": S - 1, "us_per_chain_step": 1e3 * eig_ms / max(1, S - 1), "exchange_floor_us": 4.0,
                "achieved": 1e3 * eig_ms / max(1, S - 1), "peak": 4.0, "unit": "us per dependent step (lower is better)",
                "frac": 4.0 / (1e3 * eig_ms / max(1, S - 1)), "traffic": None, "avg_call_ms": eig_ms,
                "f64_gflop_per_call": flops / 1e9}
    cpu = None
    if args.full and not args.no_cpu_baseline:
        from oracle import ncut_ref
        tf = tuple(torch.from_numpy(f) for f in feats)
        c0 = time.perf_counter()
        ref = ncut_ref.unscene3d_ref((tf[0].clone(), tf[1].clone()), np.arange(S), conn, tau=0.6, max_instances=20,
                                     min_segment_size=4)
        cdt = time.perf_counter() - c0
        cpu = {"value": 1.0 / cdt, "unit": "scenes/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"oracle/ncut_ref.unscene3d_ref (numpy + scipy.linalg.eigh subset) on the same {S}-segment "
                         f"scene, {cdt:.2f} s, {ref.shape[0]} masks"}
    print(json.dumps({
        "metric": "pseudo-mask scenes/sec (masked NCut, 625 segments, 20 iterations)", "value": 1.0 / dt,
        "scenes_in_flight": K,
        "unit": "scenes/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[4]: iterative masked NCut (affinity + generalized Fiedler vector, "
                               f"20 iterations) on one synthetic {S}-segment scene, DINO-like 384-d + CSC-like 96-d "
                               "segment features", "segments": S, "masks": int(masks.shape[0])},
        "roofline": roof,
        "cpu_baseline": cpu,
    }))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args):
    """`bench.py --gpus N` started as ONE process: re-execute through torch.distributed.run with N ranks on this node
    (the reference gets its ranks from pl.Trainer(gpus=cfg.general.gpus), main_instance_segmentation.py:86-92)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    import subprocess
    return subprocess.run(cmd, env=env).returncode


def run_dry_collectives(args, dev, rank, world):
    """The collectives of one step, alone: 13 x scalar all-reduce, then the flat gradient buffer of the
    real model in the BucketedGradReducer's buckets (last bucket first: the order backward finishes them), then the
    same bytes as ONE all-reduce.  Device time per collective from HIP events around blocking calls; median of `--steps`
    repetitions after `--warmup`.  Prints one JSON line on rank 0."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.ddp import BucketedGradReducer, flatten_grads
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    cfg = apply_overrides(default_config(), ["general.num_targets=3", f"data.batch_size={world}"])
    torch.manual_seed(1234)
    module = InstanceSegmentation(cfg).to(dev).train()
    params = [p for n, p in module.named_parameters() if ".backbone.final." not in n]
    flat = flatten_grads(params)
    red = BucketedGradReducer(params, flat, world)
    bounds = red.bounds
    nm = torch.ones(1, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def masks():
        for _ in range(13):
            dist.all_reduce(nm)

    def one_flat():
        dist.all_reduce(flat)

    per_bucket = [[] for _ in bounds]
    t_masks, t_flat, t_buckets_async = [], [], []
    for it in range(args.warmup + args.steps):
        keep = it >= args.warmup
        a = timed(masks)
        for b in reversed(range(len(bounds))):
            s_, e_ = bounds[b]
            t = timed(lambda: dist.all_reduce(flat[s_:e_]))
            if keep:
                per_bucket[b].append(t)

        def all_async():
            hs = [dist.all_reduce(flat[s_:e_], async_op=True) for s_, e_ in reversed(bounds)]
            for h in hs:
                h.wait()
        c = timed(all_async)
        d = timed(one_flat)
        if keep:
            t_masks.append(a); t_buckets_async.append(c); t_flat.append(d)
        flat.zero_()
    med = lambda v: float(np.median(v)) if v else None
    ts = [med(t_masks), med(t_buckets_async), med(t_flat)] + [med(v) for v in per_bucket]
    t = torch.tensor(ts, device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ts = t.tolist()
    if rank == 0:
        mb = [(e - s) * 4 / 1e6 for s, e in bounds]
        print(json.dumps({
            "mode": "dry-collectives", "n_gpus": world, "backend": args.dist_backend, "steps": args.steps,
            "gradient_mb": flat.numel() * 4 / 1e6, "num_masks_13_allreduces_ms": ts[0],
            "buckets_async_in_schedule_order_ms": ts[1], "one_flat_allreduce_ms": ts[2],
            "buckets": [{"index": b, "mb": mb[b], "blocking_ms": ts[3 + b],
                         "algbw_gbs": (mb[b] / 1e3) / (ts[3 + b] / 1e3) if ts[3 + b] else None} for b in range(len(bounds))],
            "note": "max over ranks of per-rank medians; the bucketed exchange of a real step starts during backward "
                    "(5 of 6 buckets at 150 k voxels) and can hide under the ~9 ms the backward pass still runs after "
                    "the first bucket is complete; compare buckets_async_in_schedule_order_ms with ms_per_step"}))


def _in_step_roofline(ring, meta, n_rec, khz, steps):
    """Per kernel variant: launches, mean duration and rate of the tile-compacted kernel inside the timed steps, from the
    marks its workgroups wrote (ring rows: min start tick, max end tick, real pairs, 0)."""
    out = {}
    if n_rec <= 0 or khz <= 0:
        return None
    for i in range(n_rec):
        t0, t1, pairs = int(ring[i, 0]), int(ring[i, 1]), int(ring[i, 2])
        if t1 <= t0 or t0 == 0xFFFFFFFFFFFFFFFF:
            continue
        m = meta[i]
        a = out.setdefault(f"usc::gather_gemm_compact_kernel<{m.nb}>", {"launches": 0, "ms": 0.0, "flops": 0.0})
        a["launches"] += 1
        a["ms"] += (t1 - t0) / khz
        a["flops"] += 2.0 * pairs * m.cin * m.cout
    return {k: {"launches_per_step": v["launches"] / max(1, steps), "avg_launch_us": 1e3 * v["ms"] / v["launches"],
                "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12, "gflop_per_launch": v["flops"] / v["launches"] / 1e9}
            for k, v in out.items() if v["launches"]}


def main():
    args = parse()
    if args.mode == "ncut":
        torch.cuda.set_device(0)
        return run_ncut(args, torch.device("cuda", 0))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # --force-dist: a ONE-rank process group (RCCL with world_size 1 works on one device): the bucketed gradient reducer,
    # the criterion's num_masks all-reduce and RCCL's own streams run exactly as on N ranks, minus the wire
    multi = world > 1 or args.force_dist
    if args.force_dist and world == 1:
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch exactly one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    if args.dist_backend == "nccl" and world > torch.cuda.device_count():
        raise SystemExit(f"bench.py: {world} ranks over RCCL need {world} devices, this node shows "
                         f"{torch.cuda.device_count()} (--dist-backend gloo shares devices; smoke test only)")
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.dist_backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
        if world > torch.cuda.device_count():
            # ranks SHARE a device (a code-path check on a one-GPU box, never a deployment): two processes with four
            # streams each on one device degenerate — 1.5-6 s per step, 100 ms with the lane or the key-preparation
            # stream off (tools/ab.sh, round 5; the queues of different processes are time-sliced) — so the shared-device run
            # keeps the second streams off unless the caller set the switches
            os.environ.setdefault("USC3D_WGRAD_LANE_MAX_ROWS", "0")
            os.environ.setdefault("USC3D_KV_SIDE_STREAM", "0")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    numa_cpus = _pin_to_device_numa(dev)
    if multi:
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world,
                                **({"device_id": dev} if args.dist_backend == "nccl" else {}))
        assert dist.get_world_size() == args.gpus

    from unscene3d_amd import profiler
    from unscene3d_amd.ddp import flatten_grads
    from unscene3d_amd.synthetic import make_scene

    if args.dry_collectives:
        if world < 2:
            raise SystemExit("bench.py --dry-collectives: needs --gpus N with N >= 2 (one rank has no collective)")
        run_dry_collectives(args, dev, rank, world)
        dist.destroy_process_group()
        return
    if args.mode == "backbone":
        model = build_model(dev)
        params = [p for n, p in model.named_parameters() if not n.startswith("final.")]  # unused in forward
        flat = flatten_grads(params)
        opt = torch.optim.AdamW(params, lr=1e-4, fused=True)
        sc = make_scene(2000 + rank, target_voxels=args.voxels)
        xyz = torch.from_numpy(sc["xyz"]).to(dev)
        colors = torch.from_numpy(sc["colors"]).to(dev)
        step = lambda w: train_step(model, opt, xyz, colors, flat, w)
        step.params = params
    else:
        step = make_mask3d_step(args, dev, rank, world)

    steady = None
    for w in range(args.warmup):
        loss, nvox = step(world)
        if w == max(0, args.warmup - 2) and args.mode == "mask3d" and os.environ.get("USC3D_STEADY", "1") == "1":
            # the trainer's one-time preparation of the steady state (stream pools pre-sized from the high-water mark,
            # interpreter heap frozen): before the LAST warm-up step, which refills the small-block pools
            from unscene3d_amd.trainer.trainer import prepare_steady_state
            steady = prepare_steady_state(dev)
    torch.cuda.synchronize()
    if multi and args.dist_backend == "nccl" and args.mode == "mask3d" and os.environ.get("USC3D_STREAM_RECHECK", "0") == "1":
        # (Off by default since the step issues no ASYNCHRONOUS collective any more — the reducer's buckets and the
        #  criterion's num_masks are synchronous all-reduces on the rank's own streams, ddp.py — so RCCL's internal stream
        #  is not in play; the probe itself puts an asynchronous all-reduce in flight.  USC3D_STREAM_RECHECK=1:)
        # RCCL's stream exists now (first collective done): do the lane and the key stream still run beside the compute
        # stream with an all-reduce in flight?  A stream that does not is switched off (config.streams says so).
        from unscene3d_amd import streams
        if any(r.get("switched_off") for r in streams.recheck_under_collective(dev)):
            for _ in range(2):
                loss, nvox = step(world)
            torch.cuda.synchronize()
    # the dominant kernel marks its own start / end (device wall clock) and counts its real pairs during the TIMED steps
    # (usc_launch_stats_begin: two atomics per workgroup) -> roofline.frac_in_step describes the configuration `value`
    # is measured in — lane, step program, captured decoder passes and all
    lstat_ring = None
    if args.full and args.mode == "mask3d" and rank == 0:
        import ctypes as C
        from unscene3d_amd._lib import LaunchStat, check, lib
        lstat_slots = max(4096, 32 * args.steps)
        lstat_ring = torch.zeros(4 * lstat_slots, dtype=torch.int64, device=dev)
        check(lib.usc_launch_stats_begin(lstat_ring.data_ptr(), lstat_slots, torch.cuda.current_stream().cuda_stream),
              "usc_launch_stats_begin")
        torch.cuda.synchronize()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)] if args.rotate else None
    own = getattr(step, "state", None) if (marks and world > 1) else None
    if own is not None:
        own["marks"] = []                  # per step: the point where this rank's backward is queued (before the exchange)
    if marks:
        marks[0].record()
    nvox_sum = 0
    for k in range(args.steps):
        loss, nvox = step(world)
        nvox_sum += int(nvox)
        if marks:
            marks[k + 1].record()          # device-side step boundaries (no host wait inside the timed loop)
    nvox = nvox_sum / max(1, args.steps)   # mean voxels per step over the timed loop (the rotated scenes differ)
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    in_step = None
    if lstat_ring is not None:
        meta = (LaunchStat * lstat_slots)()
        n_rec = int(lib.usc_launch_stats_end(meta, lstat_slots))
        in_step = _in_step_roofline(lstat_ring.cpu().numpy().astype("uint64").reshape(-1, 4), meta, n_rec,
                                    int(lib.usc_wall_clock_khz()), args.steps)
    own_marks = None
    if own is not None:                    # freeze the timed loop's marks (later steps must not append to them)
        own_marks, own["marks"] = own["marks"], None
    if multi:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(loss, getattr(step, "state", {}).get("losses"), step.params))

    # The same K steps once more in the OTHER row order: `value` is measured in the reference's first-occurrence order
    # (ME.utils.sparse_quantize, datasets/utils.py:403-408 — FPS starts at row 0 and key sampling indexes rows, so this is
    # the order in which the step picks the queries / keys the reference would pick on the same raw scene);
    # `value_zorder` groups the rows into z-ordered cells (a consistent permutation of every per-voxel array).  When
    # --spatial-sort SHIFT makes z-order the measured order, the second loop is the reference order instead.
    ref_order = None
    other = 0 if args.spatial_sort else args.zorder_shift
    if (args.full and args.mode == "mask3d" and not args.no_second_order and hasattr(step, "set_spatial_sort")
            and (other or args.spatial_sort)):
        step.set_spatial_sort(other)
        for _ in range(max(2, args.warmup)):
            step(world)
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()
        r0 = time.perf_counter()
        for k in range(args.steps):
            step(world)
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()
        rdt = time.perf_counter() - r0
        if multi:
            t = torch.tensor([rdt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            rdt = float(t.item())
        tag = "zorder" if other else "reference_order"
        ref_order = {f"value_{tag}": world * getattr(step, "scenes_per_rank", 1) * args.steps / rdt,
                     f"ms_per_step_{tag}": 1e3 * rdt / args.steps}
        step.set_spatial_sort(args.spatial_sort)
        step(world)                         # back in the measured configuration for the instrumented step below

    # roofline of the dominant kernel: one extra instrumented step (HIP events around every conv launch on
    # the launch stream; not part of the timed region so that event overhead does not pollute `value`)
    # Every rank runs it (the criterion's num_masks all-reduce and the gradient all-reduce are collectives); rank 0
    # reports.
    roof = None
    if args.full:
        with profiler.capture() as prof:
            step(world)
            torch.cuda.synchronize()
    if args.full and rank == 0:
        roof = prof.roofline(MFMA_F32_PEAK_TFLOPS)
        if roof is not None:
            # PMC counters cannot be read from inside the process; `traffic` is the per-launch HBM byte count
            # of the same kernel from the committed rocprofv3 --pmc passes over this very command.
            roof.update(_committed_traffic(roof["kernel"]))
            roof["frac_measured_on"] = ("ONE extra step after the timed loop on the per-operator issue path (an open profiler "
                                        "capture switches the step program, the native units and the weight-gradient lane "
                                        "off): HIP events around every convolution launch = the kernel ALONE")
            if in_step is not None and in_step.get(roof["kernel"]):
                d = in_step[roof["kernel"]]
                roof.update({"frac_in_step": d["tflops"] / MFMA_F32_PEAK_TFLOPS, "achieved_in_step": d["tflops"],
                             "avg_launch_us_in_step": d["avg_launch_us"], "launches_per_step_in_step": d["launches_per_step"],
                             "algorithmic_gflop_per_launch_in_step": d["gflop_per_launch"],
                             "frac_in_step_measured_on": "the K timed steps themselves (lane, step program, captured decoder "
                                                         "passes on): first-workgroup-start / last-workgroup-end wall-clock "
                                                         "marks and the real pair count written by the kernel's own "
                                                         "workgroups (usc_launch_stats_begin)",
                             "in_step_all": in_step})

    ranks_seen = None
    if multi:
        ranks_seen = _ranks_seen(dev, rank, world, args.dist_backend, getattr(step, "params", None))

    spr = getattr(step, "scenes_per_rank", 1)
    rot = None
    if marks:
        per_in_order = [marks[k].elapsed_time(marks[k + 1]) for k in range(args.steps)]
        per = sorted(per_in_order)
        q = lambda f: per[min(len(per) - 1, int(round(f * (len(per) - 1))))]
        rot = {"rotated_scene_sets": args.rotate, "rotate_spread": args.rotate_spread, "step_ms_p10": q(0.1), "step_ms_p50": q(0.5), "step_ms_p90": q(0.9),
               "step_ms_min": per[0], "step_ms_max": per[-1],
               "step_ms_max_at": int(max(range(args.steps), key=lambda k: per_in_order[k])),
               **({"step_ms_all": [round(v, 2) for v in per_in_order]} if os.environ.get("USC3D_BENCH_STEP_LIST") else {})}
    skew = None
    if own_marks is not None and len(own_marks) == args.steps:
        # per-rank step-time skew: how long each rank's OWN work of a step took (step start -> backward queued, device
        # time), all-gathered; max / mean over the ranks of a step = what the gradient exchange makes the others wait
        mine_ms = torch.tensor([marks[k].elapsed_time(own_marks[k]) for k in range(args.steps)], device=dev)
        allr = [torch.empty_like(mine_ms) for _ in range(world)]
        dist.all_gather(allr, mine_ms)
        tab = torch.stack(allr).cpu().numpy()                                  # [world, steps]
        ratio = tab.max(0) / tab.mean(0)
        skew = {**(step.skew_info or {}), "rank_own_work_ms_mean": [float(v) for v in tab.mean(1)],
                "step_own_work_max_over_mean": {"mean": float(ratio.mean()), "max": float(ratio.max())}}
    if rank == 0:
        line = {
            "metric": "training scenes/sec (Res16UNet34C+Mask3D, 150k voxels)",
            "value": world * spr * args.steps / dt, "unit": "scenes/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, **(ref_order or {}), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": WORKLOADS[args.mode].format(nvox=int(nvox) // spr, spr=spr),
                       "voxels_per_scene": int(nvox) // spr, "scenes_per_gpu": spr, "global_batch": world * spr,
                       "parallelism": f"dp{world}", "row_order": (f"z-order cells of {2 ** args.spatial_sort}^3 voxels "
                                                                   f"(value); first-occurrence (value_reference_order)"
                                                                   if args.mode == "mask3d" and args.spatial_sort else
                                                                   "first-occurrence = the reference's (value)" +
                                                                   (f"; z-order cells of {2 ** args.zorder_shift}^3 voxels (value_zorder)"
                                                                    if ref_order else "")), **(rot or {}), **({"rank_skew": skew} if skew else {}),
                       "loss": float(loss), "grad_allreduce": _allreduce_note(step, world),
                       "streams": _stream_report(),
                       "steady_state": steady,
                       "cpu_affinity": numa_cpus,
                       "optimizer": ("FlatAdamW, the trunk's ranges stepped inside the backward pass (enable_early)"
                                     if getattr(getattr(step, "opt", None), "_early_stream", None) is not None else "one launch after backward"),
                       **({} if ranks_seen is None else ranks_seen)},
            "roofline": roof,
            "cpu_baseline": (_unpinned(cpu_baseline, args.cpu_sample_voxels, args.mode)
                             if args.full and not args.no_cpu_baseline and world == 1 else None),
        }
        print(json.dumps(line))
    if hasattr(step, "close"):
        step.close()
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
