"""Developer aid: InstanceSegmentation.eval_step above 128 queries, fused attention (USC3D_FUSED_ATTN_WIDE=1, the
default) against the plain-operator branch (=0), alternated in one process after warm-up: device time per call (events
around a call that ends in a synchronise) and peak allocated memory of each — over the whole eval_step and inside the
model forward alone (the criterion and the export that follow it allocate more than the decoder does).

    python tools/attn_wide_eval.py --queries 150 --voxels 150000 --reps 12 [--test-mode]
--test-mode: data.test_mode=test, the reference's export recipe (no criterion in eval_step).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=150)
    ap.add_argument("--voxels", type=int, default=150_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--test-mode", action="store_true")
    args = ap.parse_args()

    from unscene3d_amd import _lib
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.models import mask3d
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    dev = torch.device("cuda:0")
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "data.batch_size=1",
                                             f"model.num_queries={args.queries}"]
                          + (["data.test_mode=test"] if args.test_mode else []))
    ds = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=args.voxels, seed=2000)
    vbatch = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="validation", device=str(dev))([ds[0]])
    torch.manual_seed(0)
    module = InstanceSegmentation(cfg).to(dev).eval()
    model_forward = module.model.forward
    fwd_peak = [0.0, 0.0]          # peak before the model forward, peak inside it

    def forward_with_peak(*a, **kw):
        fwd_peak[0] = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = model_forward(*a, **kw)
        fwd_peak[1] = torch.cuda.max_memory_allocated()
        return out

    module.model.forward = forward_with_peak

    def one(fused):
        mask3d._FUSED_ATTN_WIDE = fused
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        module.eval_step(vbatch)
        b.record()
        b.synchronize()
        whole = max(fwd_peak[0], torch.cuda.max_memory_allocated())
        return a.elapsed_time(b), whole / 2 ** 20, fwd_peak[1] / 2 ** 20

    for _ in range(args.warmup):
        one(True), one(False)
    ms = {True: [], False: []}
    peak = {True: 0.0, False: 0.0}
    peak_fwd = {True: 0.0, False: 0.0}
    for _ in range(args.reps):
        for fused in (True, False):
            t, m, mf = one(fused)
            ms[fused].append(t)
            peak[fused] = max(peak[fused], m)
            peak_fwd[fused] = max(peak_fwd[fused], mf)
    mask3d._FUSED_ATTN_WIDE = True
    print(f"eval_step{' (data.test_mode=test)' if args.test_mode else ''}, {args.queries} queries, {int(vbatch[0].coordinates.shape[0])} voxels, {args.reps} alternated calls "
          f"after {args.warmup} warm-up pairs; {torch.cuda.get_device_name(0)}; {_lib.lib.usc_build_info().decode()}")
    for fused, name in ((True, "fused (USC3D_FUSED_ATTN_WIDE=1)"), (False, "plain operators (=0)")):
        v = sorted(ms[fused])
        print(f"  {name:32s} median {statistics.median(v):8.2f} ms  min {v[0]:8.2f}  max {v[-1]:8.2f}  "
              f"peak allocated {peak[fused]:8.1f} MiB (model forward alone {peak_fwd[fused]:8.1f})")
    print(f"  ratio of medians plain / fused {statistics.median(ms[False]) / statistics.median(ms[True]):.3f}; "
          f"peak memory plain - fused: eval_step {peak[False] - peak[True]:.1f} MiB, model forward alone "
          f"{peak_fwd[False] - peak_fwd[True]:.1f} MiB")


if __name__ == "__main__":
    main()
