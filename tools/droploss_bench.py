#!/usr/bin/env python
"""Times the set criterion (forward + backward) and the whole training step with and without DropLoss, on the device
criterion (csrc/criterion.hip) and on the torch-operator path, at the criterion's real shapes: L = 13 levels, Q = 100
queries in the padded [S, 128] tables, S segments and T targets of one synthetic scene of --voxels voxels.

    python tools/droploss_bench.py --voxels 150000 --iters 50 --warmup 10 --repeats 3 [--step] [--package-root DIR]

--package-root DIR imports unscene3d_amd from DIR instead of this tree (a checkout of another commit next to a built
libusc3d_hip.so): on a commit whose device criterion refuses DropLoss, "device+drop" is that commit's operator path.
Every iteration is bracketed by a device synchronisation and timed on the host clock (the operator path contains a
device->host copy, so device-side events alone would miss its host share).  Prints the median, the 10th / 90th
percentile and the spread of the medians over --repeats runs per variant, then one JSON line.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=150_000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time the whole training step (eager, one scene)")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    import torch

    import unscene3d_amd
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.models import criterion as crit_mod
    from unscene3d_amd.trainer.trainer import InstanceSegmentation
    warnings.filterwarnings("ignore", message=".*torch-operator path.*")
    dev = torch.device("cuda:0")
    ds = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=a.voxels, seed=3100)
    collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="train", device=str(dev), spatial_sort=False)
    batch = collate([ds[0]])
    target = batch[1]
    tm = target[0]["segment_mask"]
    T, S = int(tm.shape[0]), int(tm.shape[1])
    L, Q, ld = 13, 100, 128
    print(f"package {os.path.dirname(unscene3d_amd.__file__)}; scene: {batch[0].coordinates.shape[0]} voxels, S = {S} "
          f"segments, T = {T} targets; L = {L}, Q = {Q}, ld = {ld}")

    def module(drop):
        cfg = apply_overrides(default_config(), [f"loss.use_droploss={drop}"])
        torch.manual_seed(7)
        return InstanceSegmentation(cfg).to(dev).train()

    g = torch.Generator().manual_seed(5)
    C = module(False).criterion.num_classes + 1
    # mask logits of a half-trained model: query t leans towards target t, everything else is noise, so that DropLoss
    # keeps some pairs and drops others
    base = torch.randn(L, S, ld, generator=g) * 3
    lean = (tm.T.float().cpu() * 2 - 1)[None] * torch.rand(L, 1, T, generator=g) * 4
    base[:, :, :T] += lean
    base[:, :, Q:] = 0
    tables = [base[l].to(dev).requires_grad_(True) for l in range(L)]
    logits = [(torch.randn(1, Q, C, generator=g) * 2).to(dev).requires_grad_(True) for _ in range(L)]

    def criterion_once(crit):
        levels = []
        for l in range(L):
            v = tables[l][:, :Q]
            v._usc_padded = tables[l]
            levels.append({"pred_logits": logits[l], "pred_masks": [v]})
        losses = crit(dict(levels[0], aux_outputs=levels[1:]), target, mask_type="segment_mask")
        total = sum(v * crit.weight_dict.get(k, 1.0) for k, v in losses.items())
        total.backward()
        for t in tables + logits:
            t.grad = None
        return total

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        meds, all_ms = [], []
        for _ in range(a.repeats):
            ms = []
            for _ in range(a.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            meds.append(float(np.median(ms)))
            all_ms += ms
        return dict(median_ms=float(np.median(meds)), p10_ms=float(np.percentile(all_ms, 10)),
                    p90_ms=float(np.percentile(all_ms, 90)), medians_ms=meds, spread_ms=max(meds) - min(meds))

    result = {"voxels": int(batch[0].coordinates.shape[0]), "S": S, "T": T, "L": L, "Q": Q,
              "package": os.path.dirname(unscene3d_amd.__file__)}
    for fused in (True, False):
        for drop in (False, True):
            crit_mod.FUSED = fused
            m = module(drop)
            name = f"criterion {'device' if fused else 'operator'}{'+drop' if drop else ''}"
            r = timed(lambda: criterion_once(m.criterion))
            if drop and getattr(m.criterion, "last_drop_weights", None) is not None:
                w = torch.cat([x for lv in m.criterion.last_drop_weights for x in lv])
                r["kept"], r["pairs"] = int(w.sum()), int(w.numel())
            r["on_device"] = bool(m.criterion.last_indices[0][0][0].is_cuda)
            result[name] = r
            print(f"{name:28s} median {r['median_ms']:.3f} ms  p10 {r['p10_ms']:.3f}  p90 {r['p90_ms']:.3f}  medians "
                  f"{['%.3f' % x for x in r['medians_ms']]}  device path {r['on_device']}  kept {r.get('kept')}/{r.get('pairs')}")
            if a.step:
                def step():
                    out = m.training_step(batch)
                    out[0].backward()
                    m.zero_grad(set_to_none=True)
                r = timed(step)
                result["step" + name[len("criterion"):]] = r
                print(f"{'step' + name[len('criterion'):]:28s} median {r['median_ms']:.3f} ms  p10 {r['p10_ms']:.3f}  p90 "
                      f"{r['p90_ms']:.3f}  medians {['%.3f' % x for x in r['medians_ms']]}")
            del m
    crit_mod.FUSED = True
    print(json.dumps(result))


if __name__ == "__main__":
    main()
