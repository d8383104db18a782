#!/usr/bin/env python
"""Times the set criterion (forward + backward through SetCriterion) at 100, 150 and 256 queries on synthetic tables:
L = 13 levels, B in {1, 8} scenes of S in {600, 3000} segments and T = 20 targets, the mask logits in tables padded to
the next multiple of 32 columns (100 -> 128, 150 -> 160), as models.mask3d._mask_logits hands them over.

    python tools/criterion_queries_bench.py [--rounds 7] [--iters 20] [--warmup 10] [--out profiles/criterion_queries_bench.txt]

Above 128 queries the device path (SetCriterion(device_max_queries=256), csrc/criterion.hip) and the torch-operator
path (the default, device_max_queries=128) run in the same process on the same inputs, alternating round by round; the
100-query row (device path, the default) is the reference point.  A round is --iters calls between two device events
(the operator path's device->host copy and host solves stall the stream, so they are inside the window); the table
gives the median per call over the rounds with min ... max.  Launches per call are counted once per path with the torch
profiler (every kernel the device executes, the library's and torch's, the few of the weighted sum over the loss table
and its backward included).  Needs a HIP device: there is no fallback."""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criterion_queries_bench.txt"))
    a = ap.parse_args()
    import torch

    from unscene3d_amd._lib import lib, require_device
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    require_device()
    warnings.filterwarnings("ignore", message=".*torch-operator path.*")
    dev = torch.device("cuda:0")
    L, T, C = 13, 20, 4
    weights = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0, "loss_noise_robust": 0.0}

    wvec = torch.tensor([weights[k] for k in ("loss_ce", "loss_mask", "loss_dice", "loss_noise_robust")] * L, device=dev)

    def criterion(max_queries):
        matcher = HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, cost_noise_robust=0.0, num_points=-1)
        return SetCriterion(num_classes=C, matcher=matcher, weight_dict=dict(weights), eos_coef=0.1,
                            losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0, importance_sample_ratio=0.75,
                            class_weights=-1, device_max_queries=max_queries).to(dev)

    def inputs(B, S, Q):
        g = torch.Generator().manual_seed(1000 * B + S + Q)
        ld = -(-Q // 32) * 32
        targets, tables = [], []
        for b in range(B):
            tm = torch.rand(T, S, generator=g) < 0.1
            tm[:, 0] = True
            targets.append({"labels": (torch.arange(T) % (C - 1)).to(dev), "segment_mask": tm.to(dev)})
            # a half-trained model: query (Q // T) t leans towards target t (above 128 queries some of those are in the
            # second column group), everything else is noise
            x = torch.randn(L, S, ld, generator=g) * 3
            step = Q // T
            x[:, :, 0:step * T:step] += (tm.T.float() * 2 - 1)[None] * 4
            x[:, :, Q:] = 0
            tables.append([x[l].to(dev).requires_grad_(True) for l in range(L)])
        logits = [(torch.randn(B, Q, C, generator=g) * 2).to(dev).requires_grad_(True) for _ in range(L)]
        return targets, tables, logits, ld

    def call(crit, targets, tables, logits, Q):
        levels = []
        for l in range(L):
            views = []
            for b in range(len(targets)):
                v = tables[b][l][:, :Q]
                if tables[b][l].shape[1] > Q:
                    v._usc_padded = tables[b][l]
                views.append(v)
            levels.append({"pred_logits": logits[l], "pred_masks": views})
        losses = crit(dict(levels[0], aux_outputs=levels[1:]), targets, mask_type="segment_mask")
        (losses.flat * wvec).sum().backward()                 # the trainer's weighted sum: one product over the table
        for t in logits + [t for ts in tables for t in ts]:
            t.grad = None

    def launches(fn):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA
                   and not any(w in e.name.lower() for w in ("memcpy", "memset", "copy")))

    lines = [f"# criterion forward + backward through SetCriterion; L = {L}, T = {T}; library: {lib.usc_build_info().decode()}",
             f"# ms per call: median over {a.rounds} rounds of {a.iters} calls between device events (min ... max); "
             f"{a.warmup} warm-up calls per path",
             f"{'B':>2} {'S':>5} {'Q':>4} {'ld':>4}  {'path':<9} {'ms per call':<30} {'launches':>8}  on device"]
    for B in (1, 8):
        for S in (600, 3000):
            for Q in (100, 150, 256):
                targets, tables, logits, ld = inputs(B, S, Q)
                paths = [("device", criterion(256 if Q > 128 else 128))]
                if Q > 128:
                    paths.append(("operator", criterion(128)))
                fns = {name: (lambda c=c: call(c, targets, tables, logits, Q)) for name, c in paths}
                for fn in fns.values():
                    for _ in range(a.warmup):
                        fn()
                ms = {name: [] for name in fns}
                for _ in range(a.rounds):                      # the paths alternate round by round
                    for name, fn in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        for _ in range(a.iters):
                            fn()
                        e1.record()
                        e1.synchronize()
                        ms[name].append(e0.elapsed_time(e1) / a.iters)
                for name, c in paths:
                    c.check_lsap_status(wait=True)
                    on_dev = bool(c.last_indices[0][0][0].is_cuda)
                    assert on_dev == (name == "device"), (name, Q)
                    try:
                        n = str(launches(fns[name]))
                    except Exception as e:                    # the count is an extra: the timings stand without it
                        n = f"not measured ({type(e).__name__})"
                    v = ms[name]
                    lines.append(f"{B:>2} {S:>5} {Q:>4} {ld:>4}  {name:<9} "
                                 f"{f'{np.median(v):.3f} ({min(v):.3f} ... {max(v):.3f})':<30} {n:>8}  {on_dev}")
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))
    print("written:", a.out)


if __name__ == "__main__":
    main()
