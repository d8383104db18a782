#!/usr/bin/env python
"""Inference precision f32 vs bf16 on the 150 k-voxel bench scene (unscene3d_amd.inference_precision).

* per shape: one trunk unit forward (conv + the unchanged f32 batch norm / ReLU, units.unit_forward) for every distinct
  (kind, level, cin, cout) of Res16UNet34C on the scene's own kernel maps, f32 kernels vs the bf16 cast + bf16 conv;
* the trunk forward (eval(), no_grad, step program) in both precisions;
* the whole InstanceSegmentation.eval_step (general.eval_precision) in both precisions.

Times are HIP-event medians over --reps calls after --warmup calls.  Kernel-level numbers (bytes moved, fraction of the
bf16 peak) come from rocprofv3 runs of this script.  Prints one JSON line.

    python tools/infer_bench.py [--reps 20] [--warmup 5] [--voxels 150000]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxels", type=int, default=150_000)
    args = ap.parse_args()

    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import inference_precision, precision, program, units
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    dev = torch.device("cuda:0")
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "data.batch_size=1"])
    ds = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=args.voxels, seed=2000)
    vbatch = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="validation", device=str(dev))([ds[0]])
    torch.manual_seed(0)
    module = InstanceSegmentation(cfg).to(dev).eval()
    trunk = module.model.backbone
    data = vbatch[0]
    feats = data.features[:, :3].contiguous().to(dev)
    x = ME.SparseTensor(coordinates=data.coordinates, features=feats, device=dev)
    res = {"voxels": int(x.F.shape[0]), "unit_us": []}

    # ---- per-shape unit forwards on the scene's maps
    with torch.no_grad():
        trunk(x)                                        # builds every map of the pyramid
        cm, ts = x.coordinate_manager, x._ts()
        pl = program.plan_of(trunk)
        rows = [cm.coord_map(ts << l).n for l in range(pl.n_levels)]
        seen = set()
        for op in pl.ops:
            if op["t"] != "unit":
                continue
            key = (op["kind"], op["lin"], op["kvol"], op["cin"], op["cout"])
            if key in seen:
                continue
            seen.add(key)
            t = ts << op["lin"]
            km = (cm.kmap_identity(t) if op["kvol"] == 1 else cm.kmap_cube(t, op["ksize"])) if op["kind"] == units.SAME \
                else (cm.kmap_down(t) if op["kind"] == units.DOWN else cm.kmap_down(t >> 1))
            W3 = units._w3(op["conv"].kernel).detach().contiguous()
            xin = torch.randn((rows[op["lin"]], op["cin"]), device=dev)
            f32 = timed(lambda: units.unit_forward(xin, W3, op["bn"], km, op["kind"], None, True), args.reps, args.warmup)
            ent = {"kind": ["same", "down", "up"][op["kind"]], "K": op["kvol"], "cin": op["cin"], "cout": op["cout"],
                   "rows_out": rows[op["lout"]], "f32": round(f32, 1)}
            if precision.shape_ok(op["kvol"], op["cin"], op["cout"]):
                wp = precision.pack_weights(W3)
                ent["bf16"] = round(timed(lambda: units.unit_forward(xin, W3, op["bn"], km, op["kind"], None, True, wp),
                                          args.reps, args.warmup), 1)
            res["unit_us"].append(ent)

    # ---- trunk forward and eval_step
    for prec in ("f32", "bf16"):
        def fwd():
            with inference_precision(prec), torch.no_grad():
                trunk(x)
        res[f"trunk_ms_{prec}"] = round(timed(fwd, args.reps, args.warmup) / 1e3, 3)

        def ev():
            module.config.general.eval_precision = prec
            module.eval_step(vbatch)
        res[f"eval_step_ms_{prec}"] = round(timed(ev, max(3, args.reps // 4), 2) / 1e3, 3)
    module.config.general.eval_precision = "f32"
    res["trunk_speedup"] = round(res["trunk_ms_f32"] / res["trunk_ms_bf16"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
