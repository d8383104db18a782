#!/usr/bin/env python
"""Training precision f32 vs bf16x2 vs bf16x3 (unscene3d_amd.training_precision, csrc/spconv_bf16.hip).

(a) Per unit: for every distinct stride-1 K = 27 unit shape of Res16UNet34C on the bench scene's own kernel maps, the
    forward and the input gradient, each as the kernel alone (operands already split / packed) and as the whole pass:
      fwd_kernel    usc_conv_forward                      | usc_spconv_gather_gemm_split on ready planes
      fwd_unit      usc_conv_bn_act_forward               | usc_conv_bn_act_forward_split (split + pack + conv + BN + ReLU)
      dgrad_kernel  usc_conv_backward, dx only            | usc_spconv_gather_gemm_split on ready planes, transposed pack
      dgrad_full    the same                              | split of dy + transposed pack + kernel
(b) Whole step: the training step of `tools/train.py --synthetic N --voxels V` (the same TrainLoop, scenes and seed) with
    general.train_precision switched between blocks of steps, under the default policy (precision.TRAIN_MIN_ROWS /
    TRAIN_MIN_CIN as committed) and with every covered unit forced onto the split path.

Method: the variants alternate inside this one process, round after round (f32, bf16x2, bf16x3, f32 again, ...), at
least three rounds; every call is timed with HIP events; reported are the median and min ... max over all rounds.  "f32"
is measured twice per round ("f32" and "f32_again"): the distance of those two is the spread a difference has to beat.

    python tools/train_precision_bench.py [--rounds 3] [--reps 10] [--voxels 150000] [--synthetic 8] [--steps 6]
                                          [--skip-step] [--out profiles/train_precision.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("f32", "bf16x2", "bf16x3", "f32_again")
PLANES = {"f32": 0, "bf16x2": 2, "bf16x3": 3, "f32_again": 0}


def event_times(fn, reps):
    """HIP-event time of each of `reps` calls, in microseconds."""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def summary(ts, digits=1):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], digits), "min": round(ts[0], digits), "max": round(ts[-1], digits), "n": len(ts)}


def alternate(fns, rounds, reps, warmup=3):
    """fns: variant -> callable.  Warm every variant up, then `rounds` rounds of `reps` timed calls per variant."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {v: [] for v in fns}
    for _ in range(rounds):
        for v, fn in fns.items():
            ts[v] += event_times(fn, reps)
    return {v: summary(t) for v, t in ts.items()}


def unit_shapes(args, dev):
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import ops, program, units
    from unscene3d_amd._lib import check, lib
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    cfg = apply_overrides(default_config(), ["general.num_targets=3", "data.batch_size=1"])
    ds = SyntheticFreeMaskDataset(n_scenes=1, target_voxels=args.voxels, seed=2000)
    batch = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="validation", device=str(dev))([ds[0]])
    torch.manual_seed(0)
    trunk = InstanceSegmentation(cfg).to(dev).train().model.backbone
    data = batch[0]
    x = ME.SparseTensor(coordinates=data.coordinates, features=data.features[:, :3].contiguous().to(dev), device=dev)
    with torch.no_grad():
        trunk(x)                                            # builds every map of the pyramid
    cm, ts = x.coordinate_manager, x._ts()
    pl = program.plan_of(trunk)
    rows = [cm.coord_map(ts << l).n for l in range(pl.n_levels)]
    out, seen = [], set()
    st = ops._stream()
    for op in pl.ops:
        if op["t"] != "unit" or op["kind"] != units.SAME or op["kvol"] == 1 or op["cin"] < 16:
            continue
        key = (op["lin"], op["cin"], op["cout"])
        if key in seen:
            continue
        seen.add(key)
        K, cin, cout, n = op["kvol"], op["cin"], op["cout"], rows[op["lin"]]
        km = cm.kmap_cube(ts << op["lin"], op["ksize"])
        nbr = km.keep[0]
        W3 = units._w3(op["conv"].kernel).detach().contiguous()
        xin, dy = torch.randn((n, cin), device=dev), torch.randn((n, cout), device=dev)
        y, dx = torch.empty((n, cout), device=dev), torch.empty((n, cin), device=dev)
        ws = units.workspace(max(lib.usc_conv_ws_bytes(km.ref, units.SAME, cin, cout),
                                 lib.usc_unit_split_ws_bytes(km.ref, units.SAME, cin, cout, 3)), dev)
        ent = {"level": op["lin"], "rows": n, "K": K, "cin": cin, "cout": cout}
        fk, fu, dk, df = {}, {}, {}, {}
        for v in VARIANTS:
            P = PLANES[v]
            if P == 0:
                def conv_f(): check(lib.usc_conv_forward(km.ref, units.SAME, xin.data_ptr(), cin, W3.data_ptr(), cout, None,
                                                         y.data_ptr(), ws.data_ptr(), ws.numel(), st), "usc_conv_forward")
                def conv_b(): check(lib.usc_conv_backward(km.ref, units.SAME, xin.data_ptr(), cin, W3.data_ptr(), cout,
                                                          dy.data_ptr(), dx.data_ptr(), 0, None, 0, ws.data_ptr(), ws.numel(), st),
                                    "usc_conv_backward")
                fk[v], dk[v], df[v] = conv_f, conv_b, conv_b
            else:
                xs, wp = ops.split_bf16(xin, P), ops.pack_w_split(W3, P)
                fk[v] = lambda xs=xs, wp=wp: ops.gather_gemm_split(xs, wp, K, cout, nbr, n, out=y)
                if cin % 32 == 0:
                    ds_, wt = ops.split_bf16(dy, P), ops.pack_w_split(W3, P, transposed=True)
                    dk[v] = lambda ds_=ds_, wt=wt: ops.gather_gemm_split(ds_, wt, K, cin, nbr, n, out=dx)
                    df[v] = lambda P=P: ops.gather_gemm_split(ops.split_bf16(dy, P), ops.pack_w_split(W3, P, transposed=True),
                                                               K, cin, nbr, n, out=dx)
            fu[v] = lambda P=P: units.unit_forward(xin, W3, op["bn"], km, units.SAME, None, True, None, P)
        ent["fwd_kernel_us"] = alternate(fk, args.rounds, args.reps)
        ent["fwd_unit_us"] = alternate(fu, args.rounds, args.reps)
        ent["dgrad_kernel_us"] = alternate(dk, args.rounds, args.reps)
        ent["dgrad_full_us"] = alternate(df, args.rounds, args.reps)
        # forward unit + whole input gradient: what the policy is decided on
        tot = {v: ent["fwd_unit_us"][v]["median"] + ent["dgrad_full_us"][v]["median"] for v in ent["dgrad_full_us"]}
        ent["fwd_unit_plus_dgrad_full_us"] = {v: round(t, 1) for v, t in tot.items()}
        ent["f32_spread_us"] = round(abs(tot["f32"] - tot["f32_again"]), 1)
        out.append(ent)
        print(json.dumps(ent), file=sys.stderr, flush=True)
    return out


def whole_step(args, dev):
    """tools/train.py's loop (world 1), the precision switched between blocks of `--steps` steps."""
    from unscene3d_amd import precision
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.trainer import InstanceSegmentation, TrainLoop
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "data.batch_size=1"])
    torch.manual_seed(1234)
    module = InstanceSegmentation(cfg).to(dev).train()
    n = max(1, args.synthetic)
    scenes = []
    for j in range(n):
        scale = 1.0 if n == 1 else 1.0 + 0.02 - 2 * 0.02 * ((j * 5) % n) / max(1, n - 1)
        scenes.append(SyntheticFreeMaskDataset(n_scenes=1, target_voxels=int(args.voxels * scale),
                                               seed=2000 if j == 0 else 2000 + 16 * j)[0])
    res = {}
    default_policy = (precision.TRAIN_MIN_ROWS, precision.TRAIN_MIN_CIN)
    with TrainLoop(module, cfg, scenes, device=dev, early_optimizer=True, total_steps=100000, steady_after=2, resident=True,
                   shuffle=True, seed=2000) as loop:
        def block(prec, policy, steps):
            cfg.general.train_precision = prec
            precision.TRAIN_MIN_ROWS, precision.TRAIN_MIN_CIN = policy
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            marks[0].record()
            for k in range(steps):
                loop.step()
                marks[k + 1].record()
            torch.cuda.synchronize()
            return [marks[k].elapsed_time(marks[k + 1]) for k in range(steps)]

        variants = [("f32", "f32", default_policy), ("bf16x2_default_policy", "bf16x2", default_policy),
                    ("bf16x3_default_policy", "bf16x3", default_policy), ("bf16x2_every_unit", "bf16x2", (0, 0)),
                    ("bf16x3_every_unit", "bf16x3", (0, 0)), ("f32_again", "f32", default_policy)]
        for name, prec, policy in variants:                    # steady state, and every variant's shapes warmed up
            block(prec, policy, 3 if name == "f32" else 2)
        ts = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, prec, policy in variants:
                ts[name] += block(prec, policy, args.steps)
        precision.TRAIN_MIN_ROWS, precision.TRAIN_MIN_CIN = default_policy
        cfg.general.train_precision = "f32"
        res["ms_per_step"] = {name: summary(t, 3) for name, t in ts.items()}
        res["skipped"] = loop.skipped
    res["policy_default"] = {"TRAIN_MIN_ROWS": default_policy[0], "TRAIN_MIN_CIN": default_policy[1]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--voxels", type=int, default=150_000)
    ap.add_argument("--synthetic", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6, help="steps per block of the whole-step measurement")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-units", action="store_true")
    ap.add_argument("--out", default=None, metavar="PATH")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: at least three rounds (A/B/A/B pairs)")
    if not torch.cuda.is_available():
        raise SystemExit("train_precision_bench: no HIP device — nothing can be measured here")
    dev = torch.device("cuda:0")
    from unscene3d_amd import _lib
    res = {"command": " ".join(["python", "tools/train_precision_bench.py"] + sys.argv[1:]), "voxels": args.voxels,
           "rounds": args.rounds, "reps": args.reps, "library": _lib.lib.usc_build_info().decode(),
           "device": torch.cuda.get_device_name(0)}
    if not args.skip_units:
        res["units"] = unit_shapes(args, dev)
    if not args.skip_step:
        res["step"] = whole_step(args, dev)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
