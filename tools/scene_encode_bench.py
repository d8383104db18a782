#!/usr/bin/env python
"""Seconds per scene and peak memory of the image branch of the pseudo-mask generator
(unscene3d_amd.pseudo_masks.pipeline.encode_scene_feats_2d: DINO ViT-S/8 encoder -> ray cast -> per-voxel running mean)
for the per-frame path through the resized feature maps (`frame_batch=None`) and for token grids projected in groups of
1 / 4 / 8 / 16 frames (`frame_batch=k`: DinoNet.forward_tokens + Project2DFeaturesCUDA.fuse_frames_tokens).

    python tools/scene_encode_bench.py                          # 64 frames of 192 x 256 on a ~130 k-voxel room, f32
    python tools/scene_encode_bench.py --precision bf16 --frames 128

Scene: synthetic.room_voxels scaled up (a closed room, `--dims` voxels, boxes inside), cameras of synthetic.camera_views
inside it, normal-random images, a DinoNet with N(0, 0.02) weights (the encoder's time does not depend on the weights).
One call = one whole scene, timed with a host clock around the call and a device synchronise at both ends.  Every
setting is warmed up with one untimed scene; then `--rounds` rounds run every setting once, in turn, so that drift of
the shared host hits all settings alike.  Peak memory is torch's allocated peak above what is resident before the call
(model, images, coordinates).  The last column compares each setting's features with `frame_batch=None`'s.
The tool sets no threshold: it is a measurement."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--dims", default="150,170,130", help="room size in voxels")
    ap.add_argument("--batches", default="none,1,4,8,16", help="frame_batch settings, 'none' = the per-frame map path")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--layer", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("scene_encode_bench: no HIP device; nothing is measured without one")
    from types import SimpleNamespace

    from unscene3d_amd.models.encoders_2d import DinoNet
    from unscene3d_amd.models.encoders_2d.dino import init_random_weights
    from unscene3d_amd.project_features_cuda import Project2DFeaturesCUDA
    from unscene3d_amd.pseudo_masks.pipeline import encode_scene_feats_2d
    from unscene3d_amd.synthetic import camera_views, room_voxels

    dev = torch.device("cuda:0")
    dims = tuple(int(v) for v in args.dims.split(","))
    H, W = args.height, args.width
    coords_np = room_voxels(5, dims=dims, n_boxes=30)
    views = camera_views(6, coords_np, args.frames, dims=dims)
    coords = torch.from_numpy(coords_np).to(dev)
    poses = torch.from_numpy(views).to(dev)
    intr = torch.tensor([[W * 0.9, W * 0.9, (W - 1) / 2, (H - 1) / 2]], dtype=torch.float32, device=dev)
    images = torch.randn((1, args.frames, 3, H, W), generator=torch.Generator().manual_seed(0)).to(dev)
    cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_feature="descriptors",
                                                     dino_vit_layer=args.layer, dino_vit_stride=4))
    model = DinoNet(cfg, precision=args.precision)
    init_random_weights(model.vit, 0)
    model = model.to(dev).eval()
    projecter = Project2DFeaturesCUDA(width=W, height=H, voxel_size=0.02)
    settings = [None if b == "none" else int(b) for b in args.batches.split(",")]

    def scene(batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = encode_scene_feats_2d(model, images, poses, intr, coords, projecter, frame_batch=batch)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    print(f"device: {torch.cuda.get_device_name(0)}; {coords.shape[0]} voxels (room {args.dims}), {args.frames} frames of "
          f"{H}x{W}, encoder {args.precision}, key of block {args.layer}; 1 warm-up scene per setting, {args.rounds} "
          f"rounds over all settings in turn")
    peak, feats = {}, {}
    for b in settings:                                              # warm-up, peak memory, features
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out, _ = scene(b)
        peak[b] = torch.cuda.max_memory_allocated() - base
        feats[b] = out.cpu()
        del out
    times = {b: [] for b in settings}
    for _ in range(args.rounds):
        for b in settings:
            times[b].append(scene(b)[1])
    ref = feats.get(None)
    seen = int((feats[settings[0]].abs().sum(1) > 0).sum())
    print(f"voxels seen by a frame: {seen} of {coords.shape[0]}")
    for b in settings:
        t = times[b]
        med = statistics.median(t)
        line = (f"frame_batch={str(b):>4s}: median {med:7.3f} s/scene (min {min(t):.3f}, max {max(t):.3f}) = "
                f"{1e3 * med / args.frames:6.2f} ms/frame, peak extra memory {peak[b] / 2**20:8.1f} MiB")
        if ref is not None and b is not None:
            line += (f", max |features - frame_batch=None| {float((feats[b] - ref).abs().max()):.3e} "
                     f"(max |feature| {float(ref.abs().max()):.3f})")
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
