#!/usr/bin/env python
"""Scan directories -> the scene files tools/pseudo_masks_run.py reads: for every `SCANS/{scene}/` (info file, mesh,
color/, pose/ — the layout unscene3d_amd/pseudo_masks/scans.py documents, ScanNet's) voxelise the mesh, over-segment it,
run the colour frames through the DINO ViT-S/8 encoder and project them onto the voxels
(scans.build_scene; reference pseudo_masks/datasets/scannet.py + unscene3d_pseudo_main.py:287-330), and write
`OUT/{scene}.npz`.  Scenes whose file exists are skipped.

Replicas only, like pseudo_masks_run.py: rank r of W takes the scenes r, r+W, ...

    python tools/scene_files_from_scans.py --scans SCANS --out SCENES --dino-weights dino_deitsmall8_pretrain.pth
    python -m torch.distributed.run --nproc-per-node 8 tools/scene_files_from_scans.py --scans SCANS --out SCENES ...
    python tools/pseudo_masks_run.py --scenes SCENES --out MASKS
    python tools/scene_files_from_scans.py --scans SCANS --out SCENES --dino-weights DINO.pth --csc-weights CSC.pth
    python tools/scene_files_from_scans.py --scans SCANS --out SCENES --no-images --csc-weights CSC.pth
    python tools/scene_files_from_scans.py --scans SCANS --out SCENES --layout arkit --csc-weights CSC.pth
    python tools/scene_files_from_scans.py --scans SCANS --out SCENES --layout points --csc-weights CSC.pth --graph-k 8 --graph-radius 0.1

--dino-weights is the published DINO ViT-S/8 checkpoint (a state_dict; not part of this repository);
--random-weights SEED initialises the encoder from a seed instead (smoke runs and benchmarks: the features mean nothing).
--frame-batch K sends K frames per encoder pass and projection launch (pipeline.encode_scene_feats_2d); 0 is the
per-frame path through the resized feature maps.  The default is what profiles/scene_encode_bench.txt measured fastest.
--csc-weights is the published CSC Res16UNet34C checkpoint (`{"state_dict": ...}`; models.weights.load_csc_backbone):
with it, or with --csc-random-weights SEED, the voxels also go through the 3D backbone and the file gets `feats_3d`, the
features of level res_{--resolution-scale} (reference unscene3d_pseudo_main.py:332-348; `modality: both`).  --no-images
reads no frame and writes the geometry modality alone (`modality: geom`); the image encoder's weights are not needed then.
--layout arkit reads mesh-only scans (`SCANS/{scene}/{scene}_3dod_mesh.ply`, ARKitScenes' naming, or a flat
`SCANS/{scene}.ply`; scans.load_mesh_only_scan, reference pseudo_masks/datasets/arkit.py): the mesh is cleaned,
over-segmented at every size of --segments-min-verts (default 50 100 150 200), small segments are removed and the rest is
shifted to the origin; the file is geometry-only and holds the segments of level --segment-dimension-order.
--layout points reads coloured point clouds without a mesh (`SCANS/{scene}/{scene}.ply` or a flat `SCANS/{scene}.ply`, a
vertex element with x y z red green blue and optionally nx ny nz; scans.load_point_cloud_scan): the cloud is
over-segmented on its k-NN graph (--graph-k neighbours inside --graph-radius metres; unmeasured starting values, DESIGN.md
§3.30) at every size of --segments-min-verts (default 50), --small-segments says what becomes of segments the graph left
small or unconnected, and the file is geometry-only as for arkit."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DINO_LAYER, DINO_STRIDE = 10, 4   # pseudo_masks/config/default.yaml:53-54
DEFAULT_FRAME_BATCH = 16      # profiles/scene_encode_bench.txt: 0.162 s per 64-frame scene (8: 0.175, per-frame maps: 0.364)


def make_encoder(args, device):
    from types import SimpleNamespace

    from unscene3d_amd.models.encoders_2d import DinoNet
    from unscene3d_amd.models.encoders_2d.dino import init_random_weights

    feature = "attention" if args.attention else "descriptors"
    cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_feature=feature,
                                                     dino_vit_layer=DINO_LAYER, dino_vit_stride=DINO_STRIDE))
    net = DinoNet(cfg, precision=args.precision)
    if args.dino_weights:
        net.vit.load_state_dict(torch.load(args.dino_weights, map_location="cpu"), strict=True)
    else:
        init_random_weights(net.vit, args.random_weights)
    return net.to(device).eval()


def make_backbone_3d(args, device):
    """The 3D feature extractor, or None without --csc-weights / --csc-random-weights."""
    from unscene3d_amd.models.weights import load_csc_backbone

    if args.csc_weights:
        return load_csc_backbone(args.csc_weights, device=device)
    if args.csc_random_weights is None:
        return None
    torch.manual_seed(args.csc_random_weights)
    return load_csc_backbone({}, device=device)


def process_scan(scan_dir, out_dir, model, args, model_3d=None):
    """-> (scene name, voxels, frames used, frames dropped, seconds) or None when the scene file exists."""
    from unscene3d_amd.pseudo_masks import scans

    name = scans.mesh_only_scan_path(scan_dir)[0] if args.layout != "scannet" else os.path.basename(os.path.normpath(scan_dir))
    path = os.path.join(out_dir, f"{name}.npz")
    if os.path.exists(path):
        return None
    t0 = time.perf_counter()
    scene = scans.build_scene(scan_dir, model, voxel_size=args.voxel_size, image_hw=(args.height, args.width),
                              segments_min_verts=args.segments_min_verts, frame_batch=args.frame_batch or None,
                              layout=args.layout, segment_dimension_order=args.segment_dimension_order,
                              attention=args.attention, every=args.every,
                              device=next((model_3d if model is None else model).parameters()).device, model_3d=model_3d,
                              resolution_scale=args.resolution_scale, precision_3d=args.precision_3d,
                              images=not args.no_images and args.layout == "scannet", graph_k=args.graph_k,
                              graph_radius=args.graph_radius, small_segments=args.small_segments)
    os.makedirs(out_dir, exist_ok=True)
    tmp = path + ".tmp.npz"
    np.savez(tmp, **scene)
    os.replace(tmp, path)                                           # a killed run leaves no half-written scene file
    return (name, scene["coords"].shape[0], scene.get("frames_used", 0), scene.get("frames_dropped", 0),
            time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", required=True, help="directory with one sub-directory per scan")
    ap.add_argument("--out", required=True, help="directory for the .npz scene files")
    w = ap.add_mutually_exclusive_group()
    w.add_argument("--dino-weights", help="state_dict file of DINO ViT-S/8")
    w.add_argument("--random-weights", type=int, metavar="SEED")
    w3 = ap.add_mutually_exclusive_group()
    w3.add_argument("--csc-weights", metavar="FILE", help="checkpoint of the CSC Res16UNet34C: also write feats_3d")
    w3.add_argument("--csc-random-weights", type=int, metavar="SEED")
    ap.add_argument("--resolution-scale", type=int, default=2, choices=(1, 2, 4, 8, 16),
                    help="level of the 3D backbone whose features become feats_3d")
    ap.add_argument("--precision-3d", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--no-images", action="store_true", help="read no frame: a geometry-only scene file")
    ap.add_argument("--frame-batch", type=int, default=DEFAULT_FRAME_BATCH, metavar="K",
                    help="frames per encoder pass and projection launch; 0 = the per-frame map path")
    ap.add_argument("--every", type=int, default=1, metavar="K", help="use every K-th frame")
    ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--attention", action="store_true", help="key and query of the last block (feats_2d_query too)")
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--segments-min-verts", type=int, nargs="+", default=None, metavar="N",
                    help="smallest segment of the over-segmentation: one number (default 50); --layout arkit / points: "
                         "one per level (default 50 100 150 200 / 50)")
    ap.add_argument("--layout", choices=("scannet", "arkit", "points"), default="scannet",
                    help="arkit: mesh-only scans; points: point clouds without a mesh; both give geometry-only scene files")
    ap.add_argument("--segment-dimension-order", type=int, default=0, metavar="L",
                    help="--layout arkit / points: the level of --segments-min-verts whose segments are written")
    ap.add_argument("--graph-k", type=int, default=8, metavar="K", help="--layout points: neighbours per point of the graph")
    ap.add_argument("--graph-radius", type=float, default=0.1, metavar="R",
                    help="--layout points: neighbours lie strictly inside this radius")
    ap.add_argument("--small-segments", choices=("merge", "drop", "keep"), default="merge",
                    help="--layout points: small or unconnected segments join the nearest kept one, lose their points, or stay")
    args = ap.parse_args(argv)
    if args.frame_batch < 0 or args.every < 1:
        ap.error("--frame-batch needs K >= 0 and --every K >= 1")
    if args.layout != "scannet":
        args.no_images = True
    elif args.segments_min_verts is not None:
        if len(args.segments_min_verts) != 1:
            ap.error("--segments-min-verts takes one number unless --layout arkit or points is given")
        args.segments_min_verts = args.segments_min_verts[0]
    has_2d = args.dino_weights is not None or args.random_weights is not None
    has_3d = args.csc_weights is not None or args.csc_random_weights is not None
    if args.no_images and not has_3d:
        ap.error("--no-images needs --csc-weights or --csc-random-weights")
    if not args.no_images and not has_2d:
        ap.error("one of the arguments --dino-weights --random-weights is required (or --no-images)")
    from unscene3d_amd.pseudo_masks.driver import scene_shard

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if args.layout != "scannet":
        from unscene3d_amd.pseudo_masks.scans import mesh_only_scans
        dirs = mesh_only_scans(args.scans)                          # the point-cloud layout lists its scans the same way
    else:
        dirs = sorted(d for d in (os.path.join(args.scans, e) for e in os.listdir(args.scans)) if os.path.isdir(d))
    mine = scene_shard(len(dirs), rank, world)
    model = make_encoder(args, device) if has_2d and not args.no_images else None
    model_3d = make_backbone_3d(args, device)
    done = 0
    for i in mine:
        r = process_scan(dirs[i], args.out, model, args, model_3d)
        if r is None:
            print(f"[rank {rank}] scene file exists: {os.path.basename(dirs[i])}", flush=True)
        else:
            done += 1
            print(f"[rank {rank}] {r[0]}: {r[1]} voxels, {r[2]} frames ({r[3]} dropped) in {r[4]:.2f} s", flush=True)
    print(f"[rank {rank}/{world}] {done} of {len(mine)} scans of this shard written ({len(dirs)} in the list)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
