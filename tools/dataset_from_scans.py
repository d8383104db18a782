#!/usr/bin/env python
"""Scan directories + pseudo-mask files -> the dataset tools/train.py --data-dir reads
(unscene3d_amd/datasets/preprocessing.py; reference datasets/preprocessing/freemask_preprocessing.py).

    python tools/dataset_from_scans.py --scans SCANS --pseudo MASKS --out DATA
    python tools/dataset_from_scans.py --scans SCANS --pseudo MASKS --out DATA --train scannetv2_train.txt --val scannetv2_val.txt
    python tools/dataset_from_scans.py --scans SCANS --pseudo MASKS --out DATA --layout arkit
    python tools/dataset_from_scans.py --scans SCANS --pseudo MASKS --out DATA --layout points --write-connectivity
    python tools/train.py --data-dir DATA --steps 100 --out RUN

SCANS holds one directory per scan (`scene0000_00/`: info file, mesh, and — for ground truth — labels PLY, segs.json,
aggregation.json); MASKS is the output directory of tools/pseudo_masks_run.py.  --train / --val are text files with one
scan name per line (ScanNet's split files); without them every directory of SCANS goes into the train split.  A scan
without pseudo-mask files is skipped with a message.  --oracle writes one-hot ground-truth masks instead of pseudo masks.
--layout arkit: SCANS holds mesh-only scans (`{scene}/{scene}_3dod_mesh.ply` or `{scene}.ply`) and MASKS was made from
their `scene_files_from_scans.py --layout arkit` scene files with the same --segments-min-verts; normals are estimated
from the points on the device (preprocessing.build_mesh_only_tables).
--layout points: SCANS holds point clouds without a mesh (`{scene}/{scene}.ply` or `{scene}.ply`) and MASKS was made from
their `scene_files_from_scans.py --layout points` scene files with the same --segments-min-verts, --graph-k, --graph-radius
and --small-segments; normals are the file's nx ny nz when it has them, else estimated
(preprocessing.build_point_cloud_tables).
Prints one JSON line: scans written per mode."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", required=True, help="directory with one sub-directory per scan")
    ap.add_argument("--pseudo", default=None, help="directory with {scene}_cloud.npy / {scene}_masks.npy")
    ap.add_argument("--out", required=True, help="dataset directory")
    ap.add_argument("--train", default=None, metavar="FILE", help="scan names of the train split")
    ap.add_argument("--val", default=None, metavar="FILE", help="scan names of the validation split")
    ap.add_argument("--oracle", action="store_true", help="one-hot ground-truth masks instead of pseudo masks")
    ap.add_argument("--segments-min-verts", type=int, nargs="+", default=None, metavar="N",
                    help="over-segmentation when a scan has no segs.json (default 20); --layout arkit / points: one "
                         "number per level (default 50 100 150 200 / 50)")
    ap.add_argument("--layout", choices=("scannet", "arkit", "points"), default="scannet")
    ap.add_argument("--segment-dimension-order", type=int, default=0, metavar="L",
                    help="--layout arkit / points: the level whose segment ids are written")
    ap.add_argument("--graph-k", type=int, default=8, metavar="K", help="--layout points: neighbours per point of the graph")
    ap.add_argument("--graph-radius", type=float, default=0.1, metavar="R",
                    help="--layout points: neighbours lie strictly inside this radius")
    ap.add_argument("--small-segments", choices=("merge", "drop", "keep"), default="merge",
                    help="--layout points: what becomes of small or unconnected segments")
    ap.add_argument("--write-connectivity", action="store_true",
                    help="also store the over-segmentation's segment pairs ({scene}_connectivity.npy) for the export "
                         "step's general.separate_instances")
    args = ap.parse_args(argv)
    if not args.oracle and args.pseudo is None:
        ap.error("--pseudo is needed unless --oracle is given")
    arkit = args.layout != "scannet"                  # frame-less scans without ground truth: arkit and points
    if arkit and args.oracle:
        ap.error(f"--oracle needs ground truth, which --layout {args.layout} has not")
    if not arkit and args.segments_min_verts is not None:
        if len(args.segments_min_verts) != 1:
            ap.error("--segments-min-verts takes one number unless --layout arkit or points is given")
        args.segments_min_verts = args.segments_min_verts[0]

    import torch

    from unscene3d_amd.datasets.preprocessing import build_dataset

    splits = {}
    if args.train:
        splits["train"] = args.train
    if args.val:
        splits["validation"] = args.val
    if not splits and arkit:
        from unscene3d_amd.pseudo_masks.scans import mesh_only_scan_path, mesh_only_scans
        splits["train"] = [mesh_only_scan_path(p)[0] for p in mesh_only_scans(args.scans)]
    elif not splits:
        splits["train"] = sorted(e for e in os.listdir(args.scans) if os.path.isdir(os.path.join(args.scans, e)))
    device = torch.device("cuda", torch.cuda.current_device())
    databases = build_dataset(args.scans, splits, args.pseudo, args.out, oracle=args.oracle, device=device,
                              segments_min_verts=args.segments_min_verts, write_connectivity=args.write_connectivity,
                              layout=args.layout, segment_dimension_order=args.segment_dimension_order,
                              graph_k=args.graph_k, graph_radius=args.graph_radius, small_segments=args.small_segments)
    print(json.dumps({"out": args.out, "scans": {mode: len(db) for mode, db in databases.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
