"""Feeders of the NCut core on the pseudo-mask path (reference pseudo_masks/unscene3d_pseudo_main.py):
the 3D branch of `encode_scene_feats` (:332-348: CSC features of a coarser level carried to the input
voxels by exact 1-NN) and the save-time lift of segment masks to the full-resolution cloud (:649-667).
Both 1-NN searches run on the device (usc_knn1) instead of scipy's KD-tree.  The image branch of
`encode_scene_feats` (:287-330) projects per-frame 2D features onto the voxels and keeps a running mean."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..precision import inference_precision


def encode_scene_feats_3d(model, sinput, resolution_scale=2, precision="f32", nn="brute"):
    """Res16UNet34CMultiRes features of level `res_{resolution_scale}` for every input voxel.  precision: the trunk's
    convolutions in "f32" or "bf16" (unscene3d_amd.inference_precision).
    nn: the 1-NN search that carries the coarse rows to the input voxels — "brute" (ops.knn1, every pair) or "grid"
    (ops.knn1_grid with cells of the coarse level's tensor stride, one coarse voxel per cell; the box comes from one
    aminmax of the coarse coordinates).  Both return the same rows."""
    if nn not in ("brute", "grid"):
        raise ValueError(f"nn must be 'brute' or 'grid', got {nn!r}")
    with torch.no_grad(), inference_precision(precision):
        _, feature_maps = model(sinput)
        enc = feature_maps[f"res_{resolution_scale}"]
        lr_coords = enc.C[:, 1:].float().contiguous()
        hr_coords = sinput.C[:, 1:].float().contiguous()
        if nn == "grid":
            lo, hi = torch.aminmax(enc.C[:, 1:], dim=0)
            lo, hi = torch.stack([lo, hi]).cpu().numpy()
            _, match = ops.knn1_grid(hr_coords, lr_coords, cell=float(enc.tensor_stride[0]), bounds=(lo, hi))
        else:
            _, match = ops.knn1(hr_coords, lr_coords)
        return enc.F[match].detach()


def encode_scene_feats_2d(model, images, camera_poses, color_intrinsics, coords, projecter, attention=False,
                          frame_batch=None):
    """Image branch of `encode_scene_feats` (unscene3d_pseudo_main.py:287-330).

    model(img[1,1,c,h,w]) -> (key_features, query_features), each [1,1,H,W,C] (the 2D backbone is the caller's, e.g.
    models.encoders_2d.DinoNet);
    images [1,n_frames,c,h,w], camera_poses [1,n_frames,4,4], color_intrinsics [1,4]; coords int[n,4];
    projecter: `Project2DFeaturesCUDA`.  One ray cast per frame serves both feature maps; every frame's features
    are reduced per voxel and folded into the running mean in one kernel (`fuse_frame`).
    frame_batch=k (an integer >= 1): the frames go, in order, in groups of k through `model.forward_tokens` and
    `projecter.fuse_frames_tokens` — one encoder pass, one ray cast and one projection kernel per group, and the
    resized [H,W,C] maps are never written; the model must have `forward_tokens` (DinoNet has).  The running mean folds
    the same frames in the same order; the bilinear samples round differently from torch's resize.
    -> scene_key_feats (and scene_query_feats when `attention`), f32[n,C]."""
    n = coords.shape[0]
    scene_key = scene_query = None
    if frame_batch is not None:
        k = int(frame_batch)
        if k < 1:
            raise ValueError(f"frame_batch must be None or an integer >= 1, got {frame_batch!r}")
        if not hasattr(model, "forward_tokens"):
            raise RuntimeError("encode_scene_feats_2d(frame_batch=k) needs a model with forward_tokens "
                               "(models.encoders_2d.DinoNet); frame_batch=None takes any model")
        for i in range(0, images.shape[1], k):
            key_tokens, query_tokens = model.forward_tokens(images[:, i:i + k])
            if scene_key is None:
                C = key_tokens.shape[-1]
                scene_key = torch.zeros((n, C), dtype=torch.float32, device=coords.device)
                scene_query = torch.zeros_like(scene_key) if attention else None
            views = camera_poses[:1, i:i + k]
            _, cast = projecter.fuse_frames_tokens(scene_key, key_tokens, coords, views, color_intrinsics)
            if attention:
                projecter.fuse_frames_tokens(scene_query, query_tokens, coords, views, color_intrinsics, hit_seg=cast)
        return (scene_key, scene_query) if attention else scene_key
    with torch.no_grad():
        for i, img in enumerate(images[0]):
            key_features, query_features = model(img.unsqueeze(0).unsqueeze(0))
            if scene_key is None:
                C = key_features.shape[-1]
                scene_key = torch.zeros((n, C), dtype=torch.float32, device=coords.device)
                scene_query = torch.zeros_like(scene_key) if attention else None
            view = camera_poses[0, i].unsqueeze(0).unsqueeze(0)
            _, cast = projecter.fuse_frame(scene_key, key_features, coords, view, color_intrinsics)
            if attention:
                projecter.fuse_frame(scene_query, query_features, coords, view, color_intrinsics, hit_seg=cast)
    return (scene_key, scene_query) if attention else scene_key


def masks_to_full_resolution(voxel_coords: torch.Tensor, full_res_coords, voxel_size: float, segment_ids, bipartitions):
    """Per-voxel segment ids / masks -> full-resolution points by 1-NN against voxel centres (+0.5)."""
    dev = voxel_coords.device
    ref = (voxel_coords[:, -3:].float() + 0.5).contiguous()
    query = torch.as_tensor(np.asarray(full_res_coords) / voxel_size, dtype=torch.float32, device=dev).contiguous()
    _, match = ops.knn1(query, ref)
    match = match.cpu().numpy()
    return np.asarray(segment_ids)[match], np.asarray(bipartitions)[match]
