"""FreeMask pseudo masks, voxel mode (reference pseudo_masks/freemask_main.py:242-279, :352-417; the full-resolution
lift of :494-508) — the baseline generator whose `{scene}_masks.npy` soft masks datasets/freemask.py reads.

A mask is a threshold on one min-max-normalised cosine row, so nothing of size Q x K is ever stored in f32: two
streaming matrix-core passes (csrc/freemask.hip) give bit-packed masks [Q, ceil(K/64)] with their sizes and maskness
numerators, the extent filter and the greedy mask NMS work on the packed rows, and only the f32 rows of the (at most
`max_instance_num`) survivors are formed at the end.  The sorts, the cuts and the selects between the kernels are torch
operators on Q-sized vectors.

Where this differs from the reference, on purpose:
* ties of the maskness sorts: `torch.argsort` leaves their order unspecified; here both sorts are stable, the lower
  query index comes first;
* when NO mask passes the extent filter the reference goes on with all of them but hands `matrix_nms` the stale,
  unsorted `sum_masks` of line 279; here the NMS always gets the counts that belong to its masks;
* the lift's rounding shift: the reference hard-codes `lr_coords + 2` ("at 1/4 resolution"); here it defaults to
  tensor_stride / 2 (= 2 at scale 4) and can be overridden.

Refused (NotImplementedError, each with its reason): segment mode, `use_fps_sampling`, `similarity_metric="l2"`,
max-fusion of frames.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from .. import ops
from .._lib import check, lib, require_device
from ..ops import _chk, _ptr, _stream, _ws


class CosineMasks(NamedTuple):
    bits: torch.Tensor       # i64[Q, ceil(K/64)]: key k = bit k % 64 of word k / 64 (two's-complement view of the u64 words)
    counts: torch.Tensor     # i32[Q]
    soft_sums: torch.Tensor  # f32[Q]  sum of the soft values inside the mask
    rowmin: torch.Tensor     # f32[Q]  of q^ k^T over all keys
    rowmax: torch.Tensor     # f32[Q]


class SceneMasks(NamedTuple):
    soft_masks: torch.Tensor   # f32[M, K]
    maskness: torch.Tensor     # f32[M]
    query_index: torch.Tensor  # i64[M]
    key_coords: torch.Tensor   # i32[K, 3]
    tensor_stride: int


def _refuse(similarity_metric="cos", segment_ids=None, use_fps_sampling=False, frame_fusion="mean"):
    if segment_ids is not None and len(segment_ids) > 0:
        raise NotImplementedError("FreeMask segment mode is not ported: that branch of the reference opens an interactive "
                                  "viewer (freemask_main.py:210) and cannot run unattended; use voxel mode")
    if use_fps_sampling:
        raise NotImplementedError("use_fps_sampling is not ported: it is pytorch3d farthest-point sampling in feature "
                                  "space and is off in the reference's configuration")
    if similarity_metric != "cos":
        raise NotImplementedError(f"similarity_metric={similarity_metric!r} is not ported: only the cosine similarity "
                                  "('cos', the reference's default) has kernels; 'l2' has none")
    if frame_fusion != "mean":
        raise NotImplementedError(f"frame_fusion={frame_fusion!r} is not ported: the max-fusion of frames "
                                  "(freemask_main.py:116) stays with the caller; encode_scene_feats_2d keeps a running mean")


def _normalize(feats, want_zero):
    n, c = feats.shape
    scale = torch.empty(n, dtype=torch.float32, device=feats.device)
    zero = torch.empty(n, dtype=torch.uint8, device=feats.device) if want_zero else None
    check(lib.usc_freemask_normalize(_ptr(feats), n, c, _ptr(scale), _ptr(zero), _stream()), "usc_freemask_normalize")
    return scale, zero


def _check_feats(key_feats, query_feats):
    require_device()
    _chk(key_feats, torch.float32, "key_feats")
    _chk(query_feats, torch.float32, "query_feats")
    if key_feats.dim() != 2 or query_feats.dim() != 2 or key_feats.shape[1] != query_feats.shape[1]:
        raise RuntimeError("key_feats [K,C] and query_feats [Q,C] must share C")
    if not 1 <= key_feats.shape[1] <= 512:
        raise RuntimeError(f"C = {key_feats.shape[1]} outside [1, 512]")


class _Prepared(NamedTuple):
    sq: torch.Tensor
    sk: torch.Tensor
    zk: torch.Tensor


def _cosine_masks(key_feats, query_feats, threshold):
    _check_feats(key_feats, query_feats)
    (K, C), Q, dev = key_feats.shape, query_feats.shape[0], key_feats.device
    W = (K + 63) // 64
    bits = torch.empty((Q, W), dtype=torch.int64, device=dev)
    counts = torch.empty(Q, dtype=torch.int32, device=dev)
    sums = torch.empty(Q, dtype=torch.float32, device=dev)
    rmin = torch.empty(Q, dtype=torch.float32, device=dev)
    rmax = torch.empty(Q, dtype=torch.float32, device=dev)
    if Q == 0 or K == 0:
        return CosineMasks(bits, counts, sums, rmin, rmax), None
    sk, zk = _normalize(key_feats, True)
    sq, _ = _normalize(query_feats, False)
    nws = lib.usc_freemask_ws_bytes(Q, K)
    ws = _ws(nws, dev)
    st = _stream()
    check(lib.usc_freemask_rowstats(_ptr(query_feats), _ptr(sq), Q, _ptr(key_feats), _ptr(sk), K, C, _ptr(rmin),
                                    _ptr(rmax), _ptr(ws), nws, st), "usc_freemask_rowstats")
    check(lib.usc_freemask_bits(_ptr(query_feats), _ptr(sq), Q, _ptr(key_feats), _ptr(sk), _ptr(zk), K, C, _ptr(rmin),
                                _ptr(rmax), float(threshold), _ptr(bits), _ptr(counts), _ptr(sums), _ptr(ws), nws, st),
          "usc_freemask_bits")
    return CosineMasks(bits, counts, sums, rmin, rmax), _Prepared(sq, sk, zk)


def cosine_masks(key_feats: torch.Tensor, query_feats: torch.Tensor, threshold: float = 0.35) -> CosineMasks:
    """Steps 1-3 of the module docstring's pipeline for every query: packed masks `a >= threshold` of the normalised
    cosine rows, their sizes, the sums of a inside them, and the row statistics of the raw cosine."""
    return _cosine_masks(key_feats, query_feats, threshold)[0]


def soft_rows(key_feats, query_feats, rowmin, rowmax, query_index, _prepared=None) -> torch.Tensor:
    """f32[M, K]: the normalised, key-zeroed cosine rows of the queries `query_index` (same arithmetic as the bits)."""
    _check_feats(key_feats, query_feats)
    (K, C), Q, dev = key_feats.shape, query_feats.shape[0], key_feats.device
    qi = query_index.to(device=dev, dtype=torch.int32).contiguous()
    M = qi.numel()
    out = torch.empty((M, K), dtype=torch.float32, device=dev)
    if M == 0 or K == 0:
        return out
    if M > 4096:
        raise RuntimeError("soft_rows: at most 4096 rows per call")
    if int(qi.min()) < 0 or int(qi.max()) >= Q:
        raise RuntimeError("soft_rows: query_index out of range")
    if _prepared is None:
        sk, zk = _normalize(key_feats, True)
        _prepared = _Prepared(_normalize(query_feats, False)[0], sk, zk)
    check(lib.usc_freemask_soft_rows(_ptr(query_feats), _ptr(_prepared.sq), Q, _ptr(key_feats), _ptr(_prepared.sk),
                                     _ptr(_prepared.zk), K, C, _ptr(rowmin), _ptr(rowmax), _ptr(qi), M, _ptr(out),
                                     _stream()), "usc_freemask_soft_rows")
    return out


def mask_extent(bits: torch.Tensor, key_coords: torch.Tensor):
    """(lo, hi) i32[Q,3]: bounding box of every packed mask over key_coords i32[K,3]; an empty mask has lo > hi."""
    require_device()
    _chk(bits, torch.int64, "bits")
    _chk(key_coords, torch.int32, "key_coords")
    n, K = bits.shape[0], key_coords.shape[0]
    if key_coords.dim() != 2 or key_coords.shape[1] != 3 or bits.shape[1] != (K + 63) // 64:
        raise RuntimeError("mask_extent: bits [n, ceil(K/64)] and key_coords [K,3] do not match")
    lo = torch.empty((n, 3), dtype=torch.int32, device=bits.device)
    hi = torch.empty((n, 3), dtype=torch.int32, device=bits.device)
    if n and K:
        check(lib.usc_mask_bits_extent(_ptr(bits), n, K, _ptr(key_coords), _ptr(lo), _ptr(hi), _stream()),
              "usc_mask_bits_extent")
    return lo, hi


def mask_nms(bits: torch.Tensor, counts: torch.Tensor, order: torch.Tensor, nms_thr: float = 0.5) -> torch.Tensor:
    """Greedy mask NMS (reference matrix_nms(kernel='mask')): `order` lists rows of `bits` by descending score; a
    live mask kills every later live one with `union > 0 ? inter / union > nms_thr : true` (an f32 division of exact
    integers).  -> keep bool[len(order)], by position in `order`."""
    require_device()
    _chk(bits, torch.int64, "bits")
    _chk(counts, torch.int32, "counts")
    order = order.to(device=bits.device, dtype=torch.int32).contiguous()
    n = order.numel()
    keep = torch.empty(n, dtype=torch.uint8, device=bits.device)
    if n == 0:
        return keep.bool()
    if bits.dim() != 2 or counts.numel() != bits.shape[0] or bits.shape[1] == 0:
        raise RuntimeError("mask_nms: bits [rows, W >= 1] and counts [rows] do not match")
    if int(order.min()) < 0 or int(order.max()) >= bits.shape[0]:
        raise RuntimeError("mask_nms: order out of range")
    nws = lib.usc_mask_bits_nms_ws_bytes(n)
    ws = _ws(nws, bits.device)
    check(lib.usc_mask_bits_nms(_ptr(bits), _ptr(counts), bits.shape[1] * 64, _ptr(order), n, float(nms_thr),
                                _ptr(keep), _ptr(ws), nws, _stream()), "usc_mask_bits_nms")
    return keep.bool()


def freemask(key_feats, key_coords, query_feats, scene_extent, *, hard_mask_threshold=0.35, min_mask_points=10,
             instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6,
             similarity_metric="cos", segment_ids=None, use_fps_sampling=False, frame_fusion="mean"):
    """Voxel mode of freemask_main.py:242-417.  key_feats f32[K,C], key_coords int[K,3] (or [K,4]: b,x,y,z),
    query_feats f32[Q,C], scene_extent [3] (max - min of the scene's voxel coordinates).
    -> (soft_masks f32[M,K], maskness f32[M], query_index i64[M]) in the reference's output order; three empty
    tensors where the reference prints "No instances detected" / "No candidates left" and skips the scene."""
    _refuse(similarity_metric, segment_ids, use_fps_sampling, frame_fusion)
    dev = key_feats.device
    K = key_feats.shape[0]
    empty = (torch.zeros((0, K), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
             torch.zeros(0, dtype=torch.int64, device=dev))
    cm, prep = _cosine_masks(key_feats, query_feats, hard_mask_threshold)
    cand = torch.nonzero(cm.counts > min_mask_points).flatten()                    # :271, ascending query index
    if cand.numel() == 0:
        return empty
    maskness = cm.soft_sums[cand] / cm.counts[cand]                                # :353 (f32 / integer)
    maskness, by = torch.sort(maskness, descending=True, stable=True)              # :354, ties: lower query first
    cand = cand[by]
    # extent filter (:375-395), x and y only, in f64 like numpy's int / int division
    coords = key_coords[:, -3:].to(device=dev, dtype=torch.int32).contiguous()
    lo, hi = mask_extent(cm.bits, coords)
    ext = (hi[cand, :2].long() - lo[cand, :2].long()).double()
    scene = torch.as_tensor(scene_extent, device=dev).double().flatten()[:2]
    ok = ~((ext / scene) > instance_to_scene_max_ratio).any(1)
    if bool(ok.any()):
        cand, maskness = cand[ok], maskness[ok]
    keep = mask_nms(cm.bits, cm.counts, cand, nms_thr)                             # :398
    maskness = torch.where(keep, maskness, torch.zeros_like(maskness))
    maskness, by = torch.sort(maskness, descending=True, stable=True)              # :400-403
    by = by[:max_instance_num]
    maskness, cand = maskness[:max_instance_num], cand[by]
    sel = maskness > nms_maskness_threshold                                        # :412
    if not bool(sel.any()):
        return empty
    maskness, cand = maskness[sel], cand[sel]
    return soft_rows(key_feats, query_feats, cm.rowmin, cm.rowmax, cand, prep), maskness, cand


def _pool_steps(resolution_scale):
    steps = int(math.log2(resolution_scale))
    if resolution_scale < 1 or 2 ** steps != resolution_scale:
        raise ValueError(f"resolution_scale must be a power of two, got {resolution_scale}")
    return steps


def _scene_extent(coords):
    c = coords[:, -3:]
    return (c.amax(0) - c.amin(0)).float()


def _from_keys(keys, steps, extent, kw):
    from .. import MinkowskiEngine as ME
    pool = ME.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=3)
    queries = keys
    for _ in range(steps):                                                         # :173-183
        queries = pool(queries)
    kf, qf = keys.F.detach().float().contiguous(), queries.F.detach().float().contiguous()
    kc = keys.C[:, 1:].contiguous()
    soft, maskness, qi = freemask(kf, kc, qf, extent, **kw)
    return SceneMasks(soft, maskness, qi, kc, keys.tensor_stride[0])


def freemask_scene(model, sinput, resolution_scale=2, **kw) -> SceneMasks:
    """3D branch (:98-101, :171-183): keys = the backbone's `res_{scale}` feature map, queries = the keys
    average-pooled log2(scale) more times."""
    _refuse(kw.get("similarity_metric", "cos"), kw.get("segment_ids"), kw.get("use_fps_sampling", False),
            kw.get("frame_fusion", "mean"))
    steps = _pool_steps(resolution_scale)
    with torch.no_grad():
        _, feature_maps = model(sinput)
        return _from_keys(feature_maps[f"res_{resolution_scale}"], steps, _scene_extent(sinput.C), kw)


def freemask_from_voxel_feats(coords, feats, resolution_scale=2, **kw) -> SceneMasks:
    """Image branch (:162-179): per-voxel features (e.g. encode_scene_feats_2d's) on the unique voxel coordinates
    `coords` int[N,3] or [N,4] are average-pooled log2(scale) times to the keys, and as often again to the queries."""
    from .. import MinkowskiEngine as ME
    _refuse(kw.get("similarity_metric", "cos"), kw.get("segment_ids"), kw.get("use_fps_sampling", False),
            kw.get("frame_fusion", "mean"))
    steps = _pool_steps(resolution_scale)
    require_device()
    coords = coords.to(torch.int32)
    if coords.shape[1] == 3:
        coords = torch.cat([torch.zeros_like(coords[:, :1]), coords], 1)
    with torch.no_grad():
        keys = ME.SparseTensor(features=feats.float().contiguous(), coordinates=coords.contiguous(), device=feats.device)
        pool = ME.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=3)
        for _ in range(steps):
            keys = pool(keys)
        return _from_keys(keys, steps, _scene_extent(coords), kw)


def freemask_scene_fn(scene, **kw) -> SceneMasks:
    """`scene_fn` of PseudoMaskDriver: scene = dict with `coords`, `feats` and optionally `resolution_scale`."""
    return freemask_from_voxel_feats(scene["coords"], scene["feats"], scene.get("resolution_scale", 2), **kw)


def soft_masks_to_full_resolution(key_coords, tensor_stride, full_res_coords, voxel_size, soft_masks,
                                  rounding_shift=None) -> np.ndarray:
    """The save-time lift (:494-505): every full-resolution point takes the soft-mask row of its nearest key voxel
    (exact 1-NN on the device against `key_coords + rounding_shift`, in voxel units).  rounding_shift defaults to
    tensor_stride / 2, the centre of a key's cell (the reference hard-codes 2, its value at scale 4).
    -> f32[N_full, M]."""
    dev = soft_masks.device
    shift = tensor_stride / 2 if rounding_shift is None else rounding_shift
    ref = (key_coords[:, -3:].to(device=dev, dtype=torch.float32) + float(shift)).contiguous()
    query = torch.as_tensor(np.asarray(full_res_coords) / voxel_size, dtype=torch.float32, device=dev).contiguous()
    _, match = ops.knn1(query, ref)
    return soft_masks.t()[match].contiguous().cpu().numpy()
