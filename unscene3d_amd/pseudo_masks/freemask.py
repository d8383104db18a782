"""FreeMask pseudo masks, voxel mode (reference pseudo_masks/freemask_main.py:242-279, :352-417; the full-resolution
lift of :494-508) — the baseline generator whose `{scene}_masks.npy` soft masks datasets/freemask.py reads.

A mask is a threshold on one min-max-normalised cosine row, so nothing of size Q x K is ever stored in f32: two
streaming matrix-core passes (csrc/freemask.hip) give bit-packed masks [Q, ceil(K/64)] with their sizes and maskness
numerators, the extent filter and the greedy mask NMS work on the packed rows, and only the f32 rows of the (at most
`max_instance_num`) survivors are formed at the end.  The sorts, the cuts and the selects between the kernels are torch
operators on Q-sized vectors: `_select`, the one selection tail of both modes (stable sort by maskness, x/y extent
filter, greedy NMS, stable sort, the two cuts); a mode hands it its candidates' rows, boxes and NMS.

Where this differs from the reference, on purpose:
* ties of the maskness sorts: `torch.argsort` leaves their order unspecified; here both sorts are stable, the lower
  query index comes first;
* when NO mask passes the extent filter the reference goes on with all of them but hands `matrix_nms` the stale,
  unsorted `sum_masks` of line 279; here the NMS always gets the counts that belong to its masks (`_select` hands its
  NMS row indices, never counts);
* the lift's rounding shift: the reference hard-codes `lr_coords + 2` ("at 1/4 resolution"); here it defaults to
  tensor_stride / 2 (= 2 at scale 4) and can be overridden.

Refused (NotImplementedError, each with its reason): `segment_ids=` on the voxel-mode functions,
`use_fps_sampling`, `similarity_metric="l2"`, max-fusion of frames.

Segment mode (the `segment_ids != []` branch: :186-233, :282-350, :359-370) has its own entry points,
`freemask_segments*`.  Keys and queries are the S segment features (mean of the not-all-zero key rows of a segment;
all-zero segments dropped), a query's mask is split into its connected parts on the segment adjacency, and the parts are
remapped to key voxels before the extent filter and the NMS.  A mask is a union of whole segments, so its voxel count,
its box and the voxel intersection of two masks are exact functions of the S-bit row and of the per-segment tables
`w[s]` (key voxels) and `lo[s]`, `hi[s]` (their box): everything up to the survivors' rows works on rows
[R, ceil(S/64)] (csrc/freemask_segments.hip), next to one f32 [candidates, S] soft matrix and its i32 labels.
Further deviations there, on purpose:
* (d) parts are the true connected components of the UNDIRECTED adjacency: a pair (a, b) of `seg_connectivity` joins a
  and b both ways; self pairs and pairs naming a dropped or unknown segment are ignored.  The reference's scan looks only
  at the out-neighbours of the segment it inserts (a one-directional pair joins or not depending on id order) and skips
  the blob that slides into a popped blob's place (`pop(fused_id)`, then `fused_id += 1`), so a segment bridging three
  blobs can leave two connected blobs apart.  The rows of one query are ordered by their part's smallest segment index;
  the reference's blob order matters only for exact maskness ties;
* (e) the NMS always gets the voxel counts of its own rows (the voxel-mode deviation above, kept by the same
  `_select`; here the stale counts would even be segment counts);
* (f) the viewer call (:210), the `.ply` dump and the PCA colouring are not ported;
* (g) the segment column of `_cloud.npy` is not reproduced (the reference indexes input-voxel ids with key-voxel
  matches, :506).
The reference pools the ids as f32; here they are pooled as integers and ids outside [0, 2^24) are refused.
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


def _refuse(similarity_metric="cos", segment_ids=None, use_fps_sampling=False, frame_fusion="mean", **_):
    """The refused keywords of either mode, by name: `_refuse(**kw)` reads them from a scene function's keywords."""
    if segment_ids is not None and len(segment_ids) > 0:
        raise NotImplementedError("segment_ids= is not taken here: that branch of the reference opens an interactive "
                                  "viewer (freemask_main.py:210) in the middle of the computation; segment mode runs "
                                  "unattended through freemask_segments / freemask_segments_scene / "
                                  "freemask_segments_from_voxel_feats / freemask_segments_scene_fn")
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


def mask_nms(bits: torch.Tensor, counts: torch.Tensor, order: torch.Tensor, nms_thr: float = 0.5,
             weight=None) -> torch.Tensor:
    """Greedy mask NMS (reference matrix_nms(kernel='mask')): `order` lists rows of `bits` by descending score; a
    live mask kills every later live one with `union > 0 ? inter / union > nms_thr : true` (an f32 division of exact
    integers).  -> keep bool[len(order)], by position in `order`.
    With `weight` i32[S], one per bit: inter = sum of weight over the AND of two rows, `counts` the rows' weighted
    sizes.  Exact while sum(weight) < 2^24 (checked)."""
    require_device()
    _chk(bits, torch.int64, "bits")
    _chk(counts, torch.int32, "counts")
    if weight is not None:
        _chk(weight, torch.int32, "weight")
    order = order.to(device=bits.device, dtype=torch.int32).contiguous()
    n = order.numel()
    keep = torch.empty(n, dtype=torch.uint8, device=bits.device)
    if n == 0:
        return keep.bool()
    if bits.dim() != 2 or counts.numel() != bits.shape[0] or bits.shape[1] == 0 or (
            weight is not None and bits.shape[1] != (weight.numel() + 63) // 64):
        raise RuntimeError("mask_nms: bits [rows, W >= 1], counts [rows] and weight [S], W = ceil(S/64), do not match")
    if int(order.min()) < 0 or int(order.max()) >= bits.shape[0]:
        raise RuntimeError("mask_nms: order out of range")
    if weight is not None and (int(weight.min()) < 0 or int(weight.long().sum()) >= 1 << 24):
        raise RuntimeError("mask_nms: weights must be >= 0 and sum to less than 2^24")
    nws = lib.usc_mask_bits_nms_ws_bytes(n)
    ws = _ws(nws, bits.device)
    if weight is None:
        check(lib.usc_mask_bits_nms(_ptr(bits), _ptr(counts), bits.shape[1] * 64, _ptr(order), n, float(nms_thr),
                                    _ptr(keep), _ptr(ws), nws, _stream()), "usc_mask_bits_nms")
    else:
        check(lib.usc_mask_bits_nms_weighted(_ptr(bits), _ptr(counts), _ptr(weight), weight.numel(), _ptr(order), n,
                                             float(nms_thr), _ptr(keep), _ptr(ws), nws, _stream()),
              "usc_mask_bits_nms_weighted")
    return keep.bool()


def mask_nms_weighted(bits, counts, weight, order, nms_thr: float = 0.5) -> torch.Tensor:
    """`mask_nms(bits, counts, order, nms_thr, weight)`."""
    return mask_nms(bits, counts, order, nms_thr, weight)


def _select(maskness, rows, lo, hi, scene_extent, nms, *, instance_to_scene_max_ratio, max_instance_num,
            nms_maskness_threshold):
    """Selection steps (4) to (7) of either mode (:353-354, :375-412), torch operators only.  maskness f32[n] of the
    candidates in candidate order, rows int[n]: every candidate's row in `lo`, `hi` i32[*, 3] and in what `nms` works on,
    scene_extent [3], nms(rows in score order) -> keep bool.  -> (maskness f32[M], rows i64[M]) of the survivors in the
    reference's output order, or None where the reference prints "No candidates left" and skips the scene.
    `nms` gets the rows to judge and nothing else, so the counts it uses are those rows' own: the reference's stale
    `sum_masks` of the "none left -> all stay" branch has no counterpart here."""
    maskness, by = torch.sort(maskness, descending=True, stable=True)              # :354, ties: lower row first
    rows = rows[by]
    # extent filter (:375-395), x and y only, in f64 like numpy's int / int division
    ext = (hi[rows, :2].long() - lo[rows, :2].long()).double()
    scene = torch.as_tensor(scene_extent, device=maskness.device).double().flatten()[:2]
    ok = ~((ext / scene) > instance_to_scene_max_ratio).any(1)
    if bool(ok.any()):                                                             # none left -> all stay
        rows, maskness = rows[ok], maskness[ok]
    keep = nms(rows)                                                               # :398
    maskness = torch.where(keep, maskness, torch.zeros_like(maskness))
    maskness, by = torch.sort(maskness, descending=True, stable=True)              # :400-403
    by = by[:max_instance_num]
    maskness, rows = maskness[:max_instance_num], rows[by]
    sel = maskness > nms_maskness_threshold                                        # :412
    if not bool(sel.any()):
        return None
    return maskness[sel], rows[sel]


def _empty(K, dev, n_index):
    """The result of a scene the reference skips: no rows of K voxels, no maskness, `n_index` empty index vectors."""
    return (torch.zeros((0, K), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
            *(torch.zeros(0, dtype=torch.int64, device=dev) for _ in range(n_index)))


def freemask(key_feats, key_coords, query_feats, scene_extent, *, hard_mask_threshold=0.35, min_mask_points=10,
             instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6,
             similarity_metric="cos", segment_ids=None, use_fps_sampling=False, frame_fusion="mean"):
    """Voxel mode of freemask_main.py:242-417.  key_feats f32[K,C], key_coords int[K,3] (or [K,4]: b,x,y,z),
    query_feats f32[Q,C], scene_extent [3] (max - min of the scene's voxel coordinates).
    -> (soft_masks f32[M,K], maskness f32[M], query_index i64[M]) in the reference's output order; three empty
    tensors where the reference prints "No instances detected" / "No candidates left" and skips the scene."""
    _refuse(similarity_metric, segment_ids, use_fps_sampling, frame_fusion)
    dev = key_feats.device
    empty = _empty(key_feats.shape[0], dev, 1)
    cm, prep = _cosine_masks(key_feats, query_feats, hard_mask_threshold)
    cand = torch.nonzero(cm.counts > min_mask_points).flatten()                    # :271, ascending query index
    if cand.numel() == 0:
        return empty
    maskness = cm.soft_sums[cand] / cm.counts[cand]                                # :353 (f32 / integer)
    coords = key_coords[:, -3:].to(device=dev, dtype=torch.int32).contiguous()
    lo, hi = mask_extent(cm.bits, coords)
    chosen = _select(maskness, cand, lo, hi, scene_extent, lambda order: mask_nms(cm.bits, cm.counts, order, nms_thr),
                     instance_to_scene_max_ratio=instance_to_scene_max_ratio, max_instance_num=max_instance_num,
                     nms_maskness_threshold=nms_maskness_threshold)
    if chosen is None:
        return empty
    maskness, cand = chosen
    return soft_rows(key_feats, query_feats, cm.rowmin, cm.rowmax, cand, prep), maskness, cand


# ---------------------------------------------------------------------------------------------------- segment mode
class SegmentMasks(NamedTuple):
    soft_masks: torch.Tensor     # f32[M, K_voxels]
    maskness: torch.Tensor       # f32[M]
    query_segment: torch.Tensor  # i64[M]  id of the segment whose feature was the query
    part_root: torch.Tensor      # i64[M]  smallest segment id of the connected part


class SegmentSceneMasks(NamedTuple):
    soft_masks: torch.Tensor
    maskness: torch.Tensor
    query_segment: torch.Tensor
    part_root: torch.Tensor
    key_coords: torch.Tensor     # i32[K, 3]
    tensor_stride: int


class SplitRows(NamedTuple):
    bits: torch.Tensor        # i64[R, ceil(S/64)]
    src: torch.Tensor         # i32[R]  position of the input row in `rows`
    root: torch.Tensor        # i32[R]  smallest segment index of the part
    seg_counts: torch.Tensor  # i32[R]
    vox_counts: torch.Tensor  # i32[R]  sum of w over the part
    soft_sums: torch.Tensor   # f32[R]  sum of the soft values over the part, ascending segment index


def segment_adjacency(seg_connectivity, unique_segments, mutual=False):
    """CSR (adj_off i64[S+1], adj i32[E]) of the undirected segment adjacency over the indices of the sorted ids
    `unique_segments` i64[S]: pairs mapped to indices, pairs naming an id that is not in `unique_segments` and self
    pairs dropped, symmetrised, deduplicated, neighbours ascending (torch operators, once per scene).
    mutual=True: a and b are neighbours only when BOTH (a, b) and (b, a) are listed (the intersection of out- and
    in-neighbours of the export step, reference trainer/trainer.py:620-621)."""
    dev = unique_segments.device
    S = unique_segments.numel()
    conn = torch.as_tensor(seg_connectivity).to(device=dev, dtype=torch.int64).reshape(-1, 2)
    off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    if S == 0 or conn.shape[0] == 0:
        return off, torch.zeros(0, dtype=torch.int32, device=dev)
    pos = torch.searchsorted(unique_segments, conn.reshape(-1)).clamp_(max=S - 1).reshape(-1, 2)
    known = (unique_segments[pos] == conn).all(1) & (pos[:, 0] != pos[:, 1])
    pos = pos[known]
    if mutual:
        listed = torch.unique(pos[:, 0] * S + pos[:, 1])
        key = listed[torch.isin(listed, pos[:, 1] * S + pos[:, 0])]               # still sorted, and symmetric
    else:
        both = torch.cat([pos, pos.flip(1)], 0)
        key = torch.unique(both[:, 0] * S + both[:, 1])                           # sorted: by source, then neighbour
    src, dst = key // S, key % S
    off[1:] = torch.cumsum(torch.bincount(src, minlength=S), 0)
    return off, dst.to(torch.int32).contiguous()


def _check_adjacency(adj_off, adj, S):
    _chk(adj_off, torch.int64, "adj_off")
    _chk(adj, torch.int32, "adj")
    if adj_off.numel() != S + 1:
        raise RuntimeError(f"adj_off must have S + 1 = {S + 1} entries, got {adj_off.numel()}")
    o = adj_off.cpu()
    if int(o[0]) != 0 or int(o[-1]) != adj.numel() or bool((o[1:] < o[:-1]).any()):
        raise RuntimeError("adj_off must rise from 0 to len(adj)")
    if adj.numel() and (int(adj.min()) < 0 or int(adj.max()) >= S):
        raise RuntimeError(f"adjacency index outside [0, {S}): {int(adj.min())} .. {int(adj.max())}")


def _check_rows(bits, rows, S, name):
    _chk(bits, torch.int64, "bits")
    if bits.dim() != 2 or bits.shape[1] != (S + 63) // 64:
        raise RuntimeError(f"{name}: bits must be [rows, ceil(S/64)]")
    rows = rows.to(device=bits.device, dtype=torch.int32).contiguous()
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= bits.shape[0]):
        raise RuntimeError(f"{name}: row index out of range")
    return rows


def mask_components(bits, rows, adj_off, adj, n_segments=None, kernel="lds"):
    """Connected parts of the masks bits[rows] on the adjacency (adj_off, adj) -> (label i32[n, S]: -1 outside the mask,
    else the smallest segment index of the part; n_comp i32[n]).  The adjacency is checked on the host first: a bad
    index raises, nothing is launched.

    kernel="lds" (the default, FreeMask segment mode's call): the LDS kernel, S up to usc_mask_bits_max_segments()
    (8 192), refused above.  "wide": the kernel that keeps a row's labels in global memory (csrc/separate.hip), S up to
    usc_mask_bits_max_segments_wide() (65 536); same labels.  "auto" (the export step's choice): the LDS kernel up to
    its cap, the wide one above."""
    require_device()
    if kernel not in ("lds", "wide", "auto"):
        raise ValueError(f"mask_components: kernel must be 'lds', 'wide' or 'auto', not {kernel!r}")
    S = adj_off.numel() - 1 if n_segments is None else int(n_segments)
    cap = lib.usc_mask_bits_max_segments()
    wide = kernel == "wide" or (kernel == "auto" and S > cap)
    if wide:
        cap_wide = lib.usc_mask_bits_max_segments_wide()
        if not 1 <= S <= cap_wide:
            raise RuntimeError(f"mask_components: S = {S} segments outside [1, {cap_wide}] (one workgroup walks a row's "
                               "labels in global memory; above this count one round is too long for one workgroup)")
    elif not 1 <= S <= cap:
        raise RuntimeError(f"mask_components: S = {S} segments outside [1, {cap}] (a row's labels live in LDS)")
    _check_adjacency(adj_off, adj, S)
    rows = _check_rows(bits, rows, S, "mask_components")
    n = rows.numel()
    label = torch.empty((n, S), dtype=torch.int32, device=bits.device)
    ncomp = torch.empty(n, dtype=torch.int32, device=bits.device)
    if n and wide:
        status = torch.empty(1, dtype=torch.int32, device=bits.device)
        check(lib.usc_mask_bits_components_wide(_ptr(bits), bits.shape[0], S, _ptr(rows), n, _ptr(adj_off), _ptr(adj),
                                                _ptr(label), _ptr(ncomp), _ptr(status), _stream()),
              "usc_mask_bits_components_wide")
    elif n:
        check(lib.usc_mask_bits_components(_ptr(bits), bits.shape[0], S, _ptr(rows), n, _ptr(adj_off), _ptr(adj),
                                           _ptr(label), _ptr(ncomp), _stream()), "usc_mask_bits_components")
    return label, ncomp


def mask_split(label, n_comp, seg_weight, soft, soft_row) -> SplitRows:
    """One row per (input row, part) in (row, root) order from `mask_components`' output; seg_weight i32[S] (key voxels
    per segment, >= 0, sum < 2^24), soft f32[*, S], soft_row int[n]: the row of `soft` that belongs to input row i."""
    require_device()
    _chk(label, torch.int32, "label")
    _chk(n_comp, torch.int32, "n_comp")
    _chk(seg_weight, torch.int32, "seg_weight")
    _chk(soft, torch.float32, "soft")
    n, S = label.shape
    dev = label.device
    soft_row = soft_row.to(device=dev, dtype=torch.int32).contiguous()
    if n_comp.numel() != n or soft_row.numel() != n or seg_weight.numel() != S or soft.dim() != 2 or soft.shape[1] != S:
        raise RuntimeError("mask_split: label [n, S], n_comp [n], soft_row [n], seg_weight [S], soft [*, S] do not match")
    if n and (int(soft_row.min()) < 0 or int(soft_row.max()) >= soft.shape[0]):
        raise RuntimeError("mask_split: soft_row out of range")
    if n and (int(n_comp.min()) < 0 or int(n_comp.max()) > S):
        raise RuntimeError("mask_split: n_comp outside [0, S]")
    if int(seg_weight.min()) < 0 or int(seg_weight.long().sum()) >= 1 << 24:
        raise RuntimeError("mask_split: weights must be >= 0 and sum to less than 2^24 (vox_counts are i32 sums, and "
                           "the weighted NMS divides them in f32)")
    incl = torch.cumsum(n_comp.long(), 0)
    R = int(incl[-1]) if n else 0
    row_off = (incl - n_comp.long()).contiguous()
    W = (S + 63) // 64
    i32 = [torch.empty(R, dtype=torch.int32, device=dev) for _ in range(4)]      # src, root, seg_counts, vox_counts
    out = SplitRows(torch.empty((R, W), dtype=torch.int64, device=dev), *i32,
                    torch.empty(R, dtype=torch.float32, device=dev))
    if R:
        check(lib.usc_mask_bits_split(_ptr(label), n, S, _ptr(row_off), _ptr(n_comp), _ptr(seg_weight), _ptr(soft), S,
                                      _ptr(soft_row), _ptr(out.bits), _ptr(out.src), _ptr(out.root),
                                      _ptr(out.seg_counts), _ptr(out.vox_counts), _ptr(out.soft_sums), _stream()),
              "usc_mask_bits_split")
    return out


def segment_features(key_feats, key_segment_ids):
    """:202-225 -> (seg_feats f32[S, C], unique_segments i64[S] sorted, idx i64[K]: the segment index of every key voxel,
    -1 for the voxels of a dropped (all-zero) segment)."""
    unique0, inv = torch.unique(key_segment_ids, return_inverse=True)
    S0 = unique0.numel()
    feats = key_feats.float().contiguous()
    csr = ops.segment_csr(inv.to(torch.int64).contiguous(), S0)
    mean = torch.empty((S0, feats.shape[1]), dtype=torch.float32, device=feats.device)
    check(lib.usc_segment_mean_nonzero(_ptr(feats), feats.shape[1], _ptr(csr.order), _ptr(csr.seg_off), S0, _ptr(mean),
                                       None, _stream()), "usc_segment_mean_nonzero")
    valid = (mean != 0).any(1)                                                    # :223-225
    new_index = torch.cumsum(valid.long(), 0) - 1
    new_index[~valid] = -1
    return mean[valid].contiguous(), unique0[valid], new_index[inv]


def segment_tables(idx, key_coords, S):
    """w i32[S] = key voxels of every segment, lo / hi i32[S, 3] = their box (idx = -1 voxels belong to none)."""
    dev = idx.device
    live = idx >= 0
    ii, cc = idx[live], key_coords[live].to(torch.int32)
    w = torch.bincount(ii, minlength=S).to(torch.int32)
    lo = torch.full((S, 3), torch.iinfo(torch.int32).max, dtype=torch.int32, device=dev)
    hi = torch.full((S, 3), torch.iinfo(torch.int32).min, dtype=torch.int32, device=dev)
    ix = ii[:, None].expand(-1, 3)
    lo.scatter_reduce_(0, ix, cc, "amin")
    hi.scatter_reduce_(0, ix, cc, "amax")
    return w, lo.contiguous(), hi.contiguous()


def freemask_segments(key_feats, key_coords, key_segment_ids, seg_connectivity, scene_extent, *,
                      hard_mask_threshold=0.35, min_mask_segments=2, min_part_segments=3,
                      instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6,
                      similarity_metric="cos", use_fps_sampling=False, frame_fusion="mean") -> SegmentMasks:
    """Segment mode of freemask_main.py (:202-233, :242, :266-279, :282-417).  key_feats f32[K,C], key_coords int[K,3]
    (or [K,4]: b,x,y,z), key_segment_ids i64[K] (the ids pooled to the keys' resolution), seg_connectivity int[P,2]
    (pairs of ids), scene_extent [3].  -> SegmentMasks in the reference's output order; empty tensors where the
    reference prints "No instances detected" / "No candidates left" and skips the scene."""
    _refuse(similarity_metric, None, use_fps_sampling, frame_fusion)
    require_device()
    dev = key_feats.device
    K = key_feats.shape[0]
    ids = key_segment_ids.to(device=dev, dtype=torch.int64).reshape(-1)
    if ids.numel() != K:
        raise RuntimeError("freemask_segments: key_segment_ids must have one id per key voxel")
    if K >= 1 << 24:
        raise RuntimeError("freemask_segments: K >= 2^24 key voxels: voxel counts would not be exact in f32")
    empty = SegmentMasks(*_empty(K, dev, 2))
    if K == 0:
        return empty
    seg_feats, unique_segments, idx = segment_features(key_feats, ids)             # :202-228
    S = seg_feats.shape[0]
    if S == 0:
        return empty
    cap = lib.usc_mask_bits_max_segments()
    if S > cap:
        raise RuntimeError(f"freemask_segments: {S} segments above the {cap} a row's LDS label image holds")
    coords = key_coords[:, -3:].to(device=dev, dtype=torch.int32).contiguous()
    w, seg_lo, seg_hi = segment_tables(idx, coords, S)
    adj_off, adj = segment_adjacency(seg_connectivity, unique_segments)            # :230-233, undirected
    cm, prep = _cosine_masks(seg_feats, seg_feats, hard_mask_threshold)            # :242, :266-268
    cand = torch.nonzero(cm.counts > min_mask_segments).flatten()                  # :271, ascending query index
    if cand.numel() == 0:
        return empty
    soft = torch.cat([soft_rows(seg_feats, seg_feats, cm.rowmin, cm.rowmax, cand[i:i + 4096], prep)
                      for i in range(0, cand.numel(), 4096)], 0)                   # f32 [candidates, S]
    label, ncomp = mask_components(cm.bits, cand, adj_off, adj, S)                 # :288-327
    sp = mask_split(label, ncomp, w, soft, torch.arange(cand.numel(), device=dev))  # :329-342
    part = torch.nonzero(sp.seg_counts > min_part_segments).flatten()              # :345, (query, root) order
    if part.numel() == 0:
        return empty
    maskness = sp.soft_sums[part] / sp.seg_counts[part]                            # :353, a segment-level mean
    # boxes of the remapped masks (:361-395): the union of the boxes of a row's segments
    lo, _ = mask_extent(sp.bits, seg_lo)
    _, hi = mask_extent(sp.bits, seg_hi)
    chosen = _select(maskness, part, lo, hi, scene_extent,
                     lambda order: mask_nms(sp.bits, sp.vox_counts, order, nms_thr, w),     # :398 on voxel counts
                     instance_to_scene_max_ratio=instance_to_scene_max_ratio, max_instance_num=max_instance_num,
                     nms_maskness_threshold=nms_maskness_threshold)
    if chosen is None:
        return empty
    maskness, part = chosen
    src, root = sp.src[part].long(), sp.root[part].long()
    seg_rows = torch.where(label[src] == root[:, None], soft[src], torch.zeros((), dtype=torch.float32, device=dev))
    seg_rows = torch.cat([seg_rows, torch.zeros((len(part), 1), dtype=torch.float32, device=dev)], 1)
    out = seg_rows[:, torch.where(idx >= 0, idx, torch.full_like(idx, S))]         # :361-368, the only [M, K] tensor
    return SegmentMasks(out.contiguous(), maskness, unique_segments[cand[src]], unique_segments[root])


# ------------------------------------------------------------------------------------- scene level, both modes
def _pool_steps(resolution_scale):
    steps = int(math.log2(resolution_scale))
    if resolution_scale < 1 or 2 ** steps != resolution_scale:
        raise ValueError(f"resolution_scale must be a power of two, got {resolution_scale}")
    return steps


def _scene_extent(coords):
    c = coords[:, -3:]
    return (c.amax(0) - c.amin(0)).float()


def _pool(x, steps, pooling):
    pool = pooling(kernel_size=2, stride=2, dimension=3)
    for _ in range(steps):
        x = pool(x)
    return x


def _pool_segment_ids(segment_ids, like, steps):
    """:189-199: the id column on `like`'s coordinate map, max-pooled `steps` times -> i64[K]."""
    from .. import MinkowskiEngine as ME
    ids = torch.as_tensor(segment_ids).to(device=like.device).reshape(-1)
    if ids.is_floating_point():
        raise RuntimeError("segment ids must be integers")
    if ids.numel() != like.F.shape[0]:
        raise RuntimeError(f"{ids.numel()} segment ids for {like.F.shape[0]} voxels")
    pooled = ME.SparseTensor(features=ids.to(torch.int64).view(-1, 1), coordinate_manager=like.coordinate_manager,
                             coordinate_map_key=like.coordinate_map_key)
    if steps == 0:          # no pooling: the range check of the pooling operator still holds
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= ops.MAXPOOL_I32_ID_LIMIT):
            raise RuntimeError(f"segment ids outside [0, 2^24): {int(ids.min())} .. {int(ids.max())}")
    return _pool(pooled, steps, ME.MinkowskiMaxPooling).F.reshape(-1).to(torch.int64)


def _keys_from_voxel_feats(coords, feats, steps, unique_for=None):
    """coords int[N,3] or [N,4], feats [N,d] -> (the fine tensor on them, the keys: it average-pooled `steps` times
    (:162-179), the scene extent).  `unique_for` names the caller that needs one row per coordinate."""
    from .. import MinkowskiEngine as ME
    require_device()
    coords = coords.to(torch.int32)
    if coords.shape[1] == 3:
        coords = torch.cat([torch.zeros_like(coords[:, :1]), coords], 1)
    fine = ME.SparseTensor(features=feats.float().contiguous(), coordinates=coords.contiguous(), device=feats.device)
    if unique_for and fine.F.shape[0] != coords.shape[0]:
        raise RuntimeError(f"{unique_for}: coords must be unique")
    return fine, _pool(fine, steps, ME.MinkowskiAvgPooling), _scene_extent(coords)


def _keys_from_backbone(model, sinput, resolution_scale):
    """:98-101: the backbone's `res_{scale}` feature map."""
    _, feature_maps = model(sinput)
    return feature_maps[f"res_{resolution_scale}"]


def _from_keys(keys, steps, extent, kw, key_ids=None, seg_connectivity=None):
    """Voxel mode (queries = the keys average-pooled `steps` more times, :173-183) or, with `key_ids`, segment mode."""
    from .. import MinkowskiEngine as ME
    kf = keys.F.detach().float().contiguous()
    kc = keys.C[:, 1:].contiguous()
    if key_ids is None:
        qf = _pool(keys, steps, ME.MinkowskiAvgPooling).F.detach().float().contiguous()
        return SceneMasks(*freemask(kf, kc, qf, extent, **kw), kc, keys.tensor_stride[0])
    return SegmentSceneMasks(*freemask_segments(kf, kc, key_ids, seg_connectivity, extent, **kw), kc,
                             keys.tensor_stride[0])


def freemask_scene(model, sinput, resolution_scale=2, **kw) -> SceneMasks:
    """3D branch (:98-101, :171-183): keys = the backbone's `res_{scale}` feature map, queries = the keys
    average-pooled log2(scale) more times."""
    _refuse(**kw)
    steps = _pool_steps(resolution_scale)
    with torch.no_grad():
        return _from_keys(_keys_from_backbone(model, sinput, resolution_scale), steps, _scene_extent(sinput.C), kw)


def freemask_from_voxel_feats(coords, feats, resolution_scale=2, **kw) -> SceneMasks:
    """Image branch (:162-179): per-voxel features (e.g. encode_scene_feats_2d's) on the unique voxel coordinates
    `coords` int[N,3] or [N,4] are average-pooled log2(scale) times to the keys, and as often again to the queries."""
    _refuse(**kw)
    steps = _pool_steps(resolution_scale)
    with torch.no_grad():
        _, keys, extent = _keys_from_voxel_feats(coords, feats, steps)
        return _from_keys(keys, steps, extent, kw)


def freemask_scene_fn(scene, **kw) -> SceneMasks:
    """`scene_fn` of PseudoMaskDriver: scene = dict with `coords`, `feats` and optionally `resolution_scale`."""
    return freemask_from_voxel_feats(scene["coords"], scene["feats"], scene.get("resolution_scale", 2), **kw)


def freemask_segments_scene(model, sinput, segment_ids, seg_connectivity, resolution_scale=2, **kw) -> SegmentSceneMasks:
    """3D branch: keys = the backbone's `res_{scale}` feature map; `segment_ids` int[N] are the ids of `sinput`'s
    voxels, max-pooled log2(scale) times onto the keys' coordinate map."""
    _refuse(**kw)
    steps = _pool_steps(resolution_scale)
    with torch.no_grad():
        keys = _keys_from_backbone(model, sinput, resolution_scale)
        key_ids = _pool_segment_ids(segment_ids, sinput, steps)
        if key_ids.numel() != keys.F.shape[0]:
            raise RuntimeError("freemask_segments_scene: the pooled ids and the feature map live on different maps")
        return _from_keys(keys, steps, _scene_extent(sinput.C), kw, key_ids, seg_connectivity)


def freemask_segments_from_voxel_feats(coords, feats, segment_ids, seg_connectivity, resolution_scale=2,
                                       **kw) -> SegmentSceneMasks:
    """Image branch: per-voxel features on the unique voxel coordinates `coords` int[N,3] or [N,4] are average-pooled
    log2(scale) times to the keys, the ids `segment_ids` int[N] max-pooled as often over the same maps."""
    _refuse(**kw)
    steps = _pool_steps(resolution_scale)
    with torch.no_grad():
        fine, keys, extent = _keys_from_voxel_feats(coords, feats, steps, "freemask_segments_from_voxel_feats")
        return _from_keys(keys, steps, extent, kw, _pool_segment_ids(segment_ids, fine, steps), seg_connectivity)


def freemask_segments_scene_fn(scene, **kw) -> SegmentSceneMasks:
    """`scene_fn` of PseudoMaskDriver: scene = dict with `coords`, `feats`, `segment_ids`, `seg_connectivity` (as
    scans.build_scene writes them) and optionally `resolution_scale`."""
    for key in ("segment_ids", "seg_connectivity"):
        if key not in scene:
            raise KeyError(f"freemask segment mode needs `{key}` in the scene")
    return freemask_segments_from_voxel_feats(scene["coords"], scene["feats"], scene["segment_ids"],
                                              scene["seg_connectivity"], scene.get("resolution_scale", 2), **kw)


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
