"""float64 numpy restatement of the FreeMask voxel-mode pipeline (unscene3d_amd/pseudo_masks/freemask.py), written
from its description, not from the device code.  Used by the host and the GPU tests.

  1  k^ = Fk / (|Fk| + 1e-9), q^ likewise; a = q^ k^T; per row a -= rowmin; a /= (rowmax_after + 1e-9)
  2  columns of all-zero keys := 0
  3  mask = a >= hard_mask_threshold; candidates: popcount > min_mask_points
  4  maskness = sum(a * mask) / count; candidates by maskness, descending, STABLE (lower query index first on ties)
  5  drop masks whose x or y extent over their keys' coordinates exceeds ratio * scene extent; none left -> keep all
  6  greedy mask NMS in that order: a live i kills every later live j with
       union > 0 ? float32(inter) / float32(union) > nms_thr : true;   dead masks get maskness 0
  7  sort again (stable), first max_instance_num, then maskness > nms_maskness_threshold
  8  soft rows, maskness, query indices of the survivors
"""
import numpy as np

EPS = 1e-9


def cosine_rows(fk, fq):
    """-> (a f64[Q,K] normalised and key-zeroed, raw rowmin f64[Q], raw rowmax f64[Q], zero-key mask bool[K])."""
    fk, fq = np.asarray(fk, np.float64), np.asarray(fq, np.float64)
    kh = fk / (np.linalg.norm(fk, axis=1, keepdims=True) + EPS)
    qh = fq / (np.linalg.norm(fq, axis=1, keepdims=True) + EPS)
    raw = qh @ kh.T
    lo, hi = raw.min(1), raw.max(1)
    a = raw - lo[:, None]
    a = a / (a.max(1, keepdims=True) + EPS)
    zero = np.all(fk == 0, axis=1)
    a[:, zero] = 0.0
    return a, lo, hi, zero


def greedy_nms(masks, counts, nms_thr=0.5):
    """masks bool[n,K] in score order, counts int[n] -> keep bool[n] (the integer greedy loop of matrix_nms)."""
    masks = np.asarray(masks, bool)
    n = len(masks)
    keep = np.ones(n, bool)
    for i in range(n):
        if not keep[i]:
            continue
        for j in range(i + 1, n):
            if not keep[j]:
                continue
            inter = int(np.count_nonzero(masks[i] & masks[j]))
            union = int(counts[i]) + int(counts[j]) - inter
            if union > 0:
                if np.float32(inter) / np.float32(union) > np.float32(nms_thr):
                    keep[j] = False
            else:
                keep[j] = False
    return keep


def mask_extent(masks, coords):
    """-> (lo, hi) int64[n,3]; an empty mask gives lo = INT32_MAX, hi = INT32_MIN."""
    masks, coords = np.asarray(masks, bool), np.asarray(coords, np.int64)
    lo = np.full((len(masks), 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((len(masks), 3), np.iinfo(np.int32).min, np.int64)
    for i, m in enumerate(masks):
        if m.any():
            lo[i], hi[i] = coords[m].min(0), coords[m].max(0)
    return lo, hi


def freemask_ref(fk, coords, fq, scene_extent, hard_mask_threshold=0.35, min_mask_points=10,
                 instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6):
    """-> (soft rows f64[M,K], maskness f64[M], query index int64[M])."""
    a, _, _, _ = cosine_rows(fk, fq)
    K = a.shape[1]
    empty = (np.zeros((0, K)), np.zeros(0), np.zeros(0, np.int64))
    masks = a >= hard_mask_threshold
    counts = masks.sum(1)
    cand = np.nonzero(counts > min_mask_points)[0]
    if len(cand) == 0:
        return empty
    maskness = (a[cand] * masks[cand]).sum(1) / counts[cand]
    by = np.argsort(-maskness, kind="stable")
    cand, maskness = cand[by], maskness[by]
    lo, hi = mask_extent(masks[cand], coords)
    ratios = (hi - lo)[:, :2] / np.asarray(scene_extent, np.float64)[:2]
    ok = ~np.any(ratios > instance_to_scene_max_ratio, axis=1)
    if ok.any():
        cand, maskness = cand[ok], maskness[ok]
    keep = greedy_nms(masks[cand], counts[cand], nms_thr)
    maskness = np.where(keep, maskness, 0.0)
    by = np.argsort(-maskness, kind="stable")[:max_instance_num]
    cand, maskness = cand[by], maskness[by]
    sel = maskness > nms_maskness_threshold
    if not sel.any():
        return empty
    return a[cand[sel]], maskness[sel], cand[sel]
