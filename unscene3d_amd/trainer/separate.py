"""`general.separate_instances` of the export step (reference trainer/trainer.py:609-650 with
utils/point_cloud_utils.py:82-121 `separate_segments`): every predicted instance that survives the overlap filter is
cut into its connected parts on the adjacency of the mesh over-segmentation, and every part becomes an instance of its
own — the mesh-topology counterpart of the DBSCAN split.

For one scene, with masks bool[N, K] (kept instances in score order), seg int[N] (the points' segment ids, in the id
space of the connectivity) and conn int[P, 2]:

1. U = sorted unique ids of seg, S = len(U), idx(r) in [0, S);
2. a — b iff BOTH (a, b) and (b, a) are listed (`segment_adjacency(mutual=True)`, the reference's set.intersection of
   out- and in-neighbours); self pairs and pairs naming an id that is not in U are ignored;
3. segment s belongs to instance j iff ANY point of s has masks[:, j] set;
4. the parts of j are the connected components of its segments on that adjacency, ordered by their smallest segment
   index;
5. one output column per (instance, part) in that order, holding all points whose segment is in the part.

Deviations from the reference, on purpose (the same two as DESIGN.md §3.22 (d), for the same scan):
* the parts are the TRUE components.  The reference's scan pops a merged blob and then still advances its cursor
  (`pop(fused_id)`, `fused_id += 1`), so the blob that slides into the popped place is never looked at and a segment
  that bridges three blobs can leave two connected blobs apart;
* the order of one instance's parts is by smallest segment index; the reference's blob order (insertion order, changed
  by merges) matters only between parts that share one score, which they all do.
The reference also indexes its segment mask with the raw ids (`segment_inst_mask[ids] = True`, :629), which is only right
for ids 0 .. S-1; here ids are looked up in U.

On the device (csrc/separate.hip) an instance is an S-bit row between two passes over the table:
`ops.mask_columns_to_segment_bits` -> `mask_components` (the LDS kernel up to 8 192 segments, the wide one up to
65 536) -> `ops.segment_parts_to_columns`.  Nothing of size N x K x anything is allocated: above its inputs
`separate_columns` holds the bit rows, the labels i32[K, S] and the [N, R] result."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .._lib import lib
from ..pseudo_masks.freemask import mask_components, segment_adjacency


def separate_columns(masks, csr, idx, adj_off, adj, check_range=True):
    """The device part.  masks bool / u8 [N, K]; csr = ops.segment_csr(idx as i64, S); idx i32[N] the points' segment
    indices; (adj_off, adj) the symmetric CSR adjacency over [0, S) -> (bool[N, R], src i64[R] the input column of
    every output column), columns in (instance, smallest segment index of the part) order.  The CSR's values and idx
    are checked on the host before the first launch (`check_range=False`: the caller built them and vouches for
    them); the adjacency is always checked by `mask_components`.  One more host read: R.

    Memory above the inputs: the bit rows (freed before the result is allocated), the labels i32[K, S], the [N, R]
    result, and beside the result only the parts' vectors src i64[R], src / root i32[R]."""
    N, K = masks.shape
    dev = masks.device
    if K == 0 or N == 0:
        return torch.zeros((N, 0), dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    S = int(csr.S)
    if check_range:
        if idx.dtype != torch.int32 or idx.shape != (N,):
            raise RuntimeError(f"separate_columns: idx must be int32 [{N}]")
        lo, hi = (int(v) for v in torch.aminmax(idx))       # host integers: no device scalar outlives the check
        if lo < 0 or hi >= S:
            raise RuntimeError(f"separate_columns: idx outside [0, {S})")
    bits = ops.mask_columns_to_segment_bits(masks, csr, check_range=check_range)
    label = mask_components(bits, torch.arange(K, dtype=torch.int32, device=dev), adj_off, adj, n_segments=S,
                            kernel="auto")[0]
    del bits
    # a part's root is the segment that carries its own index: nonzero lists them by (row, index), which is the
    # (instance, smallest segment index) order of the columns
    parts = torch.nonzero(label == torch.arange(S, dtype=torch.int32, device=dev))
    # copies, not views (a column of nonzero's table can be contiguous already), so that the table can go
    src = parts[:, 0].clone(memory_format=torch.contiguous_format)
    src32, root32 = src.to(torch.int32), parts[:, 1].to(torch.int32).contiguous()
    del parts
    out = ops.segment_parts_to_columns(label, src32, root32, idx, check_range=False)     # src < K by construction
    return out, src


def separate_instances(masks, seg_full, connectivity):
    """masks bool[N, K] (device), seg_full int[N] segment ids, connectivity int[P, 2] pairs of ids
    -> (masks bool[N, R], src i64[R]): one column per (instance, part), `src` the instance a column came from.
    Everything that indexes is checked or built on the host side of the launches: a bad argument raises before the
    first kernel."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 2 or masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("separate_instances: masks must be a bool or uint8 tensor [N, K]")
    if not masks.is_cuda:
        raise RuntimeError("separate_instances: masks must be a HIP (cuda) tensor — unscene3d_amd has no CPU path")
    N, K = masks.shape
    dev = masks.device
    seg = torch.as_tensor(seg_full)
    if seg.dim() != 1 or seg.shape[0] != N or seg.dtype.is_floating_point and bool((seg != seg.round()).any()):
        raise RuntimeError(f"separate_instances: seg_full must hold one integer segment id per point ({N}), got "
                           f"{tuple(seg.shape)} {seg.dtype}")
    conn = torch.as_tensor(np.asarray(connectivity) if not isinstance(connectivity, torch.Tensor) else connectivity)
    if conn.numel() == 0:                                  # [] arrives as an empty float array: no pairs
        conn = torch.zeros((0, 2), dtype=torch.int64)
    if conn.numel() and (conn.dim() != 2 or conn.shape[1] != 2):
        raise RuntimeError(f"separate_instances: connectivity must be [P, 2] pairs of segment ids, got {tuple(conn.shape)}")
    if conn.dtype.is_floating_point or conn.dtype == torch.bool:
        raise RuntimeError(f"separate_instances: connectivity must hold integer ids, got {conn.dtype}")
    if N == 0 or K == 0:
        return masks.new_zeros((N, 0), dtype=torch.bool), torch.zeros(0, dtype=torch.int64, device=dev)
    uniq, idx = torch.unique(seg.to(device=dev, dtype=torch.int64), return_inverse=True)
    S = uniq.numel()
    cap = lib.usc_mask_bits_max_segments_wide()
    if S > cap:
        raise RuntimeError(f"separate_instances: the scene has {S} segments, more than {cap}: one workgroup walks the "
                           "labels of an instance, and above this count one round of it is too long")
    csr = ops.segment_csr(idx.contiguous(), S)
    adj_off, adj = segment_adjacency(conn.reshape(-1, 2), uniq, mutual=True)
    # the CSR and the indices were built two lines up from torch.unique's inverse: in range by construction
    return separate_columns(masks.contiguous(), csr, idx.to(torch.int32), adj_off, adj, check_range=False)
