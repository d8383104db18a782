"""ops.attn_mask_rows (usc_attn_mask_rows, csrc/rows.hip): the thresholded attention-mask rows of a decoder pass's sampled
keys in one launch, byte for byte what the chain it replaces gives on the same inputs — ops.avgpool_down2 once per
pooling step, `threshold` on the last, then ops.sample_keys(None, mask, None, idx, ...).  Compared: the final bool[B, K, Q]
(after the all-masked-column rule) and the rows before that rule (fix=False) against the gathered rows of the chain's mask
with the padding rows masked.  Every case runs the new entry twice.

Scenes of about 3 000 and 1 400 voxels (levels of 3 082 / 1 151 / 316 / 100 / 36 and 1 396 / 558 / 151 / 46 / 17 rows),
41 segments per scene."""
import numpy as np
import pytest
import torch

import attn_mask_rows_cases as cases

pytestmark = pytest.mark.gpu

N_SEG = 41
_SCENES = {}


def _scene_coords(seed, target):
    from unscene3d_amd.synthetic import make_scene
    from oracle import sparse_ref as R

    sc = make_scene(seed, target_voxels=target, tol=0.1)
    ec = R.voxel_floor(sc["xyz"], 0.02)
    eu, _ = R.sparse_quantize(ec)
    return ec[eu]


def _batch(device, n_scenes):
    """-> dict(tables: the four child tables of the batch, finest first, the first one folded with the segment rows;
    rows[d]: per scene the batch-wide rows of the level after d pooling steps; n_seg: rows of the stacked segment
    tables).  Built once per batch size and left unchanged."""
    hit = _SCENES.get(n_scenes)
    if hit is not None:
        return hit
    from oracle import sparse_ref as R
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd.models.mask3d import _child_segment_table

    per_scene = [_scene_coords(1000, 3000), _scene_coords(1001, 1500)][:n_scenes]
    coords4, _ = R.sparse_collate(per_scene, [np.zeros((len(c), 3), np.float32) for c in per_scene])
    x = ME.SparseTensor(features=torch.zeros(len(coords4), 3, device=device),
                        coordinates=torch.from_numpy(coords4).to(device), device=device)
    cm = x.coordinate_manager
    g = torch.Generator().manual_seed(17)
    # stacked segment tables: scene b's voxels point into rows [b * N_SEG, (b + 1) * N_SEG)
    p2s = torch.cat([torch.randint(0, N_SEG, (len(c),), generator=g) + b * N_SEG for b, c in enumerate(per_scene)])
    p2s = p2s.to(device)
    tables = [_child_segment_table(cm, 1, p2s)] + [cm.stride_map(1 << s)["nbr2"] for s in (1, 2, 3)]
    rows = {}
    for d in (1, 2, 3, 4):
        bcol = cm.coord_map(1 << d).coords[:, 0].cpu()
        rows[d] = [torch.nonzero(bcol == b).flatten() for b in range(n_scenes)]
        assert sum(len(r) for r in rows[d]) == tables[d - 1].shape[1]
    hit = _SCENES[n_scenes] = dict(tables=tables, rows=rows, n_seg=N_SEG * n_scenes)
    return hit


def _logits(n_rows, q, device, seed=0, ld=128):
    """f32[n_rows, q] as a column slice of an [n_rows, ld] table.  Column 0 is negative in every row (masked at every
    key: the fix clears it), column 1 positive in every row (masked at no key)."""
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.randn(n_rows, ld, generator=g) * 0.2
    t[:, 0] = -t[:, 0].abs() - 0.01
    t[:, 1] = t[:, 1].abs() + 0.01
    return t.to(device)[:, :q]


def _key_sample(level_rows, K, seed):
    """The decoder's plan for one pass: per scene a distinct random subset of K rows, or (level smaller than K) every row
    followed by padding that repeats the scene's first row -> (idx i64[B*K], n_valid)."""
    g = torch.Generator().manual_seed(seed)
    idx, n_valid = [], []
    for r in level_rows:
        n = len(r)
        if n > K:
            idx.append(r[torch.randperm(n, generator=g)[:K]])
            n_valid.append(K)
        else:
            idx.append(torch.cat([r, r[:1].expand(K - n)]))
            n_valid.append(n)
    return torch.cat(idx).contiguous(), n_valid


def _chain(logits, tables, idx, B, K, n_valid):
    """Today's chain -> (final bool[B, K, Q], the rows before the all-masked-column rule)."""
    from unscene3d_amd import ops

    pooled = logits
    for step, tab in enumerate(tables):
        pooled = ops.avgpool_down2(pooled, tab, threshold=step == len(tables) - 1)
    final = ops.sample_keys(None, pooled, None, idx, B, K, n_valid)
    pre = pooled[idx].view(B, K, -1).clone()
    for b, nv in enumerate(n_valid):
        pre[b, nv:] = True
    return final, pre, pooled


def _check(logits, tables, idx, B, K, n_valid, with_outs=False):
    from unscene3d_amd import ops

    final, pre, pooled = _chain(logits, tables, idx, B, K, n_valid)
    q = logits.shape[1]
    outs = torch.zeros((B, K, q), dtype=torch.bool, device=logits.device) if with_outs else None
    got = ops.attn_mask_rows(logits, tables, idx, B, K, n_valid, outs=outs)
    if with_outs:
        assert got.data_ptr() == outs.data_ptr()
    got_pre = ops.attn_mask_rows(logits, tables, idx, B, K, n_valid, fix=False)
    again = ops.attn_mask_rows(logits, tables, idx, B, K, n_valid)
    assert got.dtype == torch.bool and got.shape == (B, K, q)
    a, b_, c, d_ = (t.view(torch.uint8) for t in (got, final, got_pre, pre))
    assert int(a.max()) <= 1 and int(c.max()) <= 1                                      # bool bytes are 0 / 1
    assert torch.equal(c, d_), f"rows before the fix: {int((c != d_).sum())} bytes differ"
    assert torch.equal(a, b_), f"final rows: {int((a != b_).sum())} bytes differ"
    assert torch.equal(again.view(torch.uint8), a)
    return got, got_pre, pooled


# (d, Q, B, K): K below the level (a distinct random subset), the four depths; K = 1; K = 37 (no multiple of the 64, 16
# or 4 keys of a workgroup at depth 1, 2, 3; 200 keys at depth 1 are three full workgroups and a ragged one); both ends
# of the query range
SUBSET_CASES = [(1, 100, 1, 200), (2, 100, 1, 100), (3, 100, 1, 37), (4, 100, 1, 7),
                (1, 100, 1, 1), (2, 100, 1, 1), (3, 100, 1, 1), (4, 100, 1, 1),
                (1, 100, 1, 37), (2, 100, 1, 37),
                (1, 4, 1, 50), (2, 4, 1, 50), (3, 4, 1, 21), (4, 4, 1, 5),
                (1, 128, 1, 50), (2, 128, 1, 50), (3, 128, 1, 21), (4, 128, 1, 5)]


@pytest.mark.parametrize("d,q,B,K", SUBSET_CASES)
def test_sampled_rows_equal_the_chain(device, d, q, B, K):
    s = _batch(device, B)
    assert all(len(r) > K for r in s["rows"][d])
    idx, n_valid = _key_sample(s["rows"][d], K, seed=K + d)
    got, got_pre, pooled = _check(_logits(s["n_seg"], q, device, seed=d), s["tables"][:d], idx.to(device), B, K, n_valid)
    if q >= 100 and K >= 37:
        assert 0.2 < float(pooled[:, 2:].float().mean()) < 0.8                          # both decisions occur


@pytest.mark.parametrize("d,K", [(1, 1200), (2, 330), (3, 128), (4, 40)])
def test_padding_rows_when_the_level_is_smaller_than_k(device, d, K):
    s = _batch(device, 1)
    n = len(s["rows"][d][0])
    assert n < K
    idx, n_valid = _key_sample(s["rows"][d], K, seed=0)
    assert n_valid == [n]
    got, got_pre, _ = _check(_logits(s["n_seg"], 100, device, seed=7), s["tables"][:d], idx.to(device), 1, K, n_valid)
    assert bool(got[0, n:].all()) and bool(got_pre[0, n:].all())                        # padding: masked for every query


@pytest.mark.parametrize("d,K", [(1, 600), (2, 200), (3, 50), (4, 20)])
def test_two_scenes_of_different_size(device, d, K):
    """Stacked segment tables, batch-wide rows, per-scene n_valid: the first scene is sampled, the second (half the size)
    is all-sampled with padding."""
    s = _batch(device, 2)
    n0, n1 = (len(r) for r in s["rows"][d])
    assert n0 > K > n1, (n0, n1)
    idx, n_valid = _key_sample(s["rows"][d], K, seed=d)
    assert n_valid == [K, n1]
    _check(_logits(s["n_seg"], 100, device, seed=11), s["tables"][:d], idx.to(device), 2, K, n_valid)


@pytest.mark.parametrize("d,K", [(1, 200), (4, 7)])
def test_the_callers_buffer(device, d, K):
    s = _batch(device, 1)
    idx, n_valid = _key_sample(s["rows"][d], K, seed=3)
    _check(_logits(s["n_seg"], 100, device, seed=5), s["tables"][:d], idx.to(device), 1, K, n_valid, with_outs=True)


@pytest.mark.parametrize("d,K", [(1, 200), (2, 100), (3, 37), (4, 7), (3, 100), (3, 110)])
def test_all_masked_and_never_masked_queries(device, d, K):
    """Column 0 (negative logits everywhere) is masked at every key before the fix and cleared by it — in the real rows;
    the padding rows stay masked.  Column 1 (positive everywhere) is masked at no real key."""
    s = _batch(device, 1)
    idx, n_valid = _key_sample(s["rows"][d], K, seed=9)
    nv = n_valid[0]
    got, got_pre, _ = _check(_logits(s["n_seg"], 100, device, seed=d), s["tables"][:d], idx.to(device), 1, K, n_valid)
    assert bool(got_pre[0, :, 0].all()) and not bool(got[0, :nv, 0].any()) and bool(got[0, nv:, 0].all())
    assert not bool(got_pre[0, :nv, 1].any()) and not bool(got[0, :nv, 1].any())


def test_contiguous_logits(device):
    """Leading dimension == Q == 100 (no padded table behind the columns)."""
    s = _batch(device, 1)
    idx, n_valid = _key_sample(s["rows"][2], 64, seed=1)
    _check(_logits(s["n_seg"], 100, device, seed=2, ld=100), s["tables"][:2], idx.to(device), 1, 64, n_valid)


def test_summation_order_of_a_hand_built_tree(device):
    """One coarse voxel with all 8 children at both levels and one with a single child; +-1e8 among O(1) terms.  The case
    pins the order: in numpy f32, with the chain's order, reversing the child slots of either level changes mask bytes;
    the chain's bytes are the numpy ones (every mean is 0 or at least 2^-8 in magnitude), and the new entry's are the
    chain's."""
    logits, tabs = cases.order_tree()
    want = cases.emulate_chain(logits, tabs)
    for rev in ((0,), (1,)):
        assert int((cases.emulate_chain(logits, tabs, reverse=rev) != want).sum()) >= 1, rev
    lg = torch.from_numpy(logits).to(device)
    tb = [torch.from_numpy(t).to(device) for t in tabs]
    idx = torch.tensor([0, 1], dtype=torch.int64, device=device)
    got, got_pre, pooled = _check(lg, tb, idx, 1, 2, [2])
    assert np.array_equal(pooled.cpu().numpy(), want)
    assert np.array_equal(got_pre[0].cpu().numpy(), want)
    # the single-child voxel alone, and the full one alone
    for row in (0, 1):
        _check(lg, tb, idx[row:row + 1].contiguous(), 1, 1, [1])
