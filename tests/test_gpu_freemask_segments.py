"""GPU: FreeMask segment mode — the kernels of csrc/freemask_segments.hip, the weighted NMS of csrc/freemask.hip and
their host layer (unscene3d_amd/pseudo_masks/freemask.py: freemask_segments*) against numpy (union-find, floor-divided
coordinates), the float64 restatement tests/freemask_segment_ref.py and the reference's own run
(tests/golden/freemask_segments.npz).

Bounds.  Labels, counts, bits and NMS decisions are integers: exact.  Soft sums of the split rows: 1e-5 relative
against the f64 sum over the device's own labels (the bound of test_gpu_freemask.py's soft_sum).  End to end: 1e-5 on
maskness and soft rows, the bound of the voxel-mode golden; the generator's decision margins are wider.
Both modes' entry points also return the bits recorded before their selection tail and scene layer became one
(tests/golden/freemask_bits.json, recorded on the parent commit): no tolerance."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import freemask_ref as FR
import freemask_segment_ref as SR
from unscene3d_amd import ops
from unscene3d_amd.pseudo_masks import freemask as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "freemask_segments.npz")
SIZES = [1, 2, 63, 64, 65, 129, 200]


def unpack(bits, K):
    b = np.ascontiguousarray(bits.cpu().numpy()).view(np.uint8)
    return np.unpackbits(b, axis=1, bitorder="little").astype(bool)[:, :K]


def pack(masks):
    n, K = masks.shape
    W = (K + 63) // 64
    m = np.zeros((n, W * 64), bool)
    m[:, :K] = masks
    return np.packbits(m, axis=1, bitorder="little").view(np.int64).reshape(n, W)


def golden_params(z):
    p = {k[len("param_"):]: float(z[k]) for k in z.files if k.startswith("param_")}
    for k in ("min_mask_segments", "min_part_segments", "max_instance_num"):
        p[k] = int(p[k])
    return p


# ------------------------------------------------------------------------------------------------------- max pooling
def pooling_case(seed, n_parents=300, top=(1 << 24) - 1):
    """Unique input voxels with ids up to `top`: parents with one present child, with all eight, and in between."""
    rng = np.random.default_rng(seed)
    parents = np.unique(rng.integers(-20, 20, (n_parents, 3)), axis=0) * 4
    offs = np.array([[i, j, k] for i in range(4) for j in range(4) for k in range(4)])
    coords = []
    for i, p in enumerate(parents):
        n = 1 if i % 3 == 0 else (64 if i % 3 == 1 else rng.integers(2, 64))
        coords.append(p + offs[rng.permutation(64)[:n]])
    coords = np.concatenate(coords)
    coords = coords[rng.permutation(len(coords))]
    ids = rng.integers(0, top + 1, len(coords))
    ids[:4] = [top, 0, top, 1]
    return coords.astype(np.int32), ids.astype(np.int64)


@pytest.mark.gpu
def test_maxpool_one_and_two_levels_against_numpy(device):
    from unscene3d_amd import MinkowskiEngine as ME
    coords, ids = pooling_case(3)
    bc = torch.from_numpy(np.concatenate([np.zeros((len(coords), 1), np.int32), coords], 1)).cuda()
    x = ME.SparseTensor(features=torch.from_numpy(ids).cuda().view(-1, 1), coordinates=bc)
    assert x.F.shape[0] == len(coords)
    pool = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)
    avg = ME.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=3)
    ones = ME.SparseTensor(features=torch.ones((len(coords), 1), device="cuda"), coordinate_manager=x.coordinate_manager,
                           coordinate_map_key=x.coordinate_map_key)
    children = []
    for level in (1, 2):
        x, ones = pool(x), avg(ones)
        assert x.coordinate_map_key == ones.coordinate_map_key and x.F.shape == ones.F.shape    # the same rows
        assert x.F.dtype == torch.int64
        want_c, want = SR.maxpool_ids(coords, ids, level)
        got_c = x.C[:, 1:].cpu().numpy()
        order = np.lexsort(got_c.T[::-1])
        assert np.array_equal(got_c[order], want_c)
        assert np.array_equal(x.F.cpu().numpy().ravel()[order], want)
        nbr2 = x.coordinate_manager.stride_map(2 ** (level - 1))["nbr2"]
        children.append((nbr2 >= 0).sum(0).cpu().numpy())
    assert children[0].min() == 1 and children[0].max() == 8 and int(want.max()) == (1 << 24) - 1
    # a float column holding exact integers gives the same rows, as floats
    xf = ME.SparseTensor(features=torch.from_numpy(ids).cuda().view(-1, 1).double(), coordinates=bc)
    assert torch.equal(pool(pool(xf)).F, x.F.double())
    with pytest.raises(RuntimeError, match="exact integers"):
        pool(ME.SparseTensor(features=torch.full((len(coords), 1), 0.5, device="cuda"), coordinates=bc))
    with pytest.raises(NotImplementedError):
        ME.MinkowskiMaxPooling(kernel_size=3, stride=2, dimension=3)


@pytest.mark.gpu
def test_maxpool_refuses_ids_outside_24_bits(device):
    nbr2 = torch.full((8, 2), -1, dtype=torch.int32, device="cuda")
    nbr2[0, 0], nbr2[3, 0], nbr2[1, 1] = 0, 1, 2
    ok = torch.tensor([5, (1 << 24) - 1, 7], device="cuda")
    assert ops.maxpool_down2_i32(ok, nbr2).tolist() == [(1 << 24) - 1, 7]
    assert ops.maxpool_down2_i32(ok.int().view(-1, 1), nbr2).tolist() == [[(1 << 24) - 1], [7]]
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\^24\)"):
        ops.maxpool_down2_i32(torch.tensor([5, 1 << 24, 7], device="cuda"), nbr2)
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\^24\)"):
        ops.maxpool_down2_i32(torch.tensor([5, -1, 7], device="cuda"), nbr2)


# -------------------------------------------------------------------------------------------------------- components
def graph_cases(S):
    """name -> (pairs int[P,2] over vertex numbers 0..S-1, mask bool[S])"""
    full = np.ones(S, bool)
    v = np.arange(S)
    out = {"path": (np.stack([v[:-1], v[1:]], 1), full)}        # label 0 has S - 1 hops to travel
    zig = np.empty(S, np.int64)                                 # the path 0, S-1, 1, S-2, ...: small labels far apart
    zig[0::2], zig[1::2] = v[:(S + 1) // 2], v[::-1][:S // 2]
    out["zigzag_path"] = (np.stack([zig[:-1], zig[1:]], 1), full)
    out["ring"] = (np.stack([v, (v + 1) % S], 1), full)
    out["star"] = (np.stack([np.full(S, S - 1), v], 1), full)   # the hub has the largest number
    if S >= 5:
        h = S // 2                                              # cliques 0..h-1 and h+1..S-1, joined only through h
        a, b = np.meshgrid(v[:h], v[:h])
        c, d = np.meshgrid(v[h + 1:], v[h + 1:])
        bridge = np.array([[h - 1, h], [h, h + 1]])
        mask = full.copy()
        mask[h] = False
        out["two_cliques_bridge_outside"] = (np.concatenate([np.stack([a.ravel(), b.ravel()], 1),
                                                             np.stack([c.ravel(), d.ravel()], 1), bridge]), mask)
    return out


def device_components(pairs, masks, ids):
    adj_off, adj = fm.segment_adjacency(torch.from_numpy(ids[pairs.reshape(-1, 2)]), torch.from_numpy(ids).cuda())
    bits = torch.from_numpy(pack(masks)).cuda()
    label, ncomp = fm.mask_components(bits, torch.arange(len(masks)), adj_off, adj)
    return label, ncomp, adj_off, adj, bits


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_component_labels_against_union_find(device, S):
    ids = np.arange(S, dtype=np.int64) * 3 + 5
    for name, (pairs, mask) in graph_cases(S).items():
        label, ncomp, *_ = device_components(pairs, mask[None], ids)
        want = SR.components(mask, SR.undirected_adjacency(ids[pairs], ids))
        assert np.array_equal(label.cpu().numpy()[0], want), (S, name)
        assert int(ncomp[0]) == len(np.unique(want[want >= 0])), (S, name)
        if name in ("path", "zigzag_path", "ring", "star"):
            assert int(ncomp[0]) == 1 and (want == 0).all()
        else:
            assert int(ncomp[0]) == 2


@pytest.mark.gpu
def test_component_adjacency_handling(device):
    ids = np.array([10, 20, 30, 40, 50, 60], np.int64)
    # one-directional pairs only, in "descending" direction; a self pair; pairs naming unknown ids 99 and 5
    conn = np.array([[30, 10], [40, 30], [60, 50], [20, 20], [20, 99], [5, 60], [99, 5]], np.int64)
    adj_off, adj = fm.segment_adjacency(torch.from_numpy(conn), torch.from_numpy(ids).cuda())
    assert adj_off.tolist() == [0, 1, 1, 3, 4, 5, 6] and adj.tolist() == [2, 0, 3, 2, 5, 4]
    bits = torch.from_numpy(pack(np.ones((1, 6), bool))).cuda()
    label, ncomp = fm.mask_components(bits, torch.tensor([0]), adj_off, adj)
    assert label.tolist() == [[0, 1, 0, 0, 4, 4]] and ncomp.tolist() == [3]
    # no pairs at all: every segment its own part
    off0, adj0 = fm.segment_adjacency(np.zeros((0, 2), np.int64), torch.from_numpy(ids).cuda())
    label, ncomp = fm.mask_components(bits, torch.tensor([0]), off0, adj0)
    assert label.tolist() == [[0, 1, 2, 3, 4, 5]] and ncomp.tolist() == [6]
    # an out-of-range CSR index raises on the host: the outputs are never allocated, nothing is launched
    for bad in (6, -1):
        broken = adj.clone()
        broken[2] = bad
        with pytest.raises(RuntimeError, match="adjacency index outside"):
            fm.mask_components(bits, torch.tensor([0]), adj_off, broken)
    with pytest.raises(RuntimeError, match="rise from 0"):
        fm.mask_components(bits, torch.tensor([0]), adj_off.flip(0).contiguous(), adj)
    with pytest.raises(RuntimeError, match="row index"):
        fm.mask_components(bits, torch.tensor([1]), adj_off, adj)
    cap = fm.lib.usc_mask_bits_max_segments()
    with pytest.raises(RuntimeError, match="LDS"):
        fm.mask_components(torch.zeros((1, (cap + 64) // 64), dtype=torch.int64, device="cuda"), torch.tensor([0]),
                           torch.zeros(cap + 2, dtype=torch.int64, device="cuda"),
                           torch.zeros(0, dtype=torch.int32, device="cuda"))


def random_graph(S, seed, n_rows):
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, S, (int(1.2 * S), 2))
    masks = rng.random((n_rows, S)) < rng.uniform(0.2, 0.9, (n_rows, 1))
    masks[1], masks[2] = False, True                            # an empty and a full row among the others
    return pairs, masks


@pytest.mark.gpu
def test_component_rows_and_repeatability(device):
    S, n = 130, 9
    ids = np.arange(S, dtype=np.int64)
    pairs, masks = random_graph(S, 11, n)
    label, ncomp, adj_off, adj, bits = device_components(pairs, masks, ids)
    adj_sets = SR.undirected_adjacency(pairs, ids)
    for r in range(n):
        want = SR.components(masks[r], adj_sets)
        assert np.array_equal(label.cpu().numpy()[r], want), r
        assert int(ncomp[r]) == len(np.unique(want[want >= 0]))
    assert int(ncomp[1]) == 0 and (label[1] == -1).all() and int(ncomp[2]) >= 1
    # a subset of the rows, in another order
    rows = torch.tensor([2, 0, 2, 8])
    l2, n2 = fm.mask_components(bits, rows, adj_off, adj)
    assert torch.equal(l2, label[rows.cuda()]) and torch.equal(n2, ncomp[rows.cuda()])
    l3, n3 = fm.mask_components(bits, torch.arange(n), adj_off, adj)
    assert torch.equal(l3, label) and torch.equal(n3, ncomp)    # two runs, identical bits


# ------------------------------------------------------------------------------------------------------------- split
@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 64, 130, 200])
def test_split_against_numpy_on_the_device_labels(device, S):
    n = 12
    ids = np.arange(S, dtype=np.int64)
    pairs, masks = random_graph(S, 100 + S, n)
    label, ncomp, *_ = device_components(pairs, masks, ids)
    rng = np.random.default_rng(S)
    w = rng.integers(1, 40, S).astype(np.int32)
    soft = rng.random((n + 3, S)).astype(np.float32)
    soft_row = rng.permutation(n + 3)[:n]
    sp = fm.mask_split(label, ncomp, torch.from_numpy(w).cuda(), torch.from_numpy(soft).cuda(),
                       torch.from_numpy(soft_row))
    lab = label.cpu().numpy()
    want = [(r, root) for r in range(n) for root in np.unique(lab[r][lab[r] >= 0])]     # (row, root) order
    assert len(want) == int(ncomp.sum()) == sp.bits.shape[0] and (len(want) > n or S < 64)
    assert list(zip(sp.src.tolist(), sp.root.tolist())) == want
    got_bits = unpack(sp.bits, S)
    assert sp.bits.shape[1] == (S + 63) // 64
    worst = 0.0
    for o, (r, root) in enumerate(want):
        part = lab[r] == root
        assert np.array_equal(got_bits[o], part)
        assert int(sp.seg_counts[o]) == part.sum() and int(sp.vox_counts[o]) == int(w[part].sum())
        exact = soft[soft_row[r]].astype(np.float64)[part].sum()
        worst = max(worst, abs(float(sp.soft_sums[o]) - exact) / exact)
    print(f"S = {S}: {len(want)} rows, worst relative soft-sum error {worst:.3g}")
    assert worst <= 1e-5
    with pytest.raises(RuntimeError, match="2\\^24"):
        fm.mask_split(label, ncomp, torch.full((S,), 1 << 22, dtype=torch.int32, device="cuda"),
                      torch.from_numpy(soft).cuda(), torch.from_numpy(soft_row))
    # the padding bits of the last word stay clear
    assert not np.unpackbits(np.ascontiguousarray(sp.bits.cpu().numpy()).view(np.uint8), axis=1,
                             bitorder="little")[:, S:].any()


# ------------------------------------------------------------------------------------------------------ weighted NMS
def weighted_case(n, S=100, seed=0):
    rng = np.random.default_rng(seed + n)
    w = np.where(rng.random(S) < 0.3, rng.integers(20, 60, S), rng.integers(1, 4, S)).astype(np.int32)
    protos = rng.random((4, S)) < 0.4
    m = protos[rng.integers(0, 4, n)] ^ (rng.random((n, S)) < rng.choice([0.0, 0.05, 0.15, 0.3], (n, 1)))
    if n >= 64:
        m[7] = False
        m[50] = m[3]
    return m, w


def differing_pairs(m, w, thr=0.5):
    """Pairs the voxel-level greedy loop compares whose decision differs between segment counts and voxel counts."""
    alive, differ = np.ones(len(m), bool), 0
    for i in range(len(m)):
        if not alive[i]:
            continue
        for j in range(i + 1, len(m)):
            if not alive[j]:
                continue
            both = m[i] & m[j]
            vi, vu = int(w[both].sum()), int(w[m[i]].sum() + w[m[j]].sum() - w[both].sum())
            si, su = int(both.sum()), int(m[i].sum() + m[j].sum() - both.sum())
            kv = np.float32(vi) / np.float32(vu) > np.float32(thr) if vu > 0 else True
            ks = np.float32(si) / np.float32(su) > np.float32(thr) if su > 0 else True
            differ += kv != ks
            if kv:
                alive[j] = False
    return differ


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_weighted_nms_against_the_loop_on_expanded_masks(device, n):
    m, w = weighted_case(n)
    if n > 1:
        assert differing_pairs(m, w) >= 1
    expanded = np.repeat(m, w, axis=1)                          # voxel level: segment s becomes w[s] voxels
    vox = expanded.sum(1).astype(np.int32)
    bits, dw = torch.from_numpy(pack(m)).cuda(), torch.from_numpy(w).cuda()
    rng = np.random.default_rng(n)
    for order in (np.arange(n), rng.permutation(n)):
        want = FR.greedy_nms(expanded[order], vox[order], 0.5)
        keep = fm.mask_nms_weighted(bits, torch.from_numpy(vox).cuda(), dw, torch.from_numpy(order.astype(np.int32)), 0.5)
        assert keep.cpu().numpy().tolist() == want.tolist()
    if n > 1:   # and the unweighted rule on the same rows decides otherwise
        plain = fm.mask_nms(bits, torch.from_numpy(m.sum(1).astype(np.int32)).cuda(), torch.arange(n), 0.5)
        assert plain.cpu().numpy().tolist() != FR.greedy_nms(expanded, vox, 0.5).tolist()
    with pytest.raises(RuntimeError, match="2\\^24"):
        fm.mask_nms_weighted(bits, torch.from_numpy(vox).cuda(), torch.full_like(dw, 1 << 20), torch.arange(n), 0.5)


@pytest.mark.gpu
def test_unweighted_nms_is_unchanged_and_is_the_unit_weight_case(device):
    import test_gpu_freemask as TF
    for name, m in TF.NMS.items():
        n, K = m.shape
        counts = m.sum(1).astype(np.int32)
        bits, dc = torch.from_numpy(TF.pack(m)).cuda(), torch.from_numpy(counts).cuda()
        rng = np.random.default_rng(n)
        for order in (np.arange(n), rng.permutation(n)):
            want = FR.greedy_nms(m[order], counts[order], 0.5)
            o = torch.from_numpy(order.astype(np.int32))
            plain = fm.mask_nms(bits, dc, o, 0.5)
            unit = fm.mask_nms_weighted(bits, dc, torch.ones(K, dtype=torch.int32, device="cuda"), o, 0.5)
            assert plain.cpu().numpy().tolist() == want.tolist(), name
            assert torch.equal(plain, unit), name
            assert torch.equal(unit, fm.mask_nms(bits, dc, o, 0.5, weight=torch.ones(K, dtype=torch.int32, device="cuda")))


# -------------------------------------------------------------------------------------------------------- end to end
def assert_golden(z, soft, maskness, query, root, columns=None):
    assert query.cpu().tolist() == z["query_segment"].tolist()  # the reference's survivors in the reference's order
    assert root.cpu().tolist() == z["part_root"].tolist()
    want = z["soft_masks"] if columns is None else z["soft_masks"][:, columns]
    got = soft.cpu().numpy()
    print("maskness err", np.abs(maskness.cpu().numpy() - z["maskness"]).max(), "soft err", np.abs(got - want).max())
    assert np.abs(maskness.cpu().numpy() - z["maskness"]).max() <= 1e-5
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5


@pytest.mark.gpu
def test_end_to_end_on_the_reference_run(device):
    z = np.load(GOLDEN)
    p = golden_params(z)
    args = (torch.from_numpy(z["key_feats"]).cuda(), torch.from_numpy(z["key_coords"]).cuda(),
            torch.from_numpy(z["key_segment_ids"]).cuda(), torch.from_numpy(z["seg_connectivity"]),
            torch.from_numpy(z["scene_extent"]))
    r = fm.freemask_segments(*args, **p)
    assert_golden(z, r.soft_masks, r.maskness, r.query_segment, r.part_root)
    r2 = fm.freemask_segments(*args, **p)
    assert all(torch.equal(a, b) for a, b in zip(r, r2))        # two runs, identical bits
    # no candidates / nothing above the maskness threshold -> empty tensors
    for kw in (dict(min_mask_segments=10 ** 6), dict(min_part_segments=10 ** 6), dict(nms_maskness_threshold=2.0)):
        e = fm.freemask_segments(*args, **kw)
        assert e.soft_masks.shape == (0, len(z["key_feats"])) and e.maskness.numel() == 0
        assert e.query_segment.numel() == 0 and e.part_root.numel() == 0
    for kw, what in ((dict(use_fps_sampling=True), "farthest-point sampling"),
                     (dict(similarity_metric="l2"), "'l2' has none"), (dict(frame_fusion="max"), "stays with the caller")):
        with pytest.raises(NotImplementedError, match=what):
            fm.freemask_segments(*args, **kw)


@pytest.mark.gpu
def test_end_to_end_from_input_voxels_and_ids(device):
    z = np.load(GOLDEN)
    p = golden_params(z)
    feats = torch.from_numpy(z["key_feats"][z["in_parent"]]).cuda()
    r = fm.freemask_segments_from_voxel_feats(torch.from_numpy(z["in_coords"]).cuda(), feats,
                                              torch.from_numpy(z["in_segment_ids"]), z["seg_connectivity"], 2, **p)
    assert r.tensor_stride == 2 and r.key_coords.shape == z["key_coords"].shape
    dev_order = np.lexsort(r.key_coords.cpu().numpy().T[::-1])
    gold_order = np.lexsort(z["key_coords"].T[::-1])
    assert np.array_equal(r.key_coords.cpu().numpy()[dev_order], z["key_coords"][gold_order])
    columns = np.empty(len(dev_order), np.int64)
    columns[dev_order] = gold_order                             # device column c is golden column columns[c]
    assert_golden(z, r.soft_masks, r.maskness, r.query_segment, r.part_root, columns)
    # the scene-list driver takes the per-scene function through its scene_fn hook
    from unscene3d_amd.pseudo_masks.driver import PseudoMaskDriver
    scene = dict(coords=torch.from_numpy(z["in_coords"]).cuda(), feats=feats, segment_ids=z["in_segment_ids"],
                 seg_connectivity=z["seg_connectivity"])
    out = PseudoMaskDriver(device=device, concurrent=2, scene_fn=fm.freemask_segments_scene_fn).run([scene])
    assert torch.equal(out[0].soft_masks, r.soft_masks) and torch.equal(out[0].part_root, r.part_root)
    with pytest.raises(KeyError, match="seg_connectivity"):
        fm.freemask_segments_scene_fn({k: v for k, v in scene.items() if k != "seg_connectivity"})


@pytest.mark.gpu
def test_scene_branch_pools_the_ids_onto_the_backbone_map(device):
    """3D branch: keys = the backbone's res_2 map; the ids of the input voxels are max-pooled once over the same
    coordinate manager.  Equal to the direct call with numpy-pooled ids, whatever the (untrained) features give."""
    from types import SimpleNamespace
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd.models.res16unet import Res16UNet34CMultiRes
    from unscene3d_amd.synthetic import make_scene
    sc = make_scene(1000, target_voxels=3000, tol=0.1)
    vox = np.floor(sc["xyz"] / 0.02).astype(np.int64)
    _, first = np.unique(vox, axis=0, return_index=True)
    first.sort()
    coords, ids = vox[first].astype(np.int32), sc["segment_ids"][first].astype(np.int64)
    conn = np.asarray(sc["segment_connectivity"], np.int64)
    torch.manual_seed(0)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    model = Res16UNet34CMultiRes(3, 20, cfg, out_fpn=True).to("cuda").eval()
    bc = torch.from_numpy(np.concatenate([np.zeros((len(coords), 1), np.int32), coords], 1)).cuda()
    sinput = ME.SparseTensor(features=torch.from_numpy(sc["colors"][first]).float().cuda(), coordinates=bc)
    with torch.no_grad():
        cached = model(sinput)
    kw = dict(nms_maskness_threshold=0.0)
    r = fm.freemask_segments_scene(lambda x: cached, sinput, ids, conn, 2, **kw)
    keys = cached[1]["res_2"]
    kc = keys.C[:, 1:].cpu().numpy()
    want_c, want_ids = SR.maxpool_ids(coords, ids, 1)
    order = np.lexsort(kc.T[::-1])
    assert np.array_equal(kc[order], want_c)
    key_ids = np.empty(len(kc), np.int64)
    key_ids[order] = want_ids
    d = fm.freemask_segments(keys.F.detach().float().contiguous(), keys.C[:, 1:].contiguous(),
                             torch.from_numpy(key_ids).cuda(), conn, (bc[:, 1:].amax(0) - bc[:, 1:].amin(0)).float(), **kw)
    assert r.tensor_stride == 2 and torch.equal(r.key_coords, keys.C[:, 1:])
    assert torch.equal(r.soft_masks, d.soft_masks) and torch.equal(r.maskness, d.maskness)
    assert torch.equal(r.query_segment, d.query_segment) and torch.equal(r.part_root, d.part_root)
    assert r.soft_masks.shape[1] == len(kc)
    with pytest.raises(NotImplementedError, match="'l2' has none"):
        fm.freemask_segments_scene(None, None, ids, conn, 2, similarity_metric="l2")


@pytest.mark.gpu
def test_tool_segment_mode_on_a_synthetic_scene(device, tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("pseudo_masks_run", os.path.join(ROOT, "tools", "pseudo_masks_run.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    sdir = str(tmp_path / "scenes")
    (path,) = tool.synthetic_scene_files(1, sdir)
    z = np.load(path)
    name = os.path.splitext(os.path.basename(path))[0]
    out = str(tmp_path / "seg")
    saved, real_save = [], np.save

    def recording_save(file, arr, *a, **kw):
        saved.append(os.path.basename(str(file)))
        return real_save(file, arr, *a, **kw)

    monkeypatch.setattr(tool.np, "save", recording_save)
    assert tool.main(["--scenes", sdir, "--out", out, "--method", "freemask", "--freemask-mode", "segment"]) == 0
    monkeypatch.setattr(tool.np, "save", real_save)
    assert saved == [f"{name}_masks.npy", f"{name}_cloud.npy"]  # the cloud file, the "done" marker, is written last
    masks_file, cloud_file = os.path.join(out, f"{name}_masks.npy"), os.path.join(out, f"{name}_cloud.npy")
    masks, cloud = np.load(masks_file), np.load(cloud_file)
    full = z["full_res_coords"]
    assert masks.dtype == np.float32 and masks.shape[0] == len(full) and masks.shape[1] >= 1
    assert cloud.shape == full.shape
    r = fm.freemask_segments_from_voxel_feats(torch.from_numpy(z["coords"]).cuda(), torch.from_numpy(z["feats_2d"]).cuda(),
                                              z["segment_ids"], z["seg_connectivity"], 2)
    lifted = fm.soft_masks_to_full_resolution(r.key_coords, r.tensor_stride, full, float(z["voxel_size"]), r.soft_masks)
    assert np.array_equal(masks, lifted)
    # a scene file without the segment arrays: the tool names the missing key; voxel mode does not need them
    bare = str(tmp_path / "bare")
    os.makedirs(bare)
    np.savez(os.path.join(bare, "scene9999_00.npz"), **{k: z[k] for k in z.files if k != "seg_connectivity"})
    with pytest.raises(RuntimeError, match="seg_connectivity"):
        tool.main(["--scenes", bare, "--out", str(tmp_path / "o2"), "--method", "freemask", "--freemask-mode", "segment"])
    assert tool.main(["--scenes", bare, "--out", str(tmp_path / "o3"), "--method", "freemask"]) == 0


# -------------------------------------------------------------------------------------------------------------- bits
def _sha(fields):
    h = hashlib.sha256()
    for t in fields:
        if not torch.is_tensor(t):                              # tensor_stride
            h.update(repr(t).encode())
            continue
        t = t.detach().cpu().contiguous()
        h.update(str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def freemask_bits(scene_dir):
    """name -> sha256 over every field of the result, for both modes: the golden parameters, a cut at 3 masks, a scene
    extent so small that no mask passes the extent filter (all stay), and the scene-level entry points."""
    spec = importlib.util.spec_from_file_location("pseudo_masks_run", os.path.join(ROOT, "tools", "pseudo_masks_run.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    import test_freemask_host as TH
    bits = {}
    v = np.load(TH.GOLDEN)
    vp = TH._params(v)
    vargs = [torch.from_numpy(v[k]).cuda() for k in ("key_feats", "key_coords", "query_feats")]
    z = np.load(GOLDEN)
    sp = golden_params(z)
    sargs = [torch.from_numpy(z["key_feats"]).cuda(), torch.from_numpy(z["key_coords"]).cuda(),
             torch.from_numpy(z["key_segment_ids"]).cuda(), torch.from_numpy(z["seg_connectivity"])]
    for name, scale, over in (("golden", 1.0, {}), ("cut_3", 1.0, dict(max_instance_num=3)), ("all_stay", 1e-3, {})):
        bits[f"voxel_{name}"] = _sha(fm.freemask(*vargs, torch.from_numpy(v["scene_extent"] * np.float32(scale)),
                                                 **{**vp, **over}))
        bits[f"segment_{name}"] = _sha(fm.freemask_segments(*sargs, torch.from_numpy(z["scene_extent"] * np.float32(scale)),
                                                            **{**sp, **over}))
    bits["segment_from_voxel_feats"] = _sha(fm.freemask_segments_from_voxel_feats(
        torch.from_numpy(z["in_coords"]).cuda(), torch.from_numpy(z["key_feats"][z["in_parent"]]).cuda(),
        torch.from_numpy(z["in_segment_ids"]), z["seg_connectivity"], 2, **sp))
    (path,) = tool.synthetic_scene_files(1, scene_dir)
    y = np.load(path)
    bits["voxel_from_voxel_feats"] = _sha(fm.freemask_from_voxel_feats(torch.from_numpy(y["coords"]).cuda(),
                                                                       torch.from_numpy(y["feats_2d"]).cuda(), 2))
    return bits


@pytest.mark.gpu
def test_both_modes_compute_the_recorded_bits(device, tmp_path):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "freemask_bits.json")))
    assert freemask_bits(str(tmp_path / "scenes")) == want


# ------------------------------------------------------------------------------------------------------------ memory
@pytest.mark.gpu
def test_nothing_of_size_rows_by_voxels(device):
    """The golden scene with every key voxel listed 8 times: S = 81 segments, R = 121 rows after the split and the
    small-part cut, K = 8 x 1244 voxels, so R K 4 bytes is far above 8 S^2 4 bytes.  The peak of the allocations above
    the inputs must stay below ONE f32 [R, K] matrix (the reference holds three: separated, mapped and its clone)."""
    z = np.load(GOLDEN)
    p = golden_params(z)
    dbg = {}
    SR.freemask_segments_ref(z["key_feats"], z["key_coords"], z["key_segment_ids"], z["seg_connectivity"],
                             z["scene_extent"], debug=dbg, **p)
    rep = 8
    fk = torch.from_numpy(np.repeat(z["key_feats"], rep, 0)).cuda()
    kc = torch.from_numpy(np.repeat(z["key_coords"], rep, 0)).cuda()
    ids = torch.from_numpy(np.repeat(z["key_segment_ids"], rep, 0)).cuda()
    conn = torch.from_numpy(z["seg_connectivity"]).cuda()
    ext = torch.from_numpy(z["scene_extent"]).cuda()
    R, S, K = len(dbg["rows"]), len(dbg["unique_segments"]), fk.shape[0]
    assert R * K * 4 >= 8 * S * S * 4
    fm.freemask_segments(fk[:64], kc[:64], ids[:64], conn, ext, **p)       # (library and allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fm.freemask_segments(fk, kc, ids, conn, ext, **p)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak additional memory {extra} bytes = {extra / (R * K * 4):.3f} of one f32 [R = {R}, K = {K}]")
    assert r.query_segment.cpu().tolist() == z["query_segment"].tolist()
    assert extra < R * K * 4
