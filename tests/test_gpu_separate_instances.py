"""GPU: `general.separate_instances` (csrc/separate.hip, trainer/separate.py) against the numpy restatement
tests/separate_ref.py and the reference's own parts (tests/golden/separate_instances.npz).  Everything compared is an
integer or a bit: every comparison is exact.

  columns -> segment bits   N = 1000, K in {1, 64, 70}, S in {1, 64, 65, 130}
  components                the wide kernel forced at small S = the LDS kernel; S = 8193 and an 8200-vertex path = union-find
  parts -> columns          R in {0, 1, 65}
  golden                    the reference's parts, the stated order
  export_instances          union of parts = input, repeated scores / classes / boxes, flag off = today's bytes, no instance
  eval_step                 two synthetic scenes, written files in both formats
  reader                    resegment_mesh on a two-box PLY, the stored-connectivity route through build_dataset
  memory                    peak above the inputs <= bits + labels + result"""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import dataset_cases as D
import separate_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "separate_instances.npz")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------- columns -> bits
def planted_columns(N, K, S, seed):
    """idx with every segment present, segment S-1 of ONE point, segment 0 large; column 0 sets a single point of the
    large segment, column 1 (if any) is empty, column 2 (if any) is exactly the one-point segment; the rest random."""
    rng = np.random.default_rng(seed)
    idx = np.zeros(N, np.int64)
    idx[:S] = np.arange(S)
    if S > 1:
        body = rng.integers(0, S - 1, N - S)
        body[rng.random(N - S) < 0.3] = 0
        idx[S:] = body
    idx = idx[rng.permutation(N)]
    masks = rng.random((N, K)) < 0.01
    masks[:, 0] = False
    masks[np.nonzero(idx == 0)[0][-1], 0] = True
    if K > 1:
        masks[:, 1] = False
    if K > 2:
        masks[:, 2] = idx == S - 1
    return idx, masks


@pytest.mark.parametrize("S", [1, 64, 65, 130])
@pytest.mark.parametrize("K", [1, 64, 70])
def test_columns_to_segment_bits(device, K, S):
    from unscene3d_amd import ops

    N = 1000
    idx, masks = planted_columns(N, K, S, 100 * K + S)
    assert (np.bincount(idx, minlength=S) > 0).all() and (idx == 0).sum() > 1
    assert S == 1 or (idx == S - 1).sum() == 1
    csr = ops.segment_csr(torch.from_numpy(idx).to(device), S)
    want = R.pack_rows(R.segment_masks(masks, idx, S))
    for table in (torch.from_numpy(masks).to(device), torch.from_numpy(masks.astype(np.uint8) * 7).to(device)):
        bits = ops.mask_columns_to_segment_bits(table, csr)
        assert bits.shape == (K, (S + 63) // 64) and bits.dtype == torch.int64
        assert np.array_equal(u64(bits), want)              # the bits past S are zero
    assert int(want[0].sum()) == 1                          # one point of the large segment sets bit 0 alone
    if K > 1:
        assert not want[1].any()


def test_columns_to_segment_bits_checks_its_csr(device):
    from unscene3d_amd import ops

    masks = torch.zeros((10, 3), dtype=torch.bool, device=device)
    csr = ops.segment_csr(torch.zeros(9, dtype=torch.int64, device=device), 1)
    with pytest.raises(RuntimeError, match="CSR must cover"):
        ops.mask_columns_to_segment_bits(masks, csr)
    csr = ops.segment_csr(torch.zeros(10, dtype=torch.int64, device=device), 1)
    assert ops.mask_columns_to_segment_bits(masks[:, :0].contiguous(), csr).shape == (0, 1)
    # a hand-built CSR with bad VALUES raises on the host, before the launch
    good = ops.segment_csr(torch.tensor([0, 1, 1, 2, 0, 2, 1, 0, 2, 1], device=device), 3)
    for off in ([0, 3, 7, 11], [1, 3, 7, 10], [0, 7, 3, 10]):
        bad = ops.SegmentCSR(good.seg, good.order, torch.tensor(off, dtype=torch.int64, device=device), 3)
        with pytest.raises(RuntimeError, match="seg_off must rise from 0 to 10"):
            ops.mask_columns_to_segment_bits(masks, bad)
    for v in (-1, 10):
        order = good.order.clone()
        order[4] = v
        with pytest.raises(RuntimeError, match="csr.order outside"):
            ops.mask_columns_to_segment_bits(masks, ops.SegmentCSR(good.seg, order, good.seg_off, 3))


# ------------------------------------------------------------------------------------------------------ components
def random_case(S, seed, n_rows):
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, S, (int(1.2 * S), 2))
    masks = rng.random((n_rows, S)) < rng.uniform(0.2, 0.9, (n_rows, 1))
    if n_rows > 2:
        masks[1], masks[2] = False, True                    # an instance with no segment, and a full one
    return pairs, masks


def device_graph(pairs, S, device):
    from unscene3d_amd.pseudo_masks import freemask as fm

    ids = torch.arange(S, dtype=torch.int64, device=device)
    return fm.segment_adjacency(torch.from_numpy(np.asarray(pairs, np.int64)), ids)


def undirected_sets(pairs, S):
    adj = [set() for _ in range(S)]
    for a, b in pairs:
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return adj


@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_wide_components_equal_the_lds_kernel(device, S):
    from unscene3d_amd.pseudo_masks import freemask as fm

    n = 7
    pairs, masks = random_case(S, 40 + S, n)
    adj_off, adj = device_graph(pairs, S, device)
    bits = torch.from_numpy(R.pack_rows(masks).view(np.int64)).to(device)
    rows = torch.arange(n)
    l0, n0 = fm.mask_components(bits, rows, adj_off, adj)
    l1, n1 = fm.mask_components(bits, rows, adj_off, adj, kernel="wide")
    assert torch.equal(l0, l1) and torch.equal(n0, n1)
    l2, n2 = fm.mask_components(bits, rows, adj_off, adj, kernel="auto")      # below the cap: the LDS kernel
    assert torch.equal(l0, l2) and torch.equal(n0, n2)
    assert int(n1[1]) == 0 and bool((l1[1] == -1).all())   # an instance with no segment
    sets = undirected_sets(pairs, S)
    for r in range(n):
        assert np.array_equal(l1[r].cpu().numpy(), R.components(masks[r], sets)), r
    l3, n3 = fm.mask_components(bits, rows, adj_off, adj, kernel="wide")        # two runs, identical bits
    assert torch.equal(l1, l3) and torch.equal(n1, n3)


def test_wide_components_above_the_lds_cap(device):
    from unscene3d_amd.pseudo_masks import freemask as fm

    cap = fm.lib.usc_mask_bits_max_segments()
    S = cap + 1
    pairs, masks = random_case(S, 7, 3)
    adj_off, adj = device_graph(pairs, S, device)
    bits = torch.from_numpy(R.pack_rows(masks).view(np.int64)).to(device)
    label, ncomp = fm.mask_components(bits, torch.arange(3), adj_off, adj, kernel="auto")
    sets = undirected_sets(pairs, S)
    for r in range(3):
        want = R.components(masks[r], sets)
        assert np.array_equal(label[r].cpu().numpy(), want), r
        assert int(ncomp[r]) == len(np.unique(want[want >= 0]))
    assert int(ncomp[1]) == 0
    with pytest.raises(RuntimeError, match="LDS"):          # the LDS kernel and its cap stay as they are
        fm.mask_components(bits, torch.arange(3), adj_off, adj)


def test_wide_components_on_a_long_path(device):
    """An 8200-vertex path: the longest propagation a graph of this size has.  One part, labelled 0; with one vertex
    taken out of the mask, two."""
    from unscene3d_amd.pseudo_masks import freemask as fm

    S = 8200
    v = np.arange(S)
    pairs = np.stack([v[:-1], v[1:]], 1)
    masks = np.ones((2, S), bool)
    masks[1, 5000] = False
    adj_off, adj = device_graph(pairs, S, device)
    bits = torch.from_numpy(R.pack_rows(masks).view(np.int64)).to(device)
    label, ncomp = fm.mask_components(bits, torch.arange(2), adj_off, adj, kernel="wide")
    sets = undirected_sets(pairs, S)
    for r in range(2):
        assert np.array_equal(label[r].cpu().numpy(), R.components(masks[r], sets)), r
    assert ncomp.tolist() == [1, 2] and bool((label[0] == 0).all())


def test_triple_bridge_is_one_part_on_the_device(device):
    """The deviation on the device: segment 6 joins the blobs {0, 1}, {2, 3} and {4, 5}.  The reference's scan merges the
    first two, pops, advances past the third and leaves two blobs; both kernels and the whole call give ONE part."""
    from unscene3d_amd.pseudo_masks import freemask as fm
    from unscene3d_amd.trainer.separate import separate_instances

    pairs = np.array([(0, 6), (2, 6), (4, 6), (0, 1), (2, 3), (4, 5)])
    adj_off, adj = device_graph(pairs, 7, device)
    masks = np.ones((2, 7), bool)
    masks[1, 6] = False                                     # without the bridge: three parts
    bits = torch.from_numpy(R.pack_rows(masks).view(np.int64)).to(device)
    for kernel in ("lds", "wide"):
        label, ncomp = fm.mask_components(bits, torch.arange(2), adj_off, adj, kernel=kernel)
        assert label.tolist() == [[0] * 7, [0, 0, 2, 2, 4, 4, -1]] and ncomp.tolist() == [1, 3], kernel
    ids = np.array([3, 8, 9, 20, 21, 40, 77])
    seg = np.repeat(ids, 4)
    conn = ids[np.concatenate([pairs, pairs[:, ::-1]])]
    table = torch.from_numpy(np.stack([np.ones(28, bool), seg != 77], 1)).to(device)
    out, src = separate_instances(table, seg, conn)
    assert src.tolist() == [0, 1, 1, 1] and bool(out[:, 0].all())
    want, want_src, _, _ = R.separate_ref(table.cpu().numpy(), seg, conn)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), want_src)
    with pytest.raises(ValueError, match="kernel must be"):
        fm.mask_components(bits, torch.arange(2), adj_off, adj, kernel=True)


def test_wide_components_refuse_above_their_cap(device):
    from unscene3d_amd.pseudo_masks import freemask as fm

    S = fm.lib.usc_mask_bits_max_segments_wide() + 1
    assert S == 65537
    with pytest.raises(RuntimeError, match="one round is too long"):
        fm.mask_components(torch.zeros((1, (S + 63) // 64), dtype=torch.int64, device=device), torch.tensor([0]),
                           torch.zeros(S + 1, dtype=torch.int64, device=device),
                           torch.zeros(0, dtype=torch.int32, device=device), kernel="auto")


# ------------------------------------------------------------------------------------------------ parts -> columns
@pytest.mark.parametrize("n_parts", [0, 1, 65])
def test_parts_to_columns(device, n_parts):
    from unscene3d_amd import ops

    rng = np.random.default_rng(n_parts)
    n, S, N = 5, 37, 1003
    label = rng.integers(-1, 6, (n, S)).astype(np.int32)
    src = rng.integers(0, n, n_parts).astype(np.int32)
    root = rng.integers(0, 6, n_parts).astype(np.int32)
    idx = rng.integers(0, S, N).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(device)
    out = ops.segment_parts_to_columns(t(label), t(src), t(root), t(idx))
    assert out.dtype == torch.bool and out.shape == (N, n_parts)
    want = label[src][:, idx].T == root[None, :] if n_parts else np.zeros((N, 0), bool)
    assert np.array_equal(out.cpu().numpy(), want)
    if n_parts:
        with pytest.raises(RuntimeError, match="src outside"):
            ops.segment_parts_to_columns(t(label), t(np.full(n_parts, n, np.int32)), t(root), t(idx))
        bad = idx.copy()
        bad[-1] = S
        with pytest.raises(RuntimeError, match="idx outside"):
            ops.segment_parts_to_columns(t(label), t(src), t(root), t(bad))


# ---------------------------------------------------------------------------------------------------------- golden
def test_golden_parts_and_their_order(device):
    from unscene3d_amd.trainer.separate import separate_instances

    z = np.load(GOLDEN)
    masks = torch.from_numpy(z["masks"]).to(device)
    out, src = separate_instances(masks, torch.from_numpy(z["seg"]).to(device), z["conn"])
    want, want_src, parts, uniq = R.separate_ref(z["masks"], z["seg"], z["conn"])
    assert out.dtype == torch.bool and src.dtype == torch.int64
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert np.array_equal(out.cpu().numpy(), want)         # the same columns in the stated order
    got = out.cpu().numpy()
    for j in range(z["masks"].shape[1]):                    # the reference's parts, as sets per instance
        a = {c.tobytes() for c in got[:, want_src == j].T}
        b = {c.tobytes() for c in z["ref_masks"][:, z["ref_src"] == j].T}
        assert a == b, j
    # order: instances ascending, parts by their smallest segment index
    idx = np.searchsorted(uniq, z["seg"])
    roots = np.array([idx[c].min() for c in got.T])
    assert (np.diff(want_src) >= 0).all()
    assert all((np.diff(roots[want_src == j]) > 0).all() for j in range(z["masks"].shape[1]))
    # numpy inputs and a uint8 table give the same
    out2, src2 = separate_instances(masks.view(torch.uint8), z["seg"], torch.from_numpy(z["conn"]))
    assert torch.equal(out, out2) and torch.equal(src, src2)
    # no connectivity: every segment of an instance is a part
    out3, src3 = separate_instances(masks, z["seg"], np.zeros((0, 2), np.int64))
    out4, src4 = separate_instances(masks, z["seg"], [])    # an empty list is no pairs, not a dtype error
    assert torch.equal(out3, out4) and torch.equal(src3, src4)
    assert out3.shape[1] == int(R.segment_masks(z["masks"], idx, len(uniq)).sum())


# ------------------------------------------------------------------------------------------------ export_instances
def export_case(device, z, extra_queries=2):
    """The golden scene as one model output: query q's logits are +5 on instance q's points, the extra queries are empty
    (below the filter), class 0 wins, scores fall with q.  Identity voxelisation, no low-resolution segments."""
    N, K = z["masks"].shape
    Q = K + extra_queries
    logit = np.full((N, Q), -5.0, np.float32)
    logit[:, :K][z["masks"]] = 5.0
    cls = np.zeros((1, Q, 3), np.float32)
    cls[0, :, 0] = 4.0 - 0.3 * np.arange(Q)
    cls[0, :, 1] = -9.0
    cls[0, :, 2] = -9.0
    rng = np.random.default_rng(5)
    coords = rng.random((N, 3)).astype(np.float32) * 4
    output = {"aux_outputs": [], "pred_logits": torch.from_numpy(cls).to(device),
              "pred_masks": [torch.from_numpy(logit).to(device)]}
    full = [{"point2segment": torch.from_numpy(z["seg"]).to(device)}]
    inv = [torch.arange(N, device=device)]
    return output, full, inv, [coords]


def run_export(case, general, **kw):
    from unscene3d_amd.trainer import postprocess as PP

    output, full, inv, coords = case
    return PP.export_instances(output, full, full, inv, None, general, num_classes=3, train_on_segments=False,
                               eval_on_segments=True, label_offset=2, full_res_coords=coords, **kw)[0]


def same_result(a, b):
    assert a["pred_masks"].dtype == b["pred_masks"].dtype and torch.equal(a["pred_masks"], b["pred_masks"])
    assert np.array_equal(a["pred_scores"], b["pred_scores"]) and a["pred_scores"].dtype == b["pred_scores"].dtype
    assert torch.equal(a["pred_classes"], b["pred_classes"])
    assert np.array_equal(a["pred_boxes"], b["pred_boxes"])


def test_export_instances_splits_the_kept_instances(device):
    z = np.load(GOLDEN)
    case = export_case(device, z)
    general = NS(use_dbscan=False, dbscan_eps=0.95, topk_per_image=-1, filter_out_instances=True, scores_threshold=0.1,
                 iou_threshold=0.66)
    base = run_export(case, general)
    kept = base["pred_masks"].cpu().numpy()
    assert 3 <= kept.shape[1] <= z["masks"].shape[1]
    on = NS(**vars(general), separate_instances=True)
    res = run_export(case, on, segment_connectivity=[z["conn"]])
    want, src, _, _ = R.separate_ref(kept, z["seg"], z["conn"])
    got = res["pred_masks"].cpu().numpy()
    assert got.dtype == bool and np.array_equal(got, want) and got.shape[1] > kept.shape[1]
    for j in range(kept.shape[1]):                          # eval_on_segments: whole segments, so the parts tile the input
        assert np.array_equal(got[:, src == j].any(1), kept[:, j]), j
        assert (got[:, src == j].sum(1) <= 1).all()
    assert np.array_equal(res["pred_scores"], base["pred_scores"][src])
    assert torch.equal(res["pred_classes"], base["pred_classes"][torch.from_numpy(src)])
    boxes = res["pred_boxes"]
    assert boxes.shape == (got.shape[1], 8)
    assert np.array_equal(boxes[:, 0], np.asarray(res["pred_classes"], np.float64))
    assert np.array_equal(boxes[:, 7], np.asarray(res["pred_scores"], np.float64))
    xyz = case[3][0].astype(np.float64)
    for r in range(got.shape[1]):                           # boxes of the NEW columns
        pts = xyz[got[:, r]]
        np.testing.assert_allclose(boxes[r, 1:4], pts.mean(0), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(boxes[r, 4:7], pts.max(0) - pts.min(0), rtol=0, atol=1e-6)
    # twice: identical bytes
    same_result(res, run_export(case, on, segment_connectivity=[z["conn"]]))


def test_export_instances_flag_off_or_no_connectivity_is_todays_call(device):
    z = np.load(GOLDEN)
    case = export_case(device, z)
    general = NS(use_dbscan=False, dbscan_eps=0.95, topk_per_image=-1, filter_out_instances=True, scores_threshold=0.1,
                 iou_threshold=0.66)
    base = run_export(case, general)                        # the argument is not passed at all
    same_result(base, run_export(case, general, segment_connectivity=[z["conn"]]))            # no flag
    off = NS(**vars(general), separate_instances=False)
    same_result(base, run_export(case, off, segment_connectivity=[z["conn"]]))
    on = NS(**vars(general), separate_instances=True)
    for conn in (None, [], [[]], [np.zeros((0, 2), np.int64)]):
        same_result(base, run_export(case, on, segment_connectivity=conn))
    same_result(base, run_export(case, on))


def test_export_instances_with_no_kept_instance_is_empty(device):
    z = np.load(GOLDEN)
    case = export_case(device, z)
    general = NS(use_dbscan=False, dbscan_eps=0.95, topk_per_image=-1, filter_out_instances=True, scores_threshold=2.0,
                 iou_threshold=0.66)
    base = run_export(case, general)
    assert base["pred_masks"].shape == (z["masks"].shape[0], 0)
    res = run_export(case, NS(**vars(general), separate_instances=True), segment_connectivity=[z["conn"]])
    same_result(base, res)
    assert res["pred_boxes"].shape[0] == 0 and len(res["pred_scores"]) == 0


# ------------------------------------------------------------------------------------------------------- eval_step
def test_eval_step_writes_the_split_columns(device, tmp_path):
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    ds = SyntheticFreeMaskDataset(n_scenes=2, target_voxels=6000, seed=5150)
    batch = []
    for i in range(2):                                      # hand-made connectivity: chains of three segment ids
        item = list(ds[i])
        ids = np.unique(item[2][:, -1])
        a, b = ids[:-1][np.arange(len(ids) - 1) % 3 != 2], ids[1:][np.arange(len(ids) - 1) % 3 != 2]
        item[8] = np.concatenate([np.stack([a, b], 1), np.stack([b, a], 1), [[ids[0], ids[-1]]]]).astype(np.int32)
        batch.append(tuple(item))
    collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="validation", device=str(device))
    overrides = ["general.num_targets=3", "general.filter_out_instances=true", "general.scores_threshold=0.0",
                 "general.save_for_freemask=true"]
    results = {}
    cfg = apply_overrides(default_config(), overrides)
    torch.manual_seed(11)
    module = InstanceSegmentation(cfg).to(device).eval()
    assert module.config is cfg
    for fmt, flag in (("npy", False), ("npy", True), ("bits", True)):
        save_dir = tmp_path / f"{fmt}_{flag}"
        cfg.general.separate_instances, cfg.general.freemask_format, cfg.general.save_dir = flag, fmt, str(save_dir)
        data, target, names = collate(batch)
        assert [len(c) for c in data.segment_connectivity] == [len(b[8]) for b in batch]
        res = module.eval_step((data, target, names))
        assert res is not None
        results[(fmt, flag)] = (res["instances"], save_dir, names, data)
    plain, _, names, data = results[("npy", False)]
    split, split_dir, _, _ = results[("npy", True)]
    _, bits_dir, _, _ = results[("bits", True)]
    total_kept, grew = 0, 0
    for b, name in enumerate(names):
        kept = plain[b]["pred_masks"].cpu().numpy()
        total_kept += kept.shape[1]
        grew += split[b]["pred_masks"].shape[1] > kept.shape[1]
        seg = data.target_full[b]["point2segment"].cpu().numpy()
        want, src, _, _ = R.separate_ref(kept, seg, batch[b][8])
        assert np.array_equal(split[b]["pred_masks"].cpu().numpy(), want)
        assert np.array_equal(split[b]["pred_scores"], plain[b]["pred_scores"][src])
        written = np.load(split_dir / "freemasks" / f"{name}_masks.npy")
        assert written.dtype == bool and np.array_equal(written, want)
        rows = np.load(bits_dir / "freemasks" / f"{name}_masks_bits.npy")
        assert rows.dtype == np.uint64 and rows.shape == (want.shape[1], (want.shape[0] + 63) // 64)
        unpacked = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :want.shape[0]].T.astype(bool)
        assert np.array_equal(unpacked, want)
        assert not (bits_dir / "freemasks" / f"{name}_masks.npy").exists()
    assert total_kept >= 1                                   # something went through the split ...
    assert grew >= 1                                         # ... and at least one scene came out with more columns


# ---------------------------------------------------------------------------------------------------------- reader
def box_mesh(origin, g=7, size=1.0):
    """The surface of an axis-aligned box as a triangle mesh with g x g vertices per face, shared along the edges."""
    lin = np.linspace(0.0, size, g)
    verts, index, faces = [], {}, []

    def vid(p):
        key = tuple(np.round(p, 6))
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]

    for axis in range(3):
        for side in (0.0, size):
            u, v = [a for a in range(3) if a != axis]
            grid = np.zeros((g, g), np.int64)
            for i in range(g):
                for j in range(g):
                    p = np.zeros(3)
                    p[axis], p[u], p[v] = side, lin[i], lin[j]
                    grid[i, j] = vid(p)
            for i in range(g - 1):
                for j in range(g - 1):
                    faces.append((grid[i, j], grid[i + 1, j], grid[i, j + 1]))
                    faces.append((grid[i + 1, j], grid[i + 1, j + 1], grid[i, j + 1]))
    return np.array(verts, np.float32) + np.asarray(origin, np.float32), np.array(faces, np.int32)


def two_box_scene(tmp_path, subset=False):
    va, fa = box_mesh((0, 0, 0))
    vb, fb = box_mesh((2.5, 0.5, 0))
    vertices, faces = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    rng = np.random.default_rng(9)
    rgb = rng.integers(0, 255, (len(vertices), 3)).astype(np.uint8)
    d = tmp_path / "scans" / "scene0007_00"
    os.makedirs(d, exist_ok=True)
    mesh_path = str(d / "scene0007_00_vh_clean_2.ply")
    D.write_ply(mesh_path, vertices, rgb, faces)
    take = rng.permutation(len(vertices))[: len(vertices) - 40] if subset else np.arange(len(vertices))
    points = np.zeros((len(take), 12), np.float32)
    points[:, :3], points[:, 3:6], points[:, 8], points[:, 9] = vertices[take], rgb[take], 1.0, 5.0
    os.makedirs(tmp_path / "data", exist_ok=True)
    path = str(tmp_path / "data" / ("0007_00_sub.npy" if subset else "0007_00.npy"))
    np.save(path, points)
    soft = np.stack([take < len(va), take >= len(va)], 1).astype(np.float32)
    np.save(path.replace(".npy", "_freemasks.npy"), soft)
    return {"filepath": path, "raw_filepath": mesh_path}, vertices, faces, rgb, take, len(va)


@pytest.mark.parametrize("device_tables", [False, True])
@pytest.mark.parametrize("subset", [False, True])
def test_reader_resegments_the_mesh(device, tmp_path, device_tables, subset):
    from unscene3d_amd import felzenszwalb_cpp
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader
    from unscene3d_amd.pseudo_masks import scans

    entry, vertices, faces, rgb, take, n_a = two_box_scene(tmp_path, subset)
    kw = dict(add_normals=False, add_raw_coordinates=True, device=str(device), device_tables=device_tables)
    v, colors, f = scans.read_ply_mesh(entry["raw_filepath"])
    assert np.array_equal(v, vertices) and np.array_equal(f, faces)
    seg, conn = felzenszwalb_cpp.segment_mesh(v, f, colors, 0.005, 20, device=device)
    assert conn.dtype == np.int32 and conn.ndim == 2 and len(conn) > 0
    assert not set(seg[:n_a]) & set(seg[n_a:])              # two disjoint boxes share no segment ...
    side = np.zeros(seg.max() + 1, bool)
    side[seg[n_a:]] = True
    assert (side[conn[:, 0]] == side[conn[:, 1]]).all()    # ... and no pair crosses
    plain = FreeMaskSceneReader([entry], **kw)[0]
    item = FreeMaskSceneReader([entry], resegment_mesh=True, **kw)[0]
    table = item[2].cpu().numpy() if torch.is_tensor(item[2]) else item[2]
    table0 = plain[2].cpu().numpy() if torch.is_tensor(plain[2]) else plain[2]
    assert np.array_equal(table[:, -1], seg[take]) and table.dtype == np.int32
    assert isinstance(item[8], np.ndarray) and item[8].dtype == np.int32 and np.array_equal(item[8], conn)
    # today's tuple without the flag: the stored segment column and []
    assert plain[8] == [] and (table0[:, -1] == 5).all()
    assert np.array_equal(table[:, :-1], table0[:, :-1])
    for a, b in zip(item[3:8], plain[3:8]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # train mode never re-segments
    off = FreeMaskSceneReader([entry], resegment_mesh=True, mode="train", **kw)[0]
    assert off[8] == []
    # another minimum size is honoured
    item50 = FreeMaskSceneReader([entry], resegment_mesh=True, segment_min_vert_num=50, **kw)[0]
    seg50, conn50 = felzenszwalb_cpp.segment_mesh(v, f, colors, 0.005, 50, device=device)
    table50 = item50[2].cpu().numpy() if torch.is_tensor(item50[2]) else item50[2]
    assert np.array_equal(item50[8], conn50) and np.array_equal(table50[:, -1], seg50[take])


def test_reader_with_an_unreadable_mesh_keeps_the_stored_segments(device, tmp_path, capsys):
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader

    entry, *_ = two_box_scene(tmp_path)
    entry = dict(entry, raw_filepath=str(tmp_path / "scans" / "scene0007_00" / "missing.ply"))
    item = FreeMaskSceneReader([entry], resegment_mesh=True, add_normals=False, device=str(device))[0]
    assert item[8] == [] and (item[2][:, -1] == 5).all()
    assert "Can't segment mesh" in capsys.readouterr().out


def test_stored_connectivity_route(device, tmp_path, monkeypatch):
    """build_dataset(write_connectivity=True) on a scan without segs.json stores what the over-segmentation gave; the
    reader then returns the same item as the per-item route, and the default writes today's files and entries."""
    from unscene3d_amd.datasets import freemask as F
    from unscene3d_amd.datasets.preprocessing import build_dataset

    name = "scene0003_00"
    scan = D.write_scan(str(tmp_path / "scans"), name, seed=31, side=24, gt=False, segs=False)
    D.write_pseudo(str(tmp_path / "pm"), name, scan, seed=31, K=4, compact=True)
    plain = build_dataset(str(tmp_path / "scans"), {"validation": [name]}, str(tmp_path / "pm"), str(tmp_path / "d0"),
                          device=device)["validation"]
    stored = build_dataset(str(tmp_path / "scans"), {"validation": [name]}, str(tmp_path / "pm"), str(tmp_path / "d1"),
                           device=device, write_connectivity=True)["validation"]
    assert "connectivity_filepath" not in plain[0] and "segments_min_verts" not in plain[0]
    assert sorted(os.listdir(tmp_path / "d0" / "validation")) == ["0003_00.npy", "0003_00_freemasks.npy"]
    assert set(stored[0]) == set(plain[0]) | {"connectivity_filepath", "segments_min_verts"}
    assert stored[0]["segments_min_verts"] == 20
    assert np.array_equal(np.load(plain[0]["filepath"]), np.load(stored[0]["filepath"]))
    conn = np.load(stored[0]["connectivity_filepath"])
    assert conn.dtype == np.int32 and conn.ndim == 2 and conn.shape[1] == 2 and len(conn) > 0
    kw = dict(add_normals=False, add_raw_coordinates=True, device=str(device), resegment_mesh=True)
    calls = []
    from unscene3d_amd import felzenszwalb_cpp
    real = felzenszwalb_cpp.segment_mesh
    monkeypatch.setattr(felzenszwalb_cpp, "segment_mesh", lambda *a, **k: calls.append(a[4]) or real(*a, **k))
    a = F.FreeMaskSceneReader(stored, **kw)[0]              # the file: nothing is segmented
    assert calls == []
    b = F.FreeMaskSceneReader(plain, **kw)[0]               # the per-item route
    assert calls == [20]
    F.FreeMaskSceneReader(stored, segment_min_vert_num=50, **kw)[0]         # written with another minimum: not used
    assert calls == [20, 50]
    assert np.array_equal(a[8], conn) and np.array_equal(a[8], b[8]) and np.array_equal(a[2], b[2])
    assert a[8].dtype == b[8].dtype == np.int32


# ---------------------------------------------------------------------------------------------------------- memory
def test_peak_memory_above_the_inputs(device):
    """N = 50 000, K = 40, S = 2 000: above its inputs (the table, the CSR, the segment indices, the adjacency)
    `separate_columns` holds at most the bit rows + the labels i32[K, S] + the [N, R] result."""
    from unscene3d_amd import ops
    from unscene3d_amd.pseudo_masks import freemask as fm
    from unscene3d_amd.trainer.separate import separate_columns, separate_instances

    N, K, S = 50_000, 40, 2_000
    rng = np.random.default_rng(12)
    idx = np.concatenate([np.arange(S), rng.integers(0, S, N - S)])[rng.permutation(N)]
    pairs = rng.integers(0, S, (S // 2, 2))
    conn = np.concatenate([pairs, pairs[:, ::-1]])
    masks = np.zeros((N, K), bool)
    for j in range(K):
        masks[np.isin(idx, rng.choice(S, 3, replace=False)), j] = True
    t_idx = torch.from_numpy(idx).to(device)
    t_masks = torch.from_numpy(masks).to(device)
    csr = ops.segment_csr(t_idx, S)
    idx32 = t_idx.to(torch.int32)
    adj_off, adj = fm.segment_adjacency(torch.from_numpy(conn), torch.arange(S, device=device), mutual=True)
    separate_columns(t_masks[:64].contiguous(), ops.segment_csr(t_idx[:64].contiguous(), S), idx32[:64].contiguous(),
                     adj_off, adj)                           # load the kernels outside the measurement
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, src = separate_columns(t_masks, csr, idx32, adj_off, adj)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    Rn = out.shape[1]
    bits_bytes, label_bytes, result_bytes = K * ((S + 63) // 64) * 8, K * S * 4, N * Rn
    bound = bits_bytes + label_bytes + result_bytes
    # What lives while the result does, by name: the labels, the result, and the parts' vectors src i64[R], src i32[R],
    # root i32[R] (the bit rows, the part counts and the nonzero table are freed before).  The allocator hands out
    # multiples of 512 bytes.  Every instance is three whole segments, so R <= 3 K whatever the seed, and the parts'
    # vectors with all roundings (16 R + 4 * 512 <= 3 968 bytes) fit into the bit rows' 10 240 bytes, which are free by
    # then: the named sum is below the bound by construction, not by the luck of one seed.
    blk = lambda n: -(-max(n, 1) // 512) * 512
    named = blk(label_bytes) + blk(result_bytes) + blk(8 * Rn) + 2 * blk(4 * Rn)
    print(f"separate_columns N={N} K={K} S={S} R={Rn}: additional peak {extra} bytes, named buffers {named}, "
          f"bound {bound} (one [N, K] table: {N * K} bytes)")
    want, want_src, _, _ = R.separate_ref(masks, idx, conn)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), want_src)
    assert K <= Rn <= 3 * K
    assert 16 * Rn + 4 * 512 <= bits_bytes and named <= bound
    assert extra <= named                                   # nothing beside the named buffers
    assert extra <= bound                                   # the stated bound
    # the whole call, ids and pairs included: the N-sized index vectors come on top, nothing of size N x K
    del out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, _ = separate_instances(t_masks, t_idx, conn)
    torch.cuda.synchronize()
    whole = torch.cuda.max_memory_allocated() - base
    print(f"separate_instances: additional peak {whole} bytes = bound + {whole - bound}")
    assert np.array_equal(out.cpu().numpy(), want)
    # beside the bound: idx i64[N], the CSR's order i64[N] and idx i32[N] (20 N bytes), the S- and P-sized vectors
    # (ids, offsets, adjacency, pairs: under 128 KiB here), and under 1 MiB of the caching allocator, which hands out a
    # block that torch.unique's buffers left behind whole when less than 1 MiB of it would remain.  Never N x K.
    assert whole <= bound + 20 * N + 2**17 + 2**20
