"""GPU: the supervised collate's instance targets (csrc/targets.hip through ops.instance_targets,
datasets.utils.get_instance_masks / voxelize / VoxelizeCollate, datasets.semseg.SupervisedSceneReader) against the numpy
restatement tests/instance_targets_ref.py and against the reference's own stored outputs
(tests/golden/instance_targets.npz).  Everything compared is integer or boolean: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import instance_targets_ref as R  # noqa: E402
from supervised_cases import GOLD, MODES, assert_targets_equal, stored_case, stored_targets, voxel_batch  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# ids of every kind the contract names: negative, gapped, around 2^31 and 2^32, up to 2^62
WIDE = [-(2 ** 40), -(2 ** 31) - 1, -9, -2, 0, 1, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 3, 2 ** 62]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


class GuardedAlloc:
    """alloc(shape, dtype, zero) of ops.instance_targets: every array sits between guard bytes.  Byte arrays start at an
    address that is no multiple of 4 (`shift`), so the mask rows meet every alignment."""

    def __init__(self, device, shift=3):
        self.device, self.shift, self.bufs = device, shift, []

    def __call__(self, shape, dtype, zero):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        lead = 64 + (self.shift if dtype == torch.uint8 else 0)
        raw = torch.full((lead + nbytes + 64,), GUARD, dtype=torch.uint8, device=self.device)
        body = raw[lead:lead + nbytes]
        if zero:
            body.zero_()
        self.bufs.append((raw, lead, nbytes))
        return body.view(dtype).view(shape)

    def check(self):
        for raw, lead, nbytes in self.bufs:
            assert bool((raw[:lead] == GUARD).all()) and bool((raw[lead + nbytes:] == GUARD).all()), "guard bytes written"


def make_table(rng, n, n_ids, n_seg, only_unlabeled=False):
    """[N,3] table with exactly min(n_ids, n) distinct instance ids (only_unlabeled: the single id -1)."""
    n_ids = min(n_ids, n)
    if only_unlabeled:
        ids = np.array([-1], np.int64)
    else:
        pool = np.array(WIDE + [-1], np.int64)
        extra = 11 + 7 * np.arange(max(0, n_ids - len(pool)), dtype=np.int64)
        ids = np.concatenate([rng.permutation(pool), extra])[:n_ids]
    inst = np.concatenate([ids, rng.choice(ids, n - len(ids))])     # every id at least once
    inst = inst[rng.permutation(n)]
    label_of = dict(zip(ids.tolist(), rng.integers(0, 6, len(ids)).tolist()))
    lab = np.array([label_of[int(i)] for i in inst], np.int64)
    seg = rng.integers(0, max(n_seg, 1), n)
    return np.stack([lab, inst, seg], 1)


def run_device(table, n_seg, flt, off, device, shift=3):
    from unscene3d_amd import ops

    alloc = GuardedAlloc(device, shift)
    t = torch.from_numpy(np.ascontiguousarray(table)).to(device)
    out = ops.instance_targets(t, n_seg, flt, off, alloc=alloc)
    torch.cuda.synchronize()
    alloc.check()
    return out, alloc


def assert_equals_oracle(table, n_seg, flt, off, device, shift=3):
    (lab, masks, seg), alloc = run_device(table, n_seg, flt, off, device, shift)
    wl, wm, ws = R.instance_targets(table, n_seg, flt, off)
    assert lab.dtype == torch.int64 and masks.dtype == torch.bool
    assert np.array_equal(lab.cpu().numpy(), wl)
    assert tuple(masks.shape) == wm.shape and np.array_equal(masks.cpu().numpy(), wm)
    assert np.array_equal(masks.view(torch.uint8).cpu().numpy(), wm.astype(np.uint8)), "mask bytes are not 0 / 1"
    if n_seg is None:
        assert seg is None
    else:
        assert tuple(seg.shape) == ws.shape and np.array_equal(seg.cpu().numpy(), ws)
    first = [raw.clone() for raw, _, _ in alloc.bufs]
    _, again = run_device(table, n_seg, flt, off, device, shift)          # two calls: identical bytes, work arrays too
    for a, (b, _, _) in zip(first, again.bufs):
        assert torch.equal(a, b)
    return wl


@pytest.mark.parametrize("n_ids", ["only-1", 1, 2, 33, 129, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_kernel_equals_oracle(device, n, n_ids):
    rng = np.random.default_rng(1000 * n + (0 if n_ids == "only-1" else n_ids))
    only = n_ids == "only-1"
    for n_seg in (None, 0, 1, 40, 700):
        table = make_table(rng, n, 1 if only else n_ids, n_seg or 1, only_unlabeled=only)
        if n_seg == 0:
            table = table[:0]                                   # S = 0 goes with an empty table
        kept = assert_equals_oracle(table, n_seg, [0, 1], 2, device, shift=(n + (n_seg or 0)) % 4)
        if only or n_seg == 0:
            assert kept.shape[0] == 0


def test_more_ids_than_one_window_and_no_filter(device):
    rng = np.random.default_rng(5)
    table = make_table(rng, 4097, 2100, 700)                   # > 2048 ids: two id windows in the index kernel
    assert len(np.unique(table[:, 1])) == 2100
    assert assert_equals_oracle(table, 700, [], 0, device).shape[0] == 2099
    assert_equals_oracle(table[:, :2].copy(), None, [3], 1, device)


def test_first_row_decides_interleaved_filtered_and_clamped(device):
    n = 131
    t = np.zeros((n, 3), np.int64)
    t[:, 1] = np.where(np.arange(n) % 2 == 0, 2 ** 33, -5)     # two instances interleaved row by row
    t[:, 0] = np.where(np.arange(n) % 2 == 0, 4, 9)
    t[:, 2] = np.arange(n) % 7
    assert assert_equals_oracle(t, 7, [], 0, device).tolist() == [9, 4]
    two = t.copy()
    two[0, 0] = 1                                              # id 2^33: first row says 1 (filtered), the others 4
    two[1, 0], two[3:, 0] = 9, np.where(np.arange(3, n) % 2 == 1, 0, two[3:, 0])   # id -5: first row 9, the others 0
    assert assert_equals_oracle(two, 7, [0, 1], 0, device).tolist() == [9]
    (lab, masks, seg), _ = run_device(t, 7, [4, 9], 0, device)  # every class filtered
    assert lab.shape[0] == 0 and tuple(masks.shape) == (0, n) and tuple(seg.shape) == (0, 7)
    assert assert_equals_oracle(t, 7, [], 7, device).tolist() == [2, 0]            # offset larger than a label -> 0


def test_empty_table_and_bad_arguments(device):
    from unscene3d_amd import _lib, ops

    (lab, masks, seg), _ = run_device(np.zeros((0, 3), np.int64), 0, [0], 2, device)
    assert lab.shape[0] == 0 and tuple(masks.shape) == (0, 0) and tuple(seg.shape) == (0, 0)
    with pytest.raises(RuntimeError, match="labels must be"):
        ops.instance_targets(torch.zeros((4, 2), dtype=torch.int64, device=device), 3)
    with pytest.raises(RuntimeError, match="int64"):
        ops.instance_targets(torch.zeros((4, 3), dtype=torch.int32, device=device))
    assert _lib.lib.usc_instance_index(None, 4, 1, None, 0, None, None, None, None) == -1
    assert "ld < 2" in _lib.last_error()
    assert _lib.lib.usc_instance_masks(None, 4, None, 2, 3, None, None, 1, 0, None, None) == -1
    assert "t out of range" in _lib.last_error()


def test_get_instance_masks_equals_the_reference(device, gold):
    from unscene3d_amd.datasets.utils import get_instance_masks

    for name in gold["case_names"].tolist():
        tables, n_seg, flt, off, threshold, want = stored_case(gold, name)
        dev_tables = [torch.from_numpy(t).to(device) for t in tables]
        seg = None if n_seg is None else [torch.zeros((s, 2), dtype=torch.int64, device=device) for s in n_seg]
        got = get_instance_masks(dev_tables, "instance_segmentation", list_segments=seg,
                                 ignore_class_threshold=threshold, filter_out_classes=flt, label_offset=off)
        assert_targets_equal(got, want, name)
        for t in got:
            assert all(v.is_cuda for v in t.values())


def _collate(gold, mode, device, spatial_sort=False):
    from unscene3d_amd.datasets.utils import VoxelizeCollate

    c = VoxelizeCollate(ignore_label=255, voxel_size=float(gold["vox/voxel_size"]), mode=mode,
                        filter_out_classes=[int(v) for v in gold["vox/filter"]], label_offset=int(gold["vox/offset"]),
                        device=str(device), spatial_sort=spatial_sort)
    return c(voxel_batch(gold))


@pytest.mark.parametrize("mode", MODES)
def test_collate_equals_the_reference_voxelize(device, gold, mode):
    data, target, names = _collate(gold, mode, device)
    assert names == ["scene0", "scene1"]
    assert data.coordinates.dtype == torch.int32
    assert np.array_equal(data.coordinates.cpu().numpy(), gold[f"vox/{mode}/coordinates"])
    um = R.voxelize(voxel_batch(gold), float(gold["vox/voxel_size"]), mode)["unique_maps"]
    feats = np.concatenate([gold[f"vox/scene{b}/feats"][um[b]] for b in range(2)])
    assert np.array_equal(data.features.cpu().numpy(), feats)
    for b in range(2):
        assert np.array_equal(data.inverse_maps[b].cpu().numpy(), gold[f"vox/{mode}/inverse_map{b}"])
    want = stored_targets(gold, f"vox/{mode}/target")
    assert_targets_equal(target, want, f"{mode} target")
    for t, w in zip(target, want):
        assert int(t["num_segments"]) == int(w["point2segment"].max()) + 1 and not t["num_segments"].is_cuda
    if mode == "train":
        assert data.target_full is None
    else:
        assert_targets_equal(data.target_full, stored_targets(gold, f"vox/{mode}/target_full"), f"{mode} target_full")


@pytest.mark.parametrize("mode", ["train", "validation"])
def test_spatial_sort_permutes_the_targets(device, gold, mode):
    plain, tp, _ = _collate(gold, mode, device)
    srt, ts, _ = _collate(gold, mode, device, spatial_sort=True)
    a, b = plain.coordinates.cpu().numpy(), srt.coordinates.cpu().numpy()
    perm = np.empty(len(a), np.int64)                          # b = a[perm]
    perm[np.lexsort(b.T[::-1])] = np.lexsort(a.T[::-1])
    assert np.array_equal(a[perm], b) and not np.array_equal(a, b)
    assert np.array_equal(plain.features.cpu().numpy()[perm], srt.features.cpu().numpy())
    start = 0
    for s in range(2):
        n = int((a[:, 0] == s).sum())
        p = perm[start:start + n] - start
        assert np.array_equal(np.sort(p), np.arange(n))
        for k in ("labels", "segment_mask"):
            assert torch.equal(tp[s][k], ts[s][k])
        assert np.array_equal(tp[s]["masks"].cpu().numpy()[:, p], ts[s]["masks"].cpu().numpy())
        assert np.array_equal(tp[s]["point2segment"].cpu().numpy()[p], ts[s]["point2segment"].cpu().numpy())
        assert np.array_equal(p[srt.inverse_maps[s].cpu().numpy()], plain.inverse_maps[s].cpu().numpy())
        start += n
    if mode == "validation":
        assert_targets_equal(srt.target_full, stored_targets(gold, "vox/validation/target_full"), "sorted target_full")


def test_one_dimensional_tables_and_probing(device, gold):
    from unscene3d_amd.datasets.utils import voxelize

    batch = [s[:2] + (s[2][:, 0].copy(),) + s[3:] for s in voxel_batch(gold)]
    batch[0][2][:5] = 255
    data, target, _ = voxelize(batch, 255, 0.05, False, "validation", "instance_segmentation", 100, [], 0, None,
                               device=str(device))
    ref = R.voxelize(voxel_batch(gold), 0.05, "test")
    for b in range(2):
        lab = batch[b][2][ref["unique_maps"][b]]
        ids = np.unique(lab)
        ids = ids[:-1] if 255 in ids else ids
        assert np.array_equal(target[b]["labels"].cpu().numpy(), ids)
        assert np.array_equal(target[b]["masks"].cpu().numpy(), lab[None, :] == ids[:, None])
    data, labels = voxelize(voxel_batch(gold), 255, 0.05, True, "train", "instance_segmentation", 100, [], 0, None,
                            device=str(device))
    assert data.full_res_coords is None and len(data.inverse_maps) == 2
    assert tuple(labels.shape) == (data.coordinates.shape[0], 3)


# ------------------------------------------------------------------------------------------------------- end to end
LABEL_DB = {k: {"validation": True} for k in range(20)}


def _write_scene(tmp_path, seed, parts, keep_targets=None):
    """A synthetic labelled scene as `{scene}.npy` [N,12] -> the reader's database entry."""
    from unscene3d_amd.synthetic import _COLOR_MEAN, _COLOR_STD, make_label_table, make_scene

    sc = make_scene(seed, 8000)
    table = make_label_table(sc, seed, parts=parts).astype(np.int64)
    if keep_targets is not None:     # exactly `keep_targets` kept instances, the largest after voxelisation: the rest -> -1
        voxels = np.floor(sc["xyz"].astype(np.float32).astype(np.float64) / 0.02).astype(np.int64)
        ids, counts = np.unique(table[R.first_unique(voxels)[0], 1], return_counts=True)
        first = {int(i): int(table[table[:, 1] == i][0, 0]) for i in ids}
        kept = [int(i) for i in ids[np.argsort(-counts, kind="stable")] if i != -1 and first[int(i)] not in (0, 1)]
        assert len(kept) >= keep_targets
        table[np.isin(table[:, 1], kept[keep_targets:]), 1] = -1
    pts = np.zeros((table.shape[0], 12), np.float32)
    pts[:, :3] = sc["xyz"]
    pts[:, 3:6] = np.clip(sc["colors"] * _COLOR_STD + _COLOR_MEAN, 0, 255)
    pts[:, 9], pts[:, 10], pts[:, 11] = table[:, 2], table[:, 0], table[:, 1]
    d = tmp_path / f"scene{seed:04d}_00"
    d.mkdir()
    np.save(d / "points.npy", pts)
    return {"filepath": str(d / "points.npy"), "raw_filepath": f"raw/scene{seed:04d}_00/mesh.ply"}


def _oracle_batch(item, data, device):
    """The same batch with targets built by the numpy oracle and moved to the device."""
    ref = R.voxelize([item], 0.02, "train", [0, 1], 2)
    assert np.array_equal(ref["coordinates"], data.coordinates.cpu().numpy())
    target = []
    for t in ref["target"]:
        e = {k: torch.from_numpy(v).to(device) for k, v in t.items()}
        e["num_segments"] = torch.tensor(int(t["point2segment"].max()) + 1)
        target.append(e)
    return target


@pytest.mark.parametrize("n_targets,max_targets", [(None, 32), (40, 64)])
def test_reader_collate_training_step(device, tmp_path, n_targets, max_targets):
    """scene file -> SupervisedSceneReader -> VoxelizeCollate -> training_step with 19 classes: the losses are bit-identical
    to the same step fed the oracle's targets (<= 32 targets on the default criterion path, 40 with
    device_max_targets=64); then validation_step(label_offset=2) on the validation collate's batch."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.semseg import SupervisedSceneReader
    from unscene3d_amd.datasets.utils import VoxelizeCollate
    from unscene3d_amd.evaluation import ClassSet
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    entry = _write_scene(tmp_path, 71, 1 if n_targets is None else 3, n_targets)
    reader = SupervisedSceneReader([entry], LABEL_DB, num_labels=20, mode="validation", add_normals=False,
                                   add_raw_coordinates=True, add_instance=True, device=str(device))
    item = reader[0]
    kw = dict(ignore_label=255, voxel_size=0.02, filter_out_classes=[0, 1], label_offset=2, device=str(device))
    overrides = ["general.num_targets=19"] + ([] if max_targets == 32 else [f"loss.device_max_targets={max_targets}"])
    cfg = apply_overrides(default_config(), overrides)
    torch.manual_seed(3)
    module = InstanceSegmentation(cfg).to(device).train()
    assert module.criterion.device_max_targets == max_targets
    state = {k: v.clone() for k, v in module.state_dict().items()}
    res = []
    for source in ("device", "oracle"):
        data, target, _ = VoxelizeCollate(mode="train", **kw)([item])
        T = target[0]["labels"].shape[0]
        assert (T <= 32) if n_targets is None else (T == 40)
        assert 253 in target[0]["labels"].tolist() or n_targets is not None
        if source == "oracle":
            oracle = _oracle_batch(item, data, device)
            assert_targets_equal(target, [{k: v.cpu().numpy() for k, v in t.items() if k != "num_segments"} for t in oracle])
            target = oracle
        module.load_state_dict(state)
        torch.manual_seed(17)
        total, parts = module.training_step((data, target, ["scene"]))
        total.backward()
        module.criterion.check_lsap_status(wait=True)
        torch.cuda.synchronize()
        res.append((float(total.detach()), {k: float(v.detach()) for k, v in parts.items()}))
        module.zero_grad(set_to_none=True)
    assert np.isfinite(res[0][0]) and res[0][0] == res[1][0] and res[0][1] == res[1][1]

    # validation: full-resolution targets, AP inputs
    data, target, names = VoxelizeCollate(mode="validation", **kw)([item])
    full = R.get_instance_masks([item[2]], None, [0, 1], 2)
    assert_targets_equal(data.target_full, full, "target_full")
    assert np.array_equal(data.target_full[0]["point2segment"].cpu().numpy(), item[2][:, 2])
    gt_ids = np.where(item[2][:, 1] >= 0, item[2][:, 0].astype(np.int64) * 1000 + item[2][:, 1] + 1, 0)
    ids = tuple(range(2, 20))
    module.eval()
    module.begin_validation(class_set=ClassSet(tuple(f"class{i}" for i in ids), ids), gt_ids={names[0]: gt_ids})
    out = module.validation_step((data, target, names), label_offset=2)
    inst = out["instances"][0]
    assert inst["pred_masks"].shape[0] == item[0].shape[0]
    assert bool(torch.isfinite(torch.as_tensor(inst["pred_scores"])).all())
    classes = torch.as_tensor(inst["pred_classes"])
    assert bool(((classes >= 2) & (classes < 20)).all())
    assert all(np.isfinite(v) for v in out["losses"].values())
    assert isinstance(module.validation_epoch_end(), dict)


def test_reader_train_mode_keeps_the_label_table(device, tmp_path):
    from unscene3d_amd.datasets.augment import ColorAugmentations, VolumeAugmentations
    from unscene3d_amd.datasets.semseg import SupervisedSceneReader

    entry = _write_scene(tmp_path, 72, 1)
    kw = dict(num_labels=20, add_normals=False, add_raw_coordinates=True, add_instance=True, device=str(device))
    plain = SupervisedSceneReader([entry], LABEL_DB, mode="validation", **kw)[0]
    np.random.seed(1)
    item = SupervisedSceneReader([entry], LABEL_DB, mode="train", volume_augmentations=VolumeAugmentations(),
                                 image_augmentations=ColorAugmentations(), **kw)[0]
    assert len(item) == 9 and item[3] == "scene0072_00"
    assert np.array_equal(item[2], plain[2]) and item[2].dtype == np.int32
    assert item[0].is_cuda and tuple(item[0].shape) == plain[0].shape and tuple(item[1].shape) == plain[1].shape
    assert not np.allclose(item[0].cpu().numpy(), plain[0])
