"""GPU: the validation metrics' device half — ops.mask_gt_overlap (csrc/evaluate.hip) against a numpy statement of the
histogram, bit for bit; InstanceAPEvaluator on the device against the reference evaluators' golden values
(tests/golden/instance_ap.npz); and InstanceSegmentation.validation_step / validation_epoch_end against the host path
fed with the same predictions copied to the host."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_ap.npz")


def overlap_counts(masks, slot, nslots):
    """numpy statement of ops.mask_gt_overlap: int64 [K+1, nslots]."""
    k = masks.shape[1]
    out = np.zeros((k + 1, nslots), np.int64)
    for j in range(k):
        out[j] = np.bincount(slot[masks[:, j] != 0], minlength=nslots)
    out[k] = np.bincount(slot, minlength=nslots)
    return out


def _case(rng, n, k, nslots, order, ld=None, density=0.1, void_only=False):
    ld = ld or k
    full = rng.random((n, ld)) < density
    if k >= 2 and n:
        full[:, 0] = True                       # an all-true column
        full[:, 1] = False                      # an all-false column
    if void_only:
        slot = np.full(n, nslots - 1, np.int32)
    else:
        slot = rng.integers(0, nslots, n).astype(np.int32)
        if order == "sorted":
            slot = np.sort(slot)
    return full, slot


CASES = [  # n, k, ld, nslots, order
    (0, 7, None, 61, "random"),
    (1, 1, None, 1, "random"),
    (63, 7, 9, 2, "random"),                    # ld > k
    (63, 100, 128, 1001, "sorted"),
    (150_000, 100, None, 31, "sorted"),
    (150_000, 100, None, 31, "random"),
    (150_000, 7, None, 1001, "random"),
    (150_000, 1, None, 65536, "random"),
    (20_000, 257, 300, 61, "random"),
    (20_000, 100, None, 65536, "sorted"),
    (4_000, 4096, None, 2, "random"),
    (4_000, 4096, 4100, 1001, "sorted"),
]


@pytest.mark.parametrize("n,k,ld,nslots,order", CASES)
def test_mask_gt_overlap_equals_numpy(device, n, k, ld, nslots, order):
    from unscene3d_amd import ops

    rng = np.random.default_rng(n * 7 + k * 13 + nslots)
    full, slot = _case(rng, n, k, nslots, order, ld)
    masks_dev = torch.from_numpy(full).to(device)[:, :k]                   # stride(0) = ld >= k
    assert n == 0 or masks_dev.stride(0) == full.shape[1]
    got = ops.mask_gt_overlap(masks_dev, torch.from_numpy(slot).to(device), nslots)
    want = overlap_counts(full[:, :k], slot, nslots)
    assert got.dtype == torch.int32 and tuple(got.shape) == (k + 1, nslots)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


def test_mask_gt_overlap_all_void_u8_and_repeatable(device):
    from unscene3d_amd import ops

    rng = np.random.default_rng(5)
    full, slot = _case(rng, 150_000, 100, 31, "random", void_only=True)
    m = torch.from_numpy(full.astype(np.uint8) * 3).to(device)                # nonzero bytes other than 1
    s = torch.from_numpy(slot).to(device)
    a = ops.mask_gt_overlap(m, s, 31)
    assert np.array_equal(a.cpu().numpy(), overlap_counts(full, slot, 31))
    full, slot = _case(rng, 150_000, 257, 1001, "random")
    m, s = torch.from_numpy(full).to(device), torch.from_numpy(slot).to(device)
    a, b = ops.mask_gt_overlap(m, s, 1001), ops.mask_gt_overlap(m, s, 1001)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), overlap_counts(full, slot, 1001))


def test_mask_gt_overlap_rejects_bad_arguments(device):
    from unscene3d_amd import _lib, ops

    m = torch.zeros((10, 4), dtype=torch.bool, device=device)
    s = torch.zeros(10, dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="nslots"):
        ops.mask_gt_overlap(m, s, 65537)
    with pytest.raises(RuntimeError, match="k out of range"):
        ops.mask_gt_overlap(torch.zeros((10, 4097), dtype=torch.bool, device=device), s, 2)
    assert _lib.lib.usc_mask_gt_overlap(None, 10, 4, 3, None, 2, None, None) == -1
    assert "ld < k" in _lib.last_error()


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("run", ["multi", "freemask"])
def test_device_evaluator_reproduces_reference(device, gold, run):
    from unscene3d_amd.evaluation import ClassSet, InstanceAPEvaluator, validation_results

    p = f"{run}__"
    names = dict(zip(gold[p + "label_ids"].tolist(), gold[p + "label_names"].tolist()))
    cs = ClassSet(gold[p + "class_names"].tolist(), gold[p + "class_ids"].tolist(), label_names=names)
    ev = InstanceAPEvaluator(cs)
    bp, bg = {}, {}
    for i, name in enumerate(gold[p + "scenes"].tolist()):
        q = f"{p}{i}__"
        n, k = int(gold[q + "n"]), int(gold[q + "k"])
        masks = np.unpackbits(gold[q + "masks_packed"], axis=0, count=n).astype(bool)[:, :k]
        inst = {"pred_masks": torch.from_numpy(masks).to(device), "pred_scores": gold[q + "scores"],
                "pred_classes": torch.from_numpy(gold[q + "classes"])}
        ev.add_scene(name, inst, gt_ids=gold[q + "gt_ids"].astype(np.int64))
        bp[name] = [(int(r[0]), r[1:7], np.float32(r[7])) for r in gold[q + "pred_boxes"]]
        bg[name] = [(int(r[0]), r[1:7]) for r in gold[q + "gt_boxes"]]
    r = ev.compute()
    assert np.array_equal(r["ap"], gold[p + "ap"], equal_nan=True)
    assert np.array_equal(r["ar"], gold[p + "ar"], equal_nan=True)
    assert [",".join(row) for row in ev.result_rows()] == gold[p + "csv"].tolist()
    d = validation_results(ev, bp, bg)
    assert d == dict(zip(gold[p + "val_keys"].tolist(), gold[p + "val_values"].tolist()))


def test_validation_hooks_match_host_path(device, tmp_path):
    """validation_step / validation_epoch_end on a small synthetic model and two scenes (GT from a gt_dir of .txt
    files) == the host path (numpy count tables, same predictions and boxes copied to the host)."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.evaluation import (FREEMASK, InstanceAPEvaluator, SceneGT, gt_boxes, pred_box_list,
                                          validation_results)
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    cfg = apply_overrides(default_config(), ["general.num_targets=3", "general.filter_out_instances=true",
                                             "general.topk_per_image=30", "general.scores_threshold=0.0"])
    ds = SyntheticFreeMaskDataset(n_scenes=2, target_voxels=8000, seed=6100)
    batch = [ds[i] for i in range(2)]
    for xyz, _, table, name, *_ in batch:               # GT: the first synthetic mask column of each point
        cols = table[:, 1:-1] != 0
        ids = np.where(cols.any(1), 1000 + cols.argmax(1) + 1, 0)
        (tmp_path / f"{name}.txt").write_text("\n".join(str(int(v)) for v in ids) + "\n")
    torch.manual_seed(21)
    module = InstanceSegmentation(cfg).to(device).eval()
    val_collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="validation", device=str(device))
    data, target, names = val_collate(batch)
    module.begin_validation(gt_dir=str(tmp_path))
    res = module.validation_step((data, target, names))
    assert res is not None and set(res) == {"losses", "instances", "output"}
    got = module.validation_epoch_end()

    host = InstanceAPEvaluator(FREEMASK)
    bp, bg = {}, {}
    for b, (name, inst) in enumerate(zip(names, res["instances"])):
        ids = np.loadtxt(tmp_path / f"{name}.txt", dtype=np.int64)
        sg = SceneGT(ids, FREEMASK)
        masks = inst["pred_masks"].cpu().numpy()
        counts = overlap_counts(masks, sg.slot, sg.nslots) if masks.shape[1] else None
        host.add_scene_counts(name, counts, inst["pred_scores"], inst["pred_classes"], gt_ids=ids)
        bp[name] = pred_box_list(inst["pred_boxes"])
        bg[name] = gt_boxes(data.target_full[b], data.full_res_coords[b])
    want = validation_results(host, bp, bg)
    assert "val_mean_ap_50" in got and "val_foreground_val_ap" in got and "val_mean_box_ap_25" in got
    assert got == want
    assert module.validation_epoch_end() == {}          # the pass's predictions were cleared
