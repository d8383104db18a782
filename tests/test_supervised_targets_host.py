"""CPU: the numpy restatement of the supervised collate targets (tests/instance_targets_ref.py) equals every case the
reference itself produced (tests/golden/instance_targets.npz, written by tests/golden/make_golden_supervised.py), the
reader's remap table equals the reference's sequential `_remap_from_zero`, and the new public names exist and refuse
what is not built.  Integers and booleans only: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import instance_targets_ref as R  # noqa: E402
from supervised_cases import GOLD, MODES, assert_targets_equal, stored_case, stored_targets, voxel_batch  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_the_cases_the_issue_names(gold):
    names = set(gold["case_names"].tolist())
    assert {"basic", "two_labels", "interleaved", "all_filtered", "offset_clamp", "wide_ids", "ignore_255", "two_scenes",
            "second_empty"} <= names
    assert os.path.getsize(GOLD) < 512 * 1024
    ids = gold["case/wide_ids/table0"][:, 1]
    assert ids.min() < -(2 ** 31) and ids.max() >= 2 ** 31
    assert int(gold["case/all_filtered/target/count"]) == 0 and int(gold["case/second_empty/target/count"]) == 0
    t = gold["case/two_labels/table0"]                      # instance 4: first row filtered; instance 9: first row kept
    assert len(np.unique(t[t[:, 1] == 4, 0])) == 2 and len(np.unique(t[t[:, 1] == 9, 0])) == 2
    assert gold["case/two_labels/target/0/labels"].tolist() == [6]
    assert 0 in gold["case/offset_clamp/target/0/labels"]
    assert 253 not in gold["case/ignore_255/target/0/labels"]


def test_numpy_restatement_equals_every_golden_case(gold):
    for name in gold["case_names"].tolist():
        tables, n_seg, flt, off, _, want = stored_case(gold, name)
        seg = None if n_seg is None else [np.zeros((s, 2)) for s in n_seg]
        assert_targets_equal(R.get_instance_masks(tables, seg, flt, off), want, name)


@pytest.mark.parametrize("mode", MODES)
def test_numpy_voxelize_equals_golden(gold, mode):
    got = R.voxelize(voxel_batch(gold), float(gold["vox/voxel_size"]), mode, [int(c) for c in gold["vox/filter"]],
                     int(gold["vox/offset"]))
    assert np.array_equal(got["coordinates"], gold[f"vox/{mode}/coordinates"])
    for b in range(2):
        assert np.array_equal(got["inverse_maps"][b], gold[f"vox/{mode}/inverse_map{b}"])
    assert_targets_equal(got["target"], stored_targets(gold, f"vox/{mode}/target"), f"{mode} target")
    assert_targets_equal(got["target_full"], stored_targets(gold, f"vox/{mode}/target_full"), f"{mode} target_full")
    assert len(got["target"]) == 2 and len(got["target_full"]) == (0 if mode == "train" else 2)


def test_remap_table_equals_the_sequential_remap(gold):
    from unscene3d_amd.datasets.semseg import remap_from_zero, remap_from_zero_table

    for name in gold["remap_names"].tolist():
        keys, v, want = gold[f"remap/{name}/keys"], gold[f"remap/{name}/in"], gold[f"remap/{name}/out"]
        lut = remap_from_zero_table(keys, 255)
        assert np.array_equal(remap_from_zero(v, lut, 255), want), name
        assert np.array_equal(R.remap_table(keys, 255, size=300)[v], want), name
    assert remap_from_zero(np.array([-3, 10 ** 6]), remap_from_zero_table([1, 2], 255), 255).tolist() == [255, 255]


def test_public_names_and_refusals():
    from unscene3d_amd.datasets import utils as U
    from unscene3d_amd.datasets.semseg import SupervisedSceneReader, select_labels

    for name in ("VoxelizeCollate", "voxelize", "get_instance_masks", "FreeMaskVoxelizeCollate"):
        assert hasattr(U, name)
    c = U.VoxelizeCollate(mode="train", filter_out_classes=[0, 1], label_offset=2, device="cuda", spatial_sort=True)
    assert (c.mode, c.label_offset, c.spatial_sort, c.ignore_class_threshold) == ("train", 2, True, 100)
    for kw in ({"small_crops": True}, {"very_small_crops": True}, {"batch_instance": True}):
        with pytest.raises(NotImplementedError):
            U.VoxelizeCollate(**kw)
    with pytest.raises(AssertionError):
        U.VoxelizeCollate(task="panoptic")
    with pytest.raises(NotImplementedError, match="semantic_segmentation"):
        U.get_instance_masks([], "semantic_segmentation")
    assert U.get_instance_masks([], "instance_segmentation") == []

    db = {1: {"validation": True}, 2: {"validation": True}, 7: {"validation": False}}
    entries = [{"filepath": "a/0000.npy", "raw_filepath": "raw/scene0000_00/x.ply"}]
    r = SupervisedSceneReader(entries, db, num_labels=2, mode="validation")
    assert list(r.label_info) == [1, 2] and len(r) == 1
    assert list(SupervisedSceneReader(entries, db, num_labels=3, mode="validation").label_info) == [1, 2, 7]
    with pytest.raises(ValueError):
        select_labels(db, 5)
    for kw in ({"instance_oversampling": 1}, {"add_unlabeled_pc": True}, {"cropping": True}, {"point_per_cut": 100},
               {"resample_points": 0.1}, {"noise_rate": 0.1}, {"flip_in_center": True}):
        with pytest.raises(NotImplementedError):
            SupervisedSceneReader(entries, db, num_labels=3, **kw)


def test_reader_validation_item_and_data_percent(tmp_path):
    import random

    from unscene3d_amd.datasets.semseg import SupervisedSceneReader

    rng = np.random.default_rng(3)
    pts = np.zeros((50, 12), np.float32)
    pts[:, :3], pts[:, 3:6], pts[:, 6:9] = rng.normal(size=(50, 3)), rng.uniform(0, 255, (50, 3)), rng.normal(size=(50, 3))
    pts[:, 9], pts[:, 10], pts[:, 11] = rng.integers(0, 9, 50), rng.choice([1, 2, 7, 40], 50), rng.integers(-1, 4, 50)
    entries = []
    for i in range(4):
        d = tmp_path / f"scene{i:04d}_00"
        d.mkdir()
        np.save(d / "points.npy", pts)
        entries.append({"filepath": str(d / "points.npy"), "raw_filepath": f"raw/scene{i:04d}_00/mesh.ply"})
    db = {1: {"validation": True}, 2: {"validation": True}, 7: {"validation": False}}
    r = SupervisedSceneReader(entries, db, num_labels=3, mode="validation", add_instance=True)
    item = r[1]
    assert len(item) == 9 and item[3] == "scene0001_00" and item[8] == [] and item[7] == 1
    want = np.stack([np.select([pts[:, 10] == 1, pts[:, 10] == 2, pts[:, 10] == 7], [0, 1, 2], 255), pts[:, 11], pts[:, 9]], 1)
    assert item[2].dtype == np.int32 and np.array_equal(item[2], want.astype(np.int32))
    assert item[1].shape == (50, 6) and item[1].dtype == np.float32
    assert SupervisedSceneReader(entries, db, num_labels=3, mode="validation")[0][2].shape == (50, 2)
    random.seed(5)
    expect = random.sample(entries, 2)
    random.seed(5)
    assert SupervisedSceneReader(entries, db, num_labels=3, mode="validation", data_percent=0.5).data == expect


def test_synthetic_label_table():
    from unscene3d_amd.synthetic import make_label_table, make_scene

    sc = make_scene(1000, target_voxels=20000, tol=0.1)          # large enough to hold furniture
    t = make_label_table(sc, 1000)
    assert t.dtype == np.int32 and t.shape == (sc["xyz"].shape[0], 3)
    ids = np.unique(t[:, 1])
    assert ids[0] == -1 and np.all(np.diff(ids[1:]) >= 13) and not np.array_equal(t[:, 1], np.sort(t[:, 1]))
    lab, masks, _ = R.instance_targets(t, None, [0, 1], 2)
    kept = t[np.isin(t[:, 1], ids[1:]) & ~np.isin(t[:, 0], [0, 1])]
    assert masks.shape[0] == len(np.unique(kept[:, 1])) and 253 in lab and lab.max() <= 253
    assert set(lab.tolist()) - {253} <= set(range(18))
    assert np.array_equal(t, make_label_table(sc, 1000))
    assert len(np.unique(make_label_table(sc, 1000, parts=3)[:, 1])) > len(ids)
