"""GPU: the device mask tables (csrc/dataset.hip) against the reader's host path, the vertex-normal kernel against a
float64 restatement, the dataset builder against `process_file` restated in numpy, and the two tools end to end."""
import json
import os
import random as pyrandom
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "dataset.npz")


# -------------------------------------------------------------------------------------------------------- mask tables
@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.5, 0.35])
@pytest.mark.parametrize("N,K", D.TABLE_SHAPES)
def test_mask_tables_device_equal_the_host_path(device, N, K, thr):
    """Keep list and table of `mask_tables_device` == `filter_by_extent` + the numpy lines of `__getitem__`, exactly.
    Every shape holds (over its variants) an empty column with entries AT f32(thr), a column too wide in x only, one
    in y only, one exactly at the extent limit, a column whose only hit is the last row; (300, 65) has a second column
    tile of one column, (5000, 50) twenty row blocks."""
    from unscene3d_amd import ops
    from unscene3d_amd.datasets.freemask import mask_tables_device

    kept_any = False
    for xyz, soft, seg, where in D.mask_table_cases(N, K, thr):
        ref_table, ref_keep = D.host_tables(xyz, soft, seg, thr, 0.8, device)
        table, keep = mask_tables_device(xyz, soft, seg, thr, 0.8, device)
        assert keep == ref_keep
        if N >= 8:
            for feat in ("empty", "wide_x", "wide_y"):
                assert where.get(feat, -1) not in keep
            for feat in ("limit", "last_row", "at_thr"):
                assert feat not in where or where[feat] in keep
        if not ref_keep:
            assert table is None
            continue
        kept_any = True
        assert table.is_cuda and table.dtype == torch.int32 and table.shape == ref_table.shape
        assert np.array_equal(table.cpu().numpy(), ref_table)

        hard = soft > np.float32(thr)                           # the statistics themselves, empty columns included
        count, lo, hi = ops.softmask_stats(torch.from_numpy(soft).to(device), torch.from_numpy(xyz).to(device), thr)
        assert np.array_equal(count.cpu().numpy(), hard.sum(0))
        big = np.finfo(np.float32).max
        exp_lo = np.stack([np.where(hard, xyz[:, None, d], big).min(0) for d in (0, 1)], 1)
        exp_hi = np.stack([np.where(hard, xyz[:, None, d], -big).max(0) for d in (0, 1)], 1)
        assert np.array_equal(lo.cpu().numpy(), exp_lo) and np.array_equal(hi.cpu().numpy(), exp_hi)
    assert kept_any


def _golden_reader(tmp_path, device, freemasks=None, **kw):
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader

    z = np.load(GOLD)
    d = tmp_path / "scans" / "scene0001_00"
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "0001_00.npy", z["points"])
    np.save(d / "0001_00_freemasks.npy", z["freemasks"] if freemasks is None else freemasks)
    entry = {"filepath": str(d / "0001_00.npy"), "raw_filepath": "raw/scene0001_00/scene0001_00_vh_clean_2.ply"}
    return FreeMaskSceneReader([entry], add_raw_coordinates=True, device=device, **kw)


def _same_item(a, b):
    for j, (x, y) in enumerate(zip(a, b)):
        if j == 2:
            assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.int32
            assert x.dtype == np.int32 and np.array_equal(x, y.cpu().numpy())
        elif isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        else:
            assert x == y


@pytest.mark.gpu
def test_reader_with_device_tables_returns_the_same_items(device, tmp_path):
    """On the golden scene: item 2 as a device int32 tensor with the default reader's values, every other item the
    same, in validation mode and in train mode (shipped augmentation pipelines) under the same seeds — and numpy's and
    python's generators end in the same state: the table path draws nothing."""
    from unscene3d_amd.datasets.augment import ColorAugmentations, VolumeAugmentations
    from unscene3d_amd.trainer.postprocess import save_for_freemask

    z = np.load(GOLD)
    _same_item(_golden_reader(tmp_path, device)[0], _golden_reader(tmp_path, device, device_tables=True)[0])

    same = np.unpackbits(z["st_masks_same"], axis=1)[:, :6].astype(bool)
    save_for_freemask(str(tmp_path), "scene0001_00", z["points"][:, :3], same)
    items, states = [], []
    for dev_tables in (False, True):
        reader = _golden_reader(tmp_path, device, mode="train", volume_augmentations=VolumeAugmentations(),
                                image_augmentations=ColorAugmentations(), color_drop=0.3, load_self_train_data=True,
                                self_train_data_dir=str(tmp_path), device_tables=dev_tables)
        np.random.seed(7)
        pyrandom.seed(7)
        items.append(reader[0])
        states.append((np.random.get_state(), pyrandom.getstate()))
    _same_item(*items)
    assert items[1][2].shape[0] == z["points"].shape[0] and items[1][2].shape[1] >= 3
    (n0, p0), (n1, p1) = states
    assert p0 == p1 and n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]

    for dev_tables in (False, True):
        with pytest.raises(LookupError, match="no usable pseudo mask"):
            _golden_reader(tmp_path, device, freemasks=np.zeros_like(z["freemasks"]), device_tables=dev_tables)[0]


# ------------------------------------------------------------------------------------------------------------ normals
def _normal_meshes():
    rng = np.random.default_rng(3)
    tet = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float32),        # vertex 4: isolated
           np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32), [4])
    ang = np.linspace(0, 2 * np.pi, 70, endpoint=False)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * np.sin(3 * ang)], 1)
    fan_v = np.vstack([[[0, 0, 0.3]], rim, [[3, 3, 3], [4, 4, 4]]]).astype(np.float32)            # 71, 72: zero-area faces
    fan_f = np.array([[0, 1 + i, 1 + (i + 1) % 70] for i in range(70)] + [[71, 71, 72], [71, 72, 72], [72, 71, 71]],
                     np.int32)
    V = 300
    cloud_v = rng.uniform(-2, 2, (V, 3)).astype(np.float32)
    cloud_f = rng.integers(0, V - 1, (650, 3)).astype(np.int32)                                  # vertex 299: isolated
    cloud_f = cloud_f[(cloud_f[:, 0] != cloud_f[:, 1]) & (cloud_f[:, 1] != cloud_f[:, 2]) & (cloud_f[:, 0] != cloud_f[:, 2])]
    cloud_f[17] = (5, 9, 5)                                                                      # one degenerate face
    return {"tetrahedron": tet, "fan70": (fan_v, fan_f, [71, 72]), "random300": (cloud_v, cloud_f, [299])}


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", ["tetrahedron", "fan70", "random300"])
def test_vertex_normals_against_float64(device, mesh):
    """`ops.mesh_vertex_normals` against the float64 restatement that adds faces in ascending order.  Bound per
    component, derived (dataset_cases.vertex_normals_f64): 8 (deg + 8) 2^-53 sum|terms| / |sum| on the float64 value;
    the kernel stores f32, so the stored number must be the f32 rounding of SOME value within that bound of the
    reference: f32(ref - bound) <= out <= f32(ref + bound).  Isolated vertices and vertices whose faces all have zero
    area give exactly (0,0,1)."""
    from unscene3d_amd import ops

    vertices, faces, flat = _normal_meshes()[mesh]
    got = ops.mesh_vertex_normals(torch.from_numpy(vertices).to(device), torch.from_numpy(faces).to(device)).cpu().numpy()
    ref, bound = D.vertex_normals_f64(vertices, faces)
    assert got.dtype == np.float32 and got.shape == ref.shape
    for v in flat:
        assert got[v].tolist() == [0.0, 0.0, 1.0] and bound[v] == 0
    assert np.isfinite(bound).all() and float(bound.max()) < 1e-9        # the meshes are well conditioned: the check bites
    lo, hi = (ref - bound[:, None]).astype(np.float32), (ref + bound[:, None]).astype(np.float32)
    bad = (got < lo) | (got > hi)
    assert not bad.any(), f"{int(bad.sum())} components outside the bound, worst {np.abs(got - ref).max():.3e}"
    deg = np.bincount(faces.reshape(-1), minlength=vertices.shape[0])
    assert mesh != "fan70" or deg[0] == 70                               # a degree above one wave
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, rtol=0, atol=3 * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------ builder
def _assert_tables(t, scan, cloud, masks, oracle=False):
    points, nbound, free, gt, mean, std = D.scene_tables_numpy(scan, cloud, masks, oracle=oracle)
    got = t["points"]
    assert got.dtype == np.float32 and got.shape == points.shape == (scan["vertices"].shape[0], 12)
    other = [0, 1, 2, 3, 4, 5, 9, 10, 11]
    assert np.array_equal(got[:, other], points[:, other].astype(np.float32))
    lo = (points[:, 6:9] - nbound[:, None]).astype(np.float32)
    hi = (points[:, 6:9] + nbound[:, None]).astype(np.float32)
    assert ((got[:, 6:9] >= lo) & (got[:, 6:9] <= hi)).all()
    assert t["freemasks"].dtype == np.float32 and np.array_equal(t["freemasks"], free)
    assert (t["gt"] is None) == (gt is None) and (gt is None or (t["gt"].dtype == np.int32 and np.array_equal(t["gt"], gt)))
    assert t["color_mean"] == mean and t["color_std"] == std
    return points


@pytest.mark.gpu
@pytest.mark.parametrize("soft", [False, True])
def test_builder_equals_process_file_restated(device, tmp_path, soft):
    """`build_scene_tables` / `build_dataset` on a `synthetic.make_mesh` scan with ground-truth files and pseudo masks
    on a shuffled, jittered cloud: table, freemasks, gt text and database against numpy (brute-force 1-NN)."""
    from unscene3d_amd.datasets import preprocessing as P
    from unscene3d_amd.datasets.freemask import entries_from_database, load_color_mean_std
    from unscene3d_amd.evaluation.instance_ap import load_gt_ids

    name = "scene0012_03"
    scan = D.write_scan(str(tmp_path / "scans"), name, seed=4)
    cloud, masks = D.write_pseudo(str(tmp_path / "pm"), name, scan, seed=4, soft=soft)
    t = P.build_scene_tables(scan["dir"], str(tmp_path / "pm"), device=device)
    points = _assert_tables(t, scan, cloud, masks)
    labels = points[:, 10:12].astype(np.int64)
    assert set(labels[:, 0].tolist()) == {1, 40} and (labels[labels[:, 0] != 1, 1] == -1).all()   # the quirk is in the data
    assert set(labels[:, 1].tolist()) == {-1, 0, 1, 3, 4}            # group 2 is a wall: its instance is gone

    D.write_scan(str(tmp_path / "scans"), "scene0013_00", seed=5)    # no pseudo masks: skipped with a message
    out = tmp_path / "data"
    dbs = P.build_dataset(str(tmp_path / "scans"), {"train": [name, "scene0013_00"]}, str(tmp_path / "pm"), str(out),
                          device=device)
    assert [e["scene"] for e in dbs["train"]] == [12]
    e = entries_from_database(out / "train_database.yaml")[0]
    assert e == dbs["train"][0]
    assert (e["scene"], e["sub_scene"], e["file_len"]) == (12, 3, points.shape[0])
    assert e["filepath"] == str(out / "train" / "0012_03.npy") and e["raw_filepath"].split("/")[-2] == name
    assert np.array_equal(np.load(e["filepath"]), t["points"])
    assert np.array_equal(np.load(out / "train" / "0012_03_freemasks.npy"), t["freemasks"])
    assert np.array_equal(load_gt_ids(out / "instance_gt" / "train" / f"{name}.txt"), t["gt"])
    assert not (out / "train" / "0013_00.npy").exists()
    mean, std = load_color_mean_std(out / "color_mean_std.yaml")
    assert list(mean) == e["color_mean"]
    assert list(std) == [float(v) for v in np.sqrt(np.array(e["color_std"]) - np.array(e["color_mean"]) ** 2)]
    assert sorted(os.listdir(out)) == ["color_mean_std.yaml", "instance_gt", "label_database.yaml", "train",
                                       "train_database.yaml"]


@pytest.mark.gpu
def test_builder_oracle_masks_and_scans_without_ground_truth(device, tmp_path, capsys):
    from unscene3d_amd import felzenszwalb_cpp
    from unscene3d_amd.datasets import preprocessing as P

    scan = D.write_scan(str(tmp_path / "scans"), "scene0001_00", seed=6)
    t = P.build_scene_tables(scan["dir"], None, oracle=True, device=device)
    _assert_tables(t, scan, None, None, oracle=True)
    inst = t["points"][:, 11]
    assert t["freemasks"].shape[1] == 4 and set(np.unique(t["freemasks"]).tolist()) == {0.0, 1.0}
    for i in range(4):                  # one-hot of instance == i for i < number of ids: ids 0, 1, 3, 4 -> column 2 empty
        assert np.array_equal(t["freemasks"][:, i] == 1.0, inst == i)
    assert (t["freemasks"].sum(1) <= 1).all() and not t["freemasks"][:, 2].any()

    assert P.build_scene_tables(scan["dir"], str(tmp_path / "none"), device=device) is None
    assert "Could not load pseudo masks for scene0001_00" in capsys.readouterr().out

    bare = D.write_scan(str(tmp_path / "scans"), "scene0002_00", seed=7, gt=False, segs=False, axis=None)
    cloud, masks = D.write_pseudo(str(tmp_path / "pm"), "scene0002_00", bare, seed=7)
    t = P.build_scene_tables(bare["dir"], str(tmp_path / "pm"), device=device)
    assert t["gt"] is None and (t["points"][:, 10] == 0).all() and (t["points"][:, 11] == -1).all()
    colors = (bare["rgb"].astype(np.float64) / 255.0).astype(np.float32)
    seg, _ = felzenszwalb_cpp.segment_mesh(bare["vertices"], bare["faces"], colors, 0.005, 20, device=device)
    assert np.array_equal(t["points"][:, 9], seg.astype(np.float32))
    d2 = ((bare["vertices"][:, None, :].astype(np.float64) - cloud[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(t["freemasks"], masks[d2.argmin(1)].astype(np.float32))
    out = tmp_path / "data"
    P.build_dataset(str(tmp_path / "scans"), {"validation": ["scene0002_00"]}, str(tmp_path / "pm"), str(out), device=device)
    assert not (out / "instance_gt").exists() and (out / "color_mean_std.yaml").exists()


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.gpu
def test_tools_from_scan_directories_to_a_checkpoint(device, tmp_path):
    """tools/dataset_from_scans.py, then tools/train.py --data-dir for 3 steps with device tables and with
    --host-tables: both return 0, every loss is finite, and the loss vectors of the three steps are bit-identical between
    the two runs (identical tables mean identical steps)."""
    for i, name in enumerate(("scene0000_00", "scene0001_00")):
        scan = D.write_scan(str(tmp_path / "scans"), name, seed=20 + i, side=40)
        D.write_pseudo(str(tmp_path / "pm"), name, scan, seed=20 + i, K=5, compact=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, *a], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    r = run("tools/dataset_from_scans.py", "--scans", str(tmp_path / "scans"), "--pseudo", str(tmp_path / "pm"),
            "--out", str(tmp_path / "data"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["scans"] == {"train": 2}
    lines = []
    for extra in ([], ["--host-tables"]):
        out = tmp_path / ("run_host" if extra else "run_device")
        r = run("tools/train.py", "--data-dir", str(tmp_path / "data"), "--steps", "3", "--out", str(out), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["device_tables"] == (not extra) and line["steps"] == 3 and line["skipped"] == 0
        assert len(line["losses_per_step"]) == 3 and np.isfinite(np.array(line["losses_per_step"])).all()
        assert (out / "last.ckpt").exists()
        lines.append(line)
    assert lines[0]["loss_names"] == lines[1]["loss_names"] and len(lines[0]["loss_names"]) > 0
    assert lines[0]["losses_per_step"] == lines[1]["losses_per_step"]
