"""CPU: the dataset builder's readers, the database round trip, the colour statistics and the threshold rounding the
device mask tables rely on (datasets/preprocessing.py, datasets/freemask.py, pseudo_masks/scans.py)."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_cases as D


@pytest.mark.parametrize("fmt", ["binary_little_endian", "ascii"])
def test_vertex_properties_of_a_hand_written_scan(tmp_path, fmt):
    """Mesh and labels PLY in both formats, segs / aggregation json: raw integer colours, labels, and the mesh reader
    beside it unchanged."""
    from unscene3d_amd.datasets import preprocessing as P
    from unscene3d_amd.pseudo_masks import scans

    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5], [2, 2, 2]], np.float32)
    rgb = np.array([[0, 1, 2], [255, 254, 253], [127, 128, 129], [10, 20, 30], [200, 100, 50]], np.uint8)
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3]], np.int32)
    label = np.array([1, 5, 39, 40, 0])
    d = tmp_path / "scene0007_01"
    d.mkdir()
    mesh, lab = d / "scene0007_01_vh_clean_2.ply", d / "scene0007_01_vh_clean_2.labels.ply"
    D.write_ply(mesh, xyz, rgb, faces, fmt=fmt)
    D.write_ply(lab, xyz, rgb, faces, label=label, fmt=fmt)
    got = scans.read_ply_vertex_properties(mesh, ("red", "green", "blue", "x"))
    assert [got[n].dtype for n in ("red", "green", "blue", "x")] == [np.uint8] * 3 + [np.float32]
    assert np.array_equal(np.stack([got["red"], got["green"], got["blue"]], 1), rgb)     # as stored: no / 255 round trip
    assert np.array_equal(got["x"], xyz[:, 0])
    got = scans.read_ply_vertex_properties(lab, ("label",))
    assert got["label"].dtype == np.uint16 and np.array_equal(got["label"], label)
    v, c, f = scans.read_ply_mesh(mesh)                                 # the mesh reader's return value is as before
    assert np.array_equal(v, xyz) and np.array_equal(f, faces) and c.dtype == np.float32
    assert np.array_equal(c, (rgb.astype(np.float64) / 255.0).astype(np.float32))
    assert P.parse_scene_dir(d) == ("scene0007_01", 7, 1)

    segs = np.array([30, 30, 7, 7, 1000])
    labels = P.scene_labels(segs, label, [{"id": 0, "segments": [30]}, {"id": 1, "segments": [7, 1000]},
                                          {"id": 2, "segments": [1000]}])
    # labels 5 and 39 are foreground -> 1; 1, 40 and 0 are outside the list and KEEP their id, their instances go
    assert labels.tolist() == [[1, -1], [1, 0], [1, 1], [40, -1], [0, -1]]
    assert labels.dtype == np.int64


def test_reader_errors_name_the_file(tmp_path):
    from unscene3d_amd.datasets import preprocessing as P
    from unscene3d_amd.pseudo_masks import scans

    xyz = np.zeros((3, 3), np.float32)
    path = tmp_path / "nolabel.ply"
    D.write_ply(path, xyz, np.zeros((3, 3), np.uint8), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match="nolabel.ply.*'label'"):
        scans.read_ply_vertex_properties(path, ("label",))
    plain = tmp_path / "plain.ply"
    D.write_ply(plain, xyz)
    with pytest.raises(ValueError, match="plain.ply.*'red'"):
        scans.read_ply_vertex_properties(plain, ("red",))
    short = tmp_path / "short.ply"
    short.write_bytes(path.read_bytes()[:-40])
    with pytest.raises(ValueError, match="short.ply"):
        scans.read_ply_vertex_properties(short, ("x",))
    for bad in ("scene12_00", "scene0000_0", "scan0000_00", "scene0000_00_x"):
        with pytest.raises(ValueError, match=bad):
            P.parse_scene_dir(tmp_path / bad)
        with pytest.raises(ValueError, match=bad):
            P.build_dataset(tmp_path, {"train": [bad]}, tmp_path, tmp_path / "out", device="cpu")
    assert not (tmp_path / "out" / "train").exists()                  # refused before anything was written for the mode
    info = tmp_path / "scene0000_00.txt"
    info.write_text("axisAlignment = 1 0 0\n")
    with pytest.raises(ValueError, match="scene0000_00.txt"):
        P.read_axis_alignment(info)
    info.write_text("sceneType = Office\n")
    assert np.array_equal(P.read_axis_alignment(info), np.identity(4))


@pytest.mark.parametrize("thr", [0.35, 0.3])
def test_threshold_is_rounded_to_f32_once(thr):
    """A threshold that is no f32 number against soft values at f32(thr) and its two neighbours: numpy's
    `f32 array > python float` and torch's tensor > scalar both compare against f32(thr) — the one rounding the device
    tables make (`float thr` in the kernel's argument list).  f32(0.35) lies below 0.35, f32(0.3) above 0.3: there a
    comparison in double would set the entry AT f32(thr), and neither library does."""
    t = np.float32(thr)
    assert float(t) != thr
    vals = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1)), 0.0, 1.0, 0.5], np.float32)
    expect = vals > t
    assert expect.tolist() == [False, False, True, False, True, True]
    assert (float(t) > thr) == (thr == 0.3)
    assert bool(np.float64(vals[1]) > thr) == (thr == 0.3)             # what a double comparison would give
    assert np.array_equal(vals > thr, expect)
    assert np.array_equal((torch.from_numpy(vals) > thr).numpy(), expect)
    assert np.array_equal((torch.from_numpy(vals).reshape(2, 3) > thr).numpy().reshape(-1), expect)


def test_database_round_trip_and_colour_statistics(tmp_path):
    from unscene3d_amd.datasets import preprocessing as P
    from unscene3d_amd.datasets.freemask import entries_from_database, load_color_mean_std

    rng = np.random.default_rng(5)
    entries = []
    for i in range(3):
        rgb = rng.integers(0, 256, (50 + i, 3)).astype(np.uint8).astype(np.float64)
        assert P.color_moments(rgb) == ([float((rgb[:, j] / 255).mean()) for j in range(3)],       # :162-171 restated
                                        [float(((rgb[:, j] / 255) ** 2).mean()) for j in range(3)])
        entries.append({"filepath": str(tmp_path / "train" / f"{i:04}_00.npy"), "scene": i, "sub_scene": 0,
                        "raw_filepath": f"/scans/scene{i:04}_00/scene{i:04}_00_vh_clean_2.ply", "file_len": 50 + i,
                        "color_mean": [float((rgb[:, j] / 255).mean()) for j in range(3)],
                        "color_std": [float(((rgb[:, j] / 255) ** 2).mean()) for j in range(3)]})
    P.save_yaml(tmp_path / "train_database.yaml", entries)
    assert entries_from_database(tmp_path / "train_database.yaml") == entries           # floats survive the text form

    stats = P.color_mean_std(entries)
    mean = np.array([e["color_mean"] for e in entries]).mean(axis=0)                    # :222-240 restated
    std = np.sqrt(np.array([e["color_std"] for e in entries]).mean(axis=0) - mean ** 2)
    assert stats == {"mean": [float(v) for v in mean], "std": [float(v) for v in std]}
    P.save_yaml(tmp_path / "color_mean_std.yaml", stats)
    assert load_color_mean_std(tmp_path / "color_mean_std.yaml") == (tuple(stats["mean"]), tuple(stats["std"]))

    (tmp_path / "bad.yaml").write_text(json.dumps({"mean": [1, 2]}))
    with pytest.raises(ValueError, match="bad.yaml"):
        load_color_mean_std(tmp_path / "bad.yaml")
    with pytest.raises(ValueError, match="bad.yaml"):
        entries_from_database(tmp_path / "bad.yaml")


def test_mask_table_cases_hold_what_they_claim():
    """The GPU test's inputs, checked on the host with a plain numpy extent filter: the limit column is kept, the two
    wide ones are not, the empty one has no entry above the threshold although it has entries AT it."""
    for N, K in D.TABLE_SHAPES:
        seen = set()
        for xyz, soft, seg, where in D.mask_table_cases(N, K, 0.35):
            seen |= set(where)
            hard = soft > np.float32(0.35)
            scene = (xyz[:, :2].max(0) - xyz[:, :2].min(0)) * np.float32(0.8)
            keep = []
            for j in range(K):
                if hard[:, j].any():
                    pts = xyz[hard[:, j], :2]
                    if not ((pts.max(0) - pts.min(0)) > scene).any():
                        keep.append(j)
            if "empty" in where:
                assert not hard[:, where["empty"]].any() and (soft[:, where["empty"]] == np.float32(0.35)).any()
            if N >= 8:
                assert where.get("limit", -1) in keep + [-1]
                assert where.get("wide_x", -1) not in keep and where.get("wide_y", -1) not in keep
                if "limit" in where:
                    pts = xyz[hard[:, where["limit"]], :2]
                    assert np.array_equal(pts.max(0) - pts.min(0), scene)
                if "last_row" in where:
                    assert np.flatnonzero(hard[:, where["last_row"]]).tolist() == [N - 1]
                if "at_thr" in where:
                    assert hard[:, where["at_thr"]].sum() == 1
        assert seen == set(D.FEATURES)
