"""CPU: the scan-directory readers of unscene3d_amd/pseudo_masks/scans.py (PLY, info file, poses, frame pairing,
intrinsics) on files the tests write themselves, and the float64 restatement of the token-grid sampling
(tests/token_projection_ref.py) against torch's bilinear resize."""
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_projection_ref as T
from unscene3d_amd.pseudo_masks import scans


# ----------------------------------------------------------------------------------------------------------- PLY
def _mesh(rng, n_vertices=9, n_faces=7):
    xyz = rng.standard_normal((n_vertices, 3)).astype(np.float32)
    rgba = rng.integers(0, 256, (n_vertices, 4)).astype(np.uint8)
    extra = rng.standard_normal(n_vertices)                        # a double `quality` between position and colour
    faces = np.stack([rng.permutation(n_vertices)[:3] for _ in range(n_faces)]).astype(np.int32)
    return xyz, rgba, extra, faces


def _header(fmt, n_vertices, n_faces, count_type):
    return ("ply\nformat %s 1.0\ncomment written by the test\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty double quality\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property uchar alpha\nelement face %d\nproperty list %s int vertex_indices\nend_header\n"
            % (fmt, n_vertices, n_faces, count_type)).encode()


def _write_binary(path, xyz, rgba, extra, faces, count_type="uchar", fmt="binary_little_endian"):
    with open(path, "wb") as f:
        f.write(_header(fmt, len(xyz), len(faces), count_type))
        for p, q, c in zip(xyz, extra, rgba):
            f.write(struct.pack("<3fd4B", *p, q, *c))
        for face in faces:
            f.write(struct.pack("<B" if count_type == "uchar" else "<i", len(face)))
            f.write(struct.pack("<%di" % len(face), *face))


def _write_ascii(path, xyz, rgba, extra, faces, count_type="uchar"):
    with open(path, "wb") as f:
        f.write(_header("ascii", len(xyz), len(faces), count_type))
        for p, q, c in zip(xyz, extra, rgba):
            f.write(("%r %r %r %r %d %d %d %d\n" % (float(p[0]), float(p[1]), float(p[2]), float(q), *c)).encode())
        for face in faces:
            f.write((" ".join(str(v) for v in (len(face), *face)) + "\n").encode())


@pytest.mark.parametrize("writer", [_write_binary, _write_ascii])
@pytest.mark.parametrize("count_type", ["uchar", "int"])
def test_ply_reader_binary_and_ascii(tmp_path, writer, count_type):
    xyz, rgba, extra, faces = _mesh(np.random.default_rng(0))
    path = tmp_path / "mesh.ply"
    writer(path, xyz, rgba, extra, faces, count_type)
    v, c, f = scans.read_ply_mesh(path)
    assert v.dtype == np.float32 and c.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, xyz) and np.array_equal(f, faces)
    assert np.array_equal(c, (rgba[:, :3] / 255.0).astype(np.float32)) and c.min() >= 0 and c.max() <= 1


@pytest.mark.parametrize("writer", [_write_binary, _write_ascii])
def test_ply_reader_rejects_a_quad_and_names_the_file(tmp_path, writer):
    xyz, rgba, extra, faces = _mesh(np.random.default_rng(1))
    mixed = [list(f) for f in faces[:3]] + [[0, 1, 2, 3]] + [list(f) for f in faces[3:]]
    path = tmp_path / "quad.ply"
    writer(path, xyz, rgba, extra, mixed)
    with pytest.raises(ValueError, match=r"quad\.ply.*face 3 is not a triangle"):
        scans.read_ply_mesh(path)


def test_ply_reader_rejects_big_endian_and_unknown_types(tmp_path):
    xyz, rgba, extra, faces = _mesh(np.random.default_rng(2))
    path = tmp_path / "big.ply"
    _write_binary(path, xyz, rgba, extra, faces, fmt="binary_big_endian")
    with pytest.raises(ValueError, match=r"big\.ply.*binary_big_endian"):
        scans.read_ply_mesh(path)
    odd = tmp_path / "odd.ply"
    odd.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty half x\nend_header\n")
    with pytest.raises(ValueError, match=r"odd\.ply"):
        scans.read_ply_mesh(odd)


# ------------------------------------------------------------------------------------------------- info and poses
AXIS = [0.945519, 0.325568, 0.0, -5.38439, -0.325568, 0.945519, 0.0, -2.87178, 0.0, 0.0, 1.0, -0.06435, 0.0, 0.0, 0.0, 1.0]


def _info(path, axis=True):
    lines = ["axisAlignment = " + " ".join(repr(v) for v in AXIS)] if axis else []
    lines += ["colorHeight = 968", "colorWidth = 1296", "depthHeight = 480", "fx_color = 1170.187988",
              "fy_color = 1170.187988", "mx_color = 647.75", "my_color = 483.75", "sceneType = Living room / Lounge"]
    path.write_text("\n".join(lines) + "\n")
    return path


def test_info_parser_with_and_without_axis_alignment(tmp_path):
    info = scans.read_scan_info(_info(tmp_path / "a.txt"))
    assert np.array_equal(info["axisAlignment"], np.array(AXIS).reshape(4, 4))
    assert (info["colorHeight"], info["colorWidth"]) == (968, 1296) and isinstance(info["colorHeight"], int)
    assert (info["fx_color"], info["fy_color"], info["mx_color"], info["my_color"]) == (1170.187988, 1170.187988, 647.75,
                                                                                      483.75)
    assert info["sceneType"] == "Living room / Lounge" and info["depthHeight"].tolist() == [480.0]
    assert np.array_equal(scans.read_scan_info(tmp_path / "a.txt", align=False)["axisAlignment"], np.identity(4))
    assert np.array_equal(scans.read_scan_info(_info(tmp_path / "b.txt", axis=False))["axisAlignment"], np.identity(4))
    (tmp_path / "c.txt").write_text("colorHeight = 968\n")
    with pytest.raises(ValueError, match="colorWidth"):
        scans.read_scan_info(tmp_path / "c.txt")


def test_intrinsics_follow_the_reference_formula(tmp_path):
    """scannet.py:133-138 written out: fx and mx are scaled by the HEIGHT ratio, fy and my by the WIDTH ratio."""
    info = scans.read_scan_info(_info(tmp_path / "a.txt"))
    depth_shape = (192, 256)
    orig_color_shape = np.array([info["colorHeight"], info["colorWidth"]])
    color_scale = [depth_shape[0] / orig_color_shape[0], depth_shape[1] / orig_color_shape[1]]
    want = np.array([info["fx_color"] * color_scale[0], info["fy_color"] * color_scale[1],
                     info["mx_color"] * color_scale[0], info["my_color"] * color_scale[1]])
    got = scans.color_intrinsics(info, depth_shape)
    assert np.array_equal(got, want)
    assert got[0] != got[1]                                          # equal focal lengths, unequal ratios: the quirk shows


def _pose_text(m):
    return "\n".join(" ".join(repr(float(v)) for v in row) for row in m) + "\n"


def test_pose_parsing(tmp_path):
    m = np.random.default_rng(3).standard_normal((4, 4))
    (tmp_path / "p.txt").write_text(_pose_text(m))
    assert np.array_equal(scans.read_pose(tmp_path / "p.txt"), m)
    (tmp_path / "lost.txt").write_text("-inf -inf -inf -inf\n" * 4)
    assert np.isneginf(scans.read_pose(tmp_path / "lost.txt")).all()
    (tmp_path / "short.txt").write_text("1 0 0\n0 1 0\n")
    with pytest.raises(ValueError, match="short.txt"):
        scans.read_pose(tmp_path / "short.txt")


def _frames(tmp_path, names, lost=(), H=6, W=8):
    color, pose = tmp_path / "color", tmp_path / "pose"
    color.mkdir()
    pose.mkdir()
    rng = np.random.default_rng(4)
    rgb, poses = {}, {}
    for k, name in enumerate(names):
        rgb[name] = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        np.save(color / f"{name}.npy", rgb[name])
        poses[name] = np.identity(4)
        poses[name][:3, 3] = [k + 1, 2 * k, -k]
        (pose / f"{name}.txt").write_text("-inf -inf -inf -inf\n" * 4 if name in lost else _pose_text(poses[name]))
    return color, pose, rgb, poses


def test_frames_pair_in_lexicographic_order(tmp_path):
    """sorted() of the names, as the reference pairs them: 0, 100, 20 — not numeric order."""
    color, pose, rgb, poses = _frames(tmp_path, ["0", "20", "100"])
    pairs = scans.frame_files(color, pose)
    assert [os.path.basename(c) for c, _ in pairs] == ["0.npy", "100.npy", "20.npy"]
    assert [os.path.basename(p) for _, p in pairs] == ["0.txt", "100.txt", "20.txt"]
    axis = np.array(AXIS).reshape(4, 4)
    images, got_poses, dropped = scans.load_frames(color, pose, (6, 8), axis_alignment=axis)
    assert dropped == 0 and images.shape == (3, 3, 6, 8) and images.dtype == np.float32
    for k, name in enumerate(["0", "100", "20"]):
        want = ((rgb[name] / 255.0).astype(np.float32) - np.float32(0.5)) / np.float32(0.5)
        assert np.array_equal(images[k], want.transpose(2, 0, 1))
        assert np.array_equal(got_poses[k], axis @ poses[name])
    assert images.min() >= -1 and images.max() <= 1
    assert [os.path.basename(c) for c, _ in scans.frame_files(color, pose, every=2)] == ["0.npy", "20.npy"]
    os.remove(pose / "20.txt")
    with pytest.raises(ValueError, match="same frames"):
        scans.frame_files(color, pose)


def test_non_finite_poses_are_dropped_and_counted(tmp_path):
    color, pose, rgb, poses = _frames(tmp_path, ["000", "001", "002", "003"], lost=("001", "003"))
    images, got_poses, dropped = scans.load_frames(color, pose, (6, 8))
    assert dropped == 2 and images.shape[0] == 2 and np.isfinite(got_poses).all()
    assert np.array_equal(got_poses[1], poses["002"])
    with pytest.raises(ValueError, match=r"uint8 \[5, 8, 3\]"):
        scans.load_frames(color, pose, (5, 8))


def test_png_frame_loads_like_the_direct_pillow_call(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    path = str(tmp_path / "f.png")
    Image.fromarray(rng.integers(0, 256, (30, 44, 3)).astype(np.uint8)).save(path)
    H, W = 12, 16
    rgb = np.array(Image.open(path).convert("RGB").resize((W, H), Image.BILINEAR)).astype(int)
    want = (torch.from_numpy(rgb / 255.).permute(2, 0, 1).float() - 0.5) / 0.5        # scannet.py:144, :115
    assert np.array_equal(scans.load_image(path, (H, W)), want.numpy())


# ---------------------------------------------------------------------------------- the sampling's f64 restatement
# Worst |restatement - torch| measured on the CPU with exactly these inputs (unit-normal f32 tokens, seed 0): 6.85e-7,
# 1.03e-6 and 1.48e-5.  The restatement uses the exact scale gh/H in f64; torch rounds the scale to f32 (relative 6e-8),
# which moves a source position near the far edge by 192 * 0.245 * 6e-8 = 3e-6 cells, and a neighbouring-token
# difference of up to 5 turns that into 1.5e-5 — the 47x63 figure.  The bounds are twice the measured values.
@pytest.mark.parametrize("gh,gw,H,W,C,bound", [(5, 7, 24, 32, 70, 2 * 6.85e-7), (4, 6, 20, 28, 70, 2 * 1.03e-6),
                                              (47, 63, 192, 256, 16, 2 * 1.48e-5)])
def test_f64_sampling_restatement_against_torch_resize(gh, gw, H, W, C, bound):
    tok = np.random.default_rng(0).standard_normal((gh, gw, C)).astype(np.float32)
    want = T.resize(tok, H, W)
    maps = F.interpolate(torch.from_numpy(tok).permute(2, 0, 1)[None].contiguous(), size=(H, W), mode="bilinear")
    err = float(np.abs(maps[0].permute(1, 2, 0).double().numpy() - want).max())
    print(f"grid {gh}x{gw} -> {H}x{W}: worst |f64 restatement - torch f32| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the taps clamp at both borders and the first / last pixels sit outside the outermost cell centres
    y0, y1, ly = T.taps(H, gh)
    assert y0[0] == 0 and ly[0] == 0 and y0[-1] == y1[-1] == gh - 1
