"""Scan directory -> scene file -> pseudo masks, end to end on the device: unscene3d_amd/pseudo_masks/scans.build_scene,
tools/scene_files_from_scans.py and the hand-over to tools/pseudo_masks_run.py.  The scan is written by the test: a
synthetic.make_mesh height field (3 x 3 m) as binary PLY, an info file with a rotation + translation as axisAlignment,
six 24 x 32 .npy frames looking down at the mesh plus one frame whose pose is -inf."""
import importlib.util
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import token_projection_ref as T
from oracle import sparse_ref as R
from unscene3d_amd.synthetic import look_at, make_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, VOXEL, MIN_VERTS = 24, 32, 0.06, 20
A = np.deg2rad(25.0)
AXIS = np.array([[np.cos(A), -np.sin(A), 0, 0.7], [np.sin(A), np.cos(A), 0, -1.1], [0, 0, 1, 0.25], [0, 0, 0, 1]])


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _aligned(vertices):
    return np.hstack([vertices.astype(np.float64), np.ones((len(vertices), 1))]) @ AXIS.T[:, :3]


def write_scan(scan_dir):
    """-> (vertices, faces, colors) of the mesh as a PLY reader returns them (colours through uint8)."""
    scene = os.path.basename(scan_dir)
    os.makedirs(os.path.join(scan_dir, "color"))
    os.makedirs(os.path.join(scan_dir, "pose"))
    vertices, faces, colors = make_mesh(3)
    rgb = np.round(colors * 255).astype(np.uint8)
    with open(os.path.join(scan_dir, f"{scene}_vh_clean_2.ply"), "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(vertices), len(faces))).encode())
        for p, c in zip(vertices, rgb):
            f.write(struct.pack("<3f4B", *p, *c, 255))
        for face in faces:
            f.write(struct.pack("<B3i", 3, *face))
    with open(os.path.join(scan_dir, f"{scene}.txt"), "w") as f:
        f.write("axisAlignment = " + " ".join(repr(float(v)) for v in AXIS.ravel()) + "\n")
        f.write("colorHeight = 48\ncolorWidth = 64\nfx_color = 57.6\nfy_color = 57.6\nmx_color = 31.5\nmy_color = 23.5\n")
    xyz = _aligned(vertices)
    lo, hi = xyz.min(0), xyz.max(0)
    rng = np.random.default_rng(11)
    inv_axis = np.linalg.inv(AXIS)
    for k in range(7):
        name = f"{k * 20:06d}"
        np.save(os.path.join(scan_dir, "color", name + ".npy"), rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        if k == 4:                                                  # tracking lost
            text = "-inf -inf -inf -inf\n" * 4
        else:
            eye = np.array([*(lo[:2] + (hi[:2] - lo[:2]) * rng.uniform(0.3, 0.7, 2)), hi[2] + 1.2])
            target = np.array([*(lo[:2] + (hi[:2] - lo[:2]) * rng.uniform(0.2, 0.8, 2)), lo[2]])
            pose = inv_axis @ look_at(eye, target, up=(0, 1, 0)).astype(np.float64)   # the file holds the unaligned pose
            text = "\n".join(" ".join(repr(float(v)) for v in row) for row in pose) + "\n"
        with open(os.path.join(scan_dir, "pose", name + ".txt"), "w") as f:
            f.write(text)
    return vertices, faces, (rgb / 255.0).astype(np.float32)


def _encoder(device, feature="descriptors"):
    from unscene3d_amd.models.encoders_2d import DinoNet
    from unscene3d_amd.models.encoders_2d.dino import init_random_weights

    cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_feature=feature,
                                                     dino_vit_layer=9, dino_vit_stride=4))
    net = DinoNet(cfg)
    init_random_weights(net.vit, 0)
    return net.to(device).eval()


@pytest.fixture(scope="module")
def scan(tmp_path_factory, device):
    from unscene3d_amd.pseudo_masks import scans

    scan_dir = str(tmp_path_factory.mktemp("scans") / "scene0000_00")
    mesh = write_scan(scan_dir)
    model = _encoder(device)
    kw = dict(voxel_size=VOXEL, image_hw=(H, W), segments_min_verts=MIN_VERTS, device=device)
    return SimpleNamespace(dir=scan_dir, mesh=mesh, model=model, batched=scans.build_scene(scan_dir, model, frame_batch=4, **kw),
                           per_frame=scans.build_scene(scan_dir, model, frame_batch=None, **kw))


def test_build_scene_gives_the_documented_arrays(scan):
    s = scan.batched
    vertices, faces, colors = scan.mesh
    xyz = _aligned(vertices)
    grid = np.floor(xyz * (1.0 / VOXEL)).astype(np.int64)
    kept, _ = R.sparse_quantize(grid)                               # first occurrence, vertex order
    n = len(kept)
    assert 1000 < n < len(vertices)                                  # the voxelisation merges vertices
    assert set(s) == {"coords", "colors", "feats_2d", "segment_ids", "seg_connectivity", "full_res_coords", "voxel_size",
                      "frames_used", "frames_dropped"}
    assert s["coords"].dtype == np.int32 and s["coords"].shape == (n, 4) and not s["coords"][:, 0].any()
    assert np.array_equal(s["coords"][:, 1:], grid[kept])
    assert s["colors"].dtype == np.float32 and np.array_equal(s["colors"], colors[kept] - np.float32(0.5))
    assert s["feats_2d"].dtype == np.float32 and s["feats_2d"].shape == (n, 384)
    assert s["segment_ids"].dtype == np.int64 and s["segment_ids"].shape == (n,)
    assert s["seg_connectivity"].dtype == np.int64 and s["seg_connectivity"].shape[1] == 2
    assert s["full_res_coords"].dtype == np.float32 and np.array_equal(s["full_res_coords"], xyz.astype(np.float32))
    assert s["voxel_size"] == VOXEL and (s["frames_used"], s["frames_dropped"]) == (6, 1)


def test_segments_are_segment_mesh_at_the_kept_vertices(scan, device):
    from unscene3d_amd import felzenszwalb_cpp

    vertices, faces, colors = scan.mesh
    xyz = _aligned(vertices)
    kept, _ = R.sparse_quantize(np.floor(xyz * (1.0 / VOXEL)).astype(np.int64))
    seg, conn = felzenszwalb_cpp.segment_mesh(xyz.astype(np.float32), faces, colors, 0.005, MIN_VERTS, device=device)
    assert len(np.unique(seg)) >= 3
    assert np.array_equal(scan.batched["segment_ids"], seg[kept]) and np.array_equal(scan.batched["seg_connectivity"], conn)


@pytest.mark.parametrize("feature", ["descriptors", "attention"])
def test_forward_tokens_is_forward_before_the_resize(device, feature):
    """`forward_tokens` pinned to `forward`, bit for bit: the grids it returns, resized by `_to_image`, ARE the maps
    `forward` returns — same block, same facet, same column order, key and query not swapped."""
    net = _encoder(device, feature)
    images = torch.randn((1, 3, 3, H, W), generator=torch.Generator().manual_seed(5)).to(device)
    key_map, query_map = net(images)
    key, query = net.forward_tokens(images)
    assert key.shape == (3, 5, 7, 384) and key.dtype == torch.float32 and key.is_contiguous()
    assert torch.equal(net._to_image(key.reshape(3, 35, 384), images.shape), key_map) and bool(key_map.any())
    if feature == "attention":
        assert query.shape == key.shape and not torch.equal(query, key)
        assert torch.equal(net._to_image(query.reshape(3, 35, 384), images.shape), query_map)
    else:
        assert query is None and query_map is None


def _compare_with_the_per_frame_path(scan_dir, model, device, batched, per_frame, attention):
    """Features of frame_batch=4 against frame_batch=None (`batched`, `per_frame`: build_scene's dicts), for the key
    features and, with `attention`, the query features.

    Yardstick: the f64 restatement on the tokens of every frame encoded alone (`forward_tokens`, which
    test_forward_tokens_is_forward_before_the_resize pins to `forward`) and the device's own hits.  Three assertions:
      1. the map path itself is an f32 evaluation of that restatement: worst error <= cap, with u = 2^-24 and every term
         relative to max |token| (features are convex combinations of tokens): 12 u for the bilinear sample (4 products,
         3 sums, the weights' own rounding), cnt_max u for the pixel sum, 2 u per folded frame, and 2 max(gh, gw) u for
         torch's f32 scale gh / H, which moves a source position by up to max(gh, gw) u cells between tokens at most
         2 max |token| apart;
      2. the issue's bound: worst error of the batched path <= 2 x worst error of the map path + 1e-6 max |feature|
         + d, d = the worst difference between a frame's tokens encoded in a batch of four and alone (a token difference
         d moves a convex combination by at most d);
      3. the two arrays directly: |batched - per frame| <= 3 cap + 1e-6 max |feature| + d (1. and 2. together).
    Voxels no frame saw are all-zero rows in both."""
    from unscene3d_amd import project_features_cuda as P
    from unscene3d_amd.pseudo_masks import scans

    info = scans.read_scan_info(os.path.join(scan_dir, "scene0000_00.txt"))
    images, poses, dropped = scans.load_frames(os.path.join(scan_dir, "color"), os.path.join(scan_dir, "pose"), (H, W),
                                               axis_alignment=info["axisAlignment"])
    assert dropped == 1 and images.shape == (6, 3, H, W)
    poses[:, :3, 3] /= VOXEL
    imgs = torch.from_numpy(images).to(device).unsqueeze(0)
    alone = [model.forward_tokens(imgs[:, i:i + 1]) for i in range(6)]
    grouped = [model.forward_tokens(imgs[:, i:i + 4]) for i in (0, 4)]
    coords = torch.from_numpy(batched["coords"]).to(device)
    proj = P.Project2DFeaturesCUDA(width=W, height=H, voxel_size=VOXEL)
    intr = torch.from_numpy(scans.color_intrinsics(info, (H, W)).astype(np.float32)).to(device).view(1, 4)
    _, hit, _ = proj._cast_views(coords, torch.from_numpy(poses.astype(np.float32)).to(device).unsqueeze(0), intr, False)
    n = coords.shape[0]
    for which, name in ((0, "feats_2d"), (1, "feats_2d_query"))[:2 if attention else 1]:
        tok_alone = torch.cat([t[which] for t in alone])
        tok_grouped = torch.cat([t[which] for t in grouped])
        assert tok_alone.shape == (6, 5, 7, 384)
        d_tokens = float((tok_alone - tok_grouped).abs().max())
        ref, frames_hit, pixels = T.fuse_frames(np.zeros((n, 384)), tok_alone.cpu().numpy(), hit[0].cpu().numpy())
        seen = frames_hit > 0
        assert seen.sum() > 200 and (~seen).sum() > 20 and int((frames_hit >= 2).sum()) > 20
        got, old = batched[name], per_frame[name]
        assert not got[~seen].any() and not old[~seen].any() and np.abs(got[seen]).sum(1).min() > 0
        scale, tok_max = float(np.abs(ref).max()), float(tok_alone.abs().max())
        cap = (12 + int(pixels.max()) + 2 * 6 + 2 * 7) * 2.0 ** -24 * tok_max
        err_got, err_old = float(np.abs(got - ref).max()), float(np.abs(old - ref).max())
        diff = float(np.abs(got - old).max())
        print(f"build_scene {name}: worst |frame_batch=4 - f64| {err_got:.3e}, worst |frame_batch=None - f64| {err_old:.3e} "
              f"(cap {cap:.3e}), |frame_batch=4 - None| {diff:.3e}, max |feature| {scale:.3f}, max |token| {tok_max:.3f}, "
              f"token difference batch of 4 vs alone {d_tokens:.3e}, most pixels on a voxel {int(pixels.max())}")
        assert err_old <= cap
        assert err_got <= 2 * err_old + 1e-6 * scale + d_tokens
        assert diff <= 3 * cap + 1e-6 * scale + d_tokens


def test_batched_features_against_the_per_frame_path(scan, device):
    """Measured on an MI355X: 7.99e-7 (frame_batch=4) and 1.69e-7 (None) against f64 at max |feature| 1.115, tokens of a
    batch of four within 1.6e-6 of the frame encoded alone."""
    _compare_with_the_per_frame_path(scan.dir, scan.model, device, scan.batched, scan.per_frame, attention=False)


def test_attention_mode_against_the_per_frame_path(scan, device):
    from unscene3d_amd.pseudo_masks import scans

    model = _encoder(device, "attention")
    kw = dict(voxel_size=VOXEL, image_hw=(H, W), segments_min_verts=MIN_VERTS, attention=True, device=device)
    batched = scans.build_scene(scan.dir, model, frame_batch=4, **kw)
    per_frame = scans.build_scene(scan.dir, model, frame_batch=None, **kw)
    assert batched["feats_2d_query"].shape == batched["feats_2d"].shape and batched["feats_2d_query"].dtype == np.float32
    assert not np.array_equal(batched["feats_2d_query"], batched["feats_2d"])
    assert not np.array_equal(batched["feats_2d"], scan.batched["feats_2d"])          # the last block's key, not block 9's
    _compare_with_the_per_frame_path(scan.dir, model, device, batched, per_frame, attention=True)


def _old_encode_scene_feats_2d(model, images, camera_poses, color_intrinsics, coords, projecter, attention=False):
    """The loop of pipeline.encode_scene_feats_2d before `frame_batch` existed — the comparator for its default path."""
    n = coords.shape[0]
    scene_key = scene_query = None
    with torch.no_grad():
        for i, img in enumerate(images[0]):
            key_features, query_features = model(img.unsqueeze(0).unsqueeze(0))
            if scene_key is None:
                C = key_features.shape[-1]
                scene_key = torch.zeros((n, C), dtype=torch.float32, device=coords.device)
                scene_query = torch.zeros_like(scene_key) if attention else None
            view = camera_poses[0, i].unsqueeze(0).unsqueeze(0)
            _, cast = projecter.fuse_frame(scene_key, key_features, coords, view, color_intrinsics)
            if attention:
                projecter.fuse_frame(scene_query, query_features, coords, view, color_intrinsics, hit_seg=cast)
    return (scene_key, scene_query) if attention else scene_key


def test_default_arguments_keep_the_per_frame_path_bit_for_bit(scan, device):
    from unscene3d_amd import project_features_cuda as P
    from unscene3d_amd.pseudo_masks import pipeline, scans

    info = scans.read_scan_info(os.path.join(scan.dir, "scene0000_00.txt"))
    images, poses, _ = scans.load_frames(os.path.join(scan.dir, "color"), os.path.join(scan.dir, "pose"), (H, W),
                                         axis_alignment=info["axisAlignment"])
    poses[:, :3, 3] /= VOXEL
    args = (torch.from_numpy(images).to(device).unsqueeze(0), torch.from_numpy(poses.astype(np.float32)).to(device).unsqueeze(0),
            torch.from_numpy(scans.color_intrinsics(info, (H, W)).astype(np.float32)).to(device).view(1, 4),
            torch.from_numpy(scan.batched["coords"]).to(device))
    want = _old_encode_scene_feats_2d(scan.model, *args, P.Project2DFeaturesCUDA(width=W, height=H, voxel_size=VOXEL))
    got = pipeline.encode_scene_feats_2d(scan.model, *args, P.Project2DFeaturesCUDA(width=W, height=H, voxel_size=VOXEL))
    assert torch.equal(got, want) and bool(got.any())
    assert np.array_equal(scan.per_frame["feats_2d"], want.cpu().numpy())
    with pytest.raises(RuntimeError, match="forward_tokens"):
        pipeline.encode_scene_feats_2d(lambda img: None, *args, None, frame_batch=2)
    with pytest.raises(ValueError, match="frame_batch"):
        pipeline.encode_scene_feats_2d(scan.model, *args, None, frame_batch=0)


def test_tool_writes_the_scene_file_once_and_the_mask_tool_reads_it(scan, device, tmp_path, capsys):
    tool = _tool("scene_files_from_scans")
    out = str(tmp_path / "scenes")
    argv = ["--scans", os.path.dirname(scan.dir), "--out", out, "--random-weights", "0", "--frame-batch", "4",
            "--height", str(H), "--width", str(W), "--voxel-size", str(VOXEL), "--segments-min-verts", str(MIN_VERTS)]
    assert tool.main(argv) == 0
    assert "1 of 1 scans" in capsys.readouterr().out
    path = os.path.join(out, "scene0000_00.npz")
    assert os.listdir(out) == ["scene0000_00.npz"]
    z = np.load(path)
    for k in ("coords", "segment_ids", "seg_connectivity", "full_res_coords", "colors"):
        assert np.array_equal(z[k], scan.batched[k]), k
    assert z["feats_2d"].shape == scan.batched["feats_2d"].shape and int(z["frames_dropped"]) == 1
    stamp = os.stat(path).st_mtime_ns
    assert tool.main(argv) == 0
    printed = capsys.readouterr().out
    assert "scene file exists: scene0000_00" in printed and "0 of 1 scans" in printed
    assert os.stat(path).st_mtime_ns == stamp

    masks_tool = _tool("pseudo_masks_run")
    masks_out = str(tmp_path / "masks")
    ncut_args = dict(affinity_tau=0.6, max_number_of_instances=20, min_segment_size=4, separation_mode="max",
                     max_extent_ratio=0.8)
    name, n_masks, _ = masks_tool.process_scene(path, masks_out, device, ncut_args)
    cloud = np.load(os.path.join(masks_out, "scene0000_00_cloud.npy"))
    masks = np.load(os.path.join(masks_out, "scene0000_00_masks.npy"))
    assert name == "scene0000_00" and np.array_equal(cloud, scan.batched["full_res_coords"])
    assert masks.dtype == bool and masks.shape == (cloud.shape[0], n_masks)
