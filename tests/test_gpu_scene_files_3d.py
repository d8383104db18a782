"""The 3D branch of the scan builder (unscene3d_amd/pseudo_masks/scans.py::build_scene with `model_3d`, `images=False`) and
the command lines around it (tools/scene_files_from_scans.py --csc-*/--no-images, tools/pseudo_masks_run.py --modality) on
a synthetic scan directory: a floor and two boxes, an info file, two .npy frames with poses."""
import os
import struct
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from unscene3d_amd.synthetic import look_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, VOXEL, MIN_VERTS = 24, 32, 0.06, 20
SCENE = "scene0001_00"


def _patch(origin, u, v, nu, nv, base):
    """An nu x nv grid of vertices spanning origin + s*u + t*v, two triangles per quad -> (vertices, faces)."""
    s, t = np.meshgrid(np.linspace(0, 1, nu), np.linspace(0, 1, nv), indexing="ij")
    verts = np.asarray(origin, float) + s[..., None] * np.asarray(u, float) + t[..., None] * np.asarray(v, float)
    i = (np.arange(nu - 1)[:, None] * nv + np.arange(nv - 1)[None, :]).ravel() + base
    faces = np.concatenate([np.stack([i, i + nv, i + 1], 1), np.stack([i + 1, i + nv, i + nv + 1], 1)])
    return verts.reshape(-1, 3), faces


def _mesh():
    """A 3 m x 3 m floor and two boxes standing on it (top and four sides each): 2590 vertices."""
    parts, faces, n = [], [], 0

    def add(origin, u, v, nu, nv):
        nonlocal n
        p, f = _patch(origin, u, v, nu, nv, n)
        parts.append(p)
        faces.append(f)
        n += p.shape[0]

    add((0, 0, 0), (3, 0, 0), (0, 3, 0), 30, 30)
    for (x, y), (a, b, h) in (((0.5, 0.6), (0.8, 0.6, 0.7)), ((1.8, 1.7), (0.7, 0.9, 0.45))):
        add((x, y, h), (a, 0, 0), (0, b, 0), 13, 13)
        add((x, y, 0.02), (a, 0, 0), (0, 0, h - 0.02), 13, 13)
        add((x, y + b, 0.02), (a, 0, 0), (0, 0, h - 0.02), 13, 13)
        add((x, y, 0.02), (0, b, 0), (0, 0, h - 0.02), 13, 13)
        add((x + a, y, 0.02), (0, b, 0), (0, 0, h - 0.02), 13, 13)
    vertices = np.concatenate(parts).astype(np.float32)
    rgb = np.clip(vertices * 70 + 20, 0, 255).astype(np.uint8)      # colour follows position
    return vertices, np.concatenate(faces).astype(np.int32), rgb


def write_scan(scan_dir, frames=True):
    scene = os.path.basename(scan_dir)
    os.makedirs(scan_dir)
    vertices, faces, rgb = _mesh()
    with open(os.path.join(scan_dir, f"{scene}_vh_clean_2.ply"), "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(vertices), len(faces))).encode())
        for p, c in zip(vertices, rgb):
            f.write(struct.pack("<3f3B", *p, *c))
        for face in faces:
            f.write(struct.pack("<B3i", 3, *face))
    with open(os.path.join(scan_dir, f"{scene}.txt"), "w") as f:
        f.write("colorHeight = 48\ncolorWidth = 64\nfx_color = 57.6\nfy_color = 57.6\nmx_color = 31.5\nmy_color = 23.5\n")
    if frames:
        os.makedirs(os.path.join(scan_dir, "color"))
        os.makedirs(os.path.join(scan_dir, "pose"))
        rng = np.random.default_rng(6)
        for k, (eye, target) in enumerate((((1.2, 1.0, 2.6), (1.0, 1.2, 0.0)), ((2.0, 1.8, 2.4), (2.1, 2.0, 0.0)))):
            np.save(os.path.join(scan_dir, "color", f"{k:06d}.npy"), rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
            pose = look_at(np.array(eye), np.array(target), up=(0, 1, 0)).astype(np.float64)
            with open(os.path.join(scan_dir, "pose", f"{k:06d}.txt"), "w") as f:
                f.write("\n".join(" ".join(repr(float(v)) for v in row) for row in pose) + "\n")
    return len(vertices)


def _encoder(device):
    from unscene3d_amd.models.encoders_2d import DinoNet
    from unscene3d_amd.models.encoders_2d.dino import init_random_weights

    cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_feature="descriptors",
                                                     dino_vit_layer=9, dino_vit_stride=4))
    net = DinoNet(cfg)
    init_random_weights(net.vit, 0)
    return net.to(device).eval()


@pytest.fixture(scope="module")
def scan(tmp_path_factory, device):
    from unscene3d_amd.models.weights import load_csc_backbone
    from unscene3d_amd.pseudo_masks import scans

    root = tmp_path_factory.mktemp("scans3d")
    scan_dir = str(root / "with_frames" / SCENE)
    n_vertices = write_scan(scan_dir)
    bare_dir = str(root / "no_frames" / SCENE)
    write_scan(bare_dir, frames=False)
    torch.manual_seed(0)
    model_3d = load_csc_backbone({}, device=device)
    model = _encoder(device)
    kw = dict(voxel_size=VOXEL, image_hw=(H, W), segments_min_verts=MIN_VERTS, frame_batch=2, device=device)
    return SimpleNamespace(dir=scan_dir, bare_dir=bare_dir, n_vertices=n_vertices, model=model, model_3d=model_3d, kw=kw,
                           both=scans.build_scene(scan_dir, model, model_3d=model_3d, **kw),
                           color=scans.build_scene(scan_dir, model, **kw))


def test_feats_3d_is_the_brute_force_lift_bit_for_bit(scan, device):
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import ops
    from unscene3d_amd.pseudo_masks.pipeline import encode_scene_feats_3d

    s = scan.both
    n = s["coords"].shape[0]
    assert 2000 <= scan.n_vertices <= 3000 and 1000 < n <= scan.n_vertices
    assert s["feats_3d"].dtype == np.float32 and s["feats_3d"].shape == (n, 96) and s["resolution_scale"] == 2
    assert np.isfinite(s["feats_3d"]).all() and np.abs(s["feats_3d"]).max() > 0

    def sinput():
        return ME.SparseTensor(features=torch.from_numpy(s["colors"]).to(device),
                               coordinates=torch.from_numpy(s["coords"]).to(device), device=device)

    brute = encode_scene_feats_3d(scan.model_3d, sinput(), resolution_scale=2, nn="brute")
    assert np.array_equal(s["feats_3d"].view(np.uint32), brute.cpu().numpy().view(np.uint32))
    grid = encode_scene_feats_3d(scan.model_3d, sinput(), resolution_scale=2, nn="grid")
    assert torch.equal(grid, brute)
    # the two lifts gather the same rows
    with torch.no_grad():
        _, fmaps = scan.model_3d(sinput())
    enc = fmaps["res_2"]
    hr, lr = torch.from_numpy(s["coords"][:, 1:]).to(device).float().contiguous(), enc.C[:, 1:].float().contiguous()
    assert enc.tensor_stride[0] == 2 and lr.shape[0] < n
    d_b, i_b = ops.knn1(hr, lr)
    d_g, i_g = ops.knn1_grid(hr, lr, cell=2.0)
    assert torch.equal(i_b, i_g) and torch.equal(d_b, d_g)
    with pytest.raises(ValueError):
        encode_scene_feats_3d(scan.model_3d, sinput(), nn="kdtree")


def test_without_model_3d_nothing_changes(scan):
    both, color = scan.both, scan.color
    assert set(color) == {"coords", "colors", "feats_2d", "segment_ids", "seg_connectivity", "full_res_coords",
                          "voxel_size", "frames_used", "frames_dropped"}
    assert set(both) == set(color) | {"feats_3d", "resolution_scale"}
    for k in color:
        assert np.array_equal(np.asarray(color[k]), np.asarray(both[k])), k
    assert both["frames_used"] == 2 and np.abs(both["feats_2d"]).max() > 0
    assert list(both)[:3] == ["coords", "colors", "feats_2d"] and list(color)[-2:] == ["frames_used", "frames_dropped"]


def test_geometry_only_scene(scan):
    from unscene3d_amd.pseudo_masks import scans

    geom = scans.build_scene(scan.dir, None, model_3d=scan.model_3d, images=False, **scan.kw)
    assert set(geom) == {"coords", "colors", "feats_3d", "resolution_scale", "segment_ids", "seg_connectivity",
                         "full_res_coords", "voxel_size"}
    for k in geom:
        assert np.array_equal(np.asarray(geom[k]), np.asarray(scan.both[k])), k
    bare = scans.build_scene(scan.bare_dir, None, model_3d=scan.model_3d, **scan.kw)     # no color/, no pose/
    assert set(bare) == set(geom) and np.array_equal(bare["feats_3d"], geom["feats_3d"])
    with pytest.raises(ValueError, match="model_3d"):
        scans.build_scene(os.path.join(scan.dir, "does-not-exist"), scan.model, images=False, **scan.kw)
    # today's behaviour: an image encoder and no usable frame -> feats_2d of zeros
    zeros = scans.build_scene(scan.bare_dir, scan.model, **scan.kw)
    assert zeros["feats_2d"].shape == (geom["coords"].shape[0], 384) and not zeros["feats_2d"].any()
    assert zeros["frames_used"] == 0 and "feats_3d" not in zeros


def _run(tool, *argv):
    """A tool of the repository in a fresh child process under its own time limit -> CompletedProcess."""
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *argv], capture_output=True, text=True,
                          timeout=300)


def test_command_lines(scan, tmp_path):
    common = ["--height", str(H), "--width", str(W), "--voxel-size", str(VOXEL), "--segments-min-verts", str(MIN_VERTS)]
    scenes, geom_scenes = str(tmp_path / "scenes"), str(tmp_path / "scenes_geom")
    r = _run("scene_files_from_scans.py", "--scans", os.path.dirname(scan.dir), "--out", scenes, "--csc-random-weights", "0",
             "--random-weights", "0", "--frame-batch", "2", *common)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(os.path.join(scenes, SCENE + ".npz"))
    assert np.array_equal(z["coords"], scan.both["coords"]) and int(z["resolution_scale"]) == 2
    assert np.array_equal(z["feats_3d"], scan.both["feats_3d"])          # seed 0, as the fixture's backbone
    assert z["feats_2d"].shape == scan.both["feats_2d"].shape and int(z["frames_used"]) == 2
    r = _run("scene_files_from_scans.py", "--scans", os.path.dirname(scan.dir), "--out", geom_scenes,
             "--csc-random-weights", "0", "--no-images", *common)
    assert r.returncode == 0, r.stderr[-2000:]
    zg = np.load(os.path.join(geom_scenes, SCENE + ".npz"))
    assert "feats_2d" not in zg.files and np.array_equal(zg["feats_3d"], z["feats_3d"])

    n_full = scan.both["full_res_coords"].shape[0]
    for src, modality in ((scenes, "both"), (scenes, "geom"), (scenes, "color"), (geom_scenes, "geom")):
        out = str(tmp_path / f"masks_{os.path.basename(src)}_{modality}")
        r = _run("pseudo_masks_run.py", "--scenes", src, "--out", out, "--modality", modality)
        assert r.returncode == 0, r.stderr[-2000:]
        cloud, masks = np.load(os.path.join(out, SCENE + "_cloud.npy")), np.load(os.path.join(out, SCENE + "_masks.npy"))
        assert cloud.shape == (n_full, 3) and masks.dtype == bool and masks.shape[0] == n_full
    out = str(tmp_path / "masks_refused")
    r = _run("pseudo_masks_run.py", "--scenes", geom_scenes, "--out", out, "--modality", "color")
    assert r.returncode != 0 and "RuntimeError" in r.stderr
    assert SCENE + ".npz: needs feats_2d for --modality color" in r.stderr
    assert not os.path.exists(os.path.join(out, SCENE + "_cloud.npy"))
