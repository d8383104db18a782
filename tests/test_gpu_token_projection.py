"""usc_project_fuse_tokens through `Project2DFeaturesCUDA.fuse_frames_tokens`: several frames' token grids sampled at
the hit pixels and folded into the scene's running mean in one launch — against today's path (`DinoNet._to_image` on the
same tokens, then `fuse_frame` frame by frame) and against the float64 restatement tests/token_projection_ref.py, with
the hits of the CPU ray-cast oracle oracle/project_ref.py.

Scene: room_voxels(3) (7120 voxels), five cameras of camera_views(9, ...) with frame 1 re-aimed from outside the room
into empty space and frames 2 and 3 swapped, so that the first three frames already hold an overlapping pair.  Counts of
the oracle on the CPU for these seeds (24x32 / 20x28 images): rows hit by >= 2 frames of the five-frame call 287 / 236
(of the first three frames 285 / 236), rows with >= 2 pixels in one frame 736 / 461, frames that hit nothing 1 / 1, hit
pixels in image row 0: 128 / 112, row H-1: 128 / 112, column 0: 96 / 80, column W-1: 96 / 80 (every ray of the four
inside frames hits: the room is closed)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import token_projection_ref as T
from oracle import project_ref as PR
from unscene3d_amd.synthetic import camera_views, look_at, room_voxels

pytestmark = pytest.mark.gpu
F = np.float32
DMIN, DMAX, INC = 0.1 / 0.02, 0.9 / 0.02, 0.01
SIZES = {(24, 32): (5, 7), (20, 28): (4, 6)}            # image -> token grid at stride 4; 20x28 clamps at both borders
AWAY = 1


@functools.lru_cache(maxsize=None)
def _scene(H, W):
    """-> coords, views f32[1,5,4,4], intr f32[1,4], hit i32[5,H,W] of the CPU oracle (computed once, read only)."""
    coords = room_voxels(3)
    views = camera_views(9, coords, 5)
    hi = coords[:, 1:].max(0).astype(np.float64)
    views[0, AWAY] = look_at(hi + 30.0, hi + 60.0)
    views[0, [2, 3]] = views[0, [3, 2]]
    occ, shifts = PR.dense_occupancy(coords)
    intr = np.array([[W * 0.9, W * 0.9, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.4]], F)
    hit = PR.first_hit(occ, PR.shift_views(views, shifts), intr, W, H, DMIN, DMAX, INC)[0]
    for a in (coords, views, intr, hit):
        a.setflags(write=False)
    return coords, views, intr, hit


@functools.lru_cache(maxsize=None)
def _dinonet():
    from unscene3d_amd.models.encoders_2d import DinoNet

    cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_feature="descriptors",
                                                     dino_vit_layer=9, dino_vit_stride=4))
    return DinoNet(cfg)


def _projecter(H, W):
    from unscene3d_amd import project_features_cuda as P

    return P.Project2DFeaturesCUDA(width=W, height=H, voxel_size=0.02, depth_min=DMIN * 0.02, depth_max=DMAX * 0.02)


def _inputs(H, W, C, V, device, seed=0):
    coords, views, intr, hit = _scene(H, W)
    gh, gw = SIZES[(H, W)]
    rng = np.random.default_rng(1000 * seed + C + V)
    tokens = rng.standard_normal((V, gh, gw, C)).astype(F)
    sentinel = rng.standard_normal((coords.shape[0], C)).astype(F)      # every row has bits of its own to keep
    dev = lambda a: torch.from_numpy(np.array(a)).to(device)          # a copy: the cached arrays are read-only
    return dev(coords), dev(views[:, :V]), dev(intr), hit[:V], tokens, sentinel


@pytest.mark.parametrize("H,W", list(SIZES))
def test_the_scene_exercises_the_kernel(H, W):
    """The non-vacuity counts of the module docstring, on the oracle's hits."""
    coords, _, _, hit = _scene(H, W)
    _, frames_hit, pixels = T.fuse_frames(np.zeros((coords.shape[0], 1)), np.zeros((5,) + SIZES[(H, W)] + (1,)), hit)
    assert int((frames_hit >= 2).sum()) >= 20
    assert int(((pixels[:3] > 0).sum(0) >= 2).sum()) >= 20
    assert int((pixels >= 2).any(0).sum()) >= 20
    assert pixels[AWAY].sum() == 0 and (pixels.sum(1) == 0).sum() >= 1
    ok = hit >= 0
    assert ok[:, 0].any() and ok[:, H - 1].any() and ok[:, :, 0].any() and ok[:, :, W - 1].any()


@pytest.mark.parametrize("V", [1, 3, 5])
@pytest.mark.parametrize("C", [6, 70, 384, 512])      # 512: the channel limit, all eight accumulators of a lane in use
@pytest.mark.parametrize("H,W", list(SIZES))
def test_fused_tokens_against_the_map_path_and_f64(device, H, W, C, V):
    """Worst error against f64 of the fused call <= 2 x the worst error of today's path + 1e-6 * max |feature|; rows no
    frame hits keep the sentinel's bits; frames_hit equals the oracle's count.  Measured on an MI355X over the
    18 cases with C <= 384: fused 3.5e-7 ... 9.6e-7, map path 2.8e-7 ... 6.3e-7 at max |feature| 1.9 ... 3.3 (the bound
    is 2.5e-6 ... 4.5e-6)."""
    coords, views, intr, hit, tokens, sentinel = _inputs(H, W, C, V, device)
    proj = _projecter(H, W)
    ref, ref_frames, _ = T.fuse_frames(sentinel, tokens, hit)
    tok_d = torch.from_numpy(tokens).to(device)

    fused = torch.from_numpy(sentinel).to(device)
    frames_hit, _ = proj.fuse_frames_tokens(fused, tok_d, coords, views, intr)
    assert frames_hit.dtype == torch.int32 and np.array_equal(frames_hit.cpu().numpy(), ref_frames)

    maps = _dinonet()._to_image(tok_d.reshape(V, -1, C), (1, V, 3, H, W))          # [1, V, H, W, C]
    old = torch.from_numpy(sentinel).to(device)
    for v in range(V):
        proj.fuse_frame(old, maps[:, v:v + 1].contiguous(), coords, views[:, v:v + 1].contiguous(), intr)

    seen = ref_frames > 0
    assert seen.any() and not seen.all()
    fused, old = fused.cpu().numpy(), old.cpu().numpy()
    assert np.array_equal(fused[~seen].view(np.int32), sentinel[~seen].view(np.int32))
    assert np.array_equal(old[~seen].view(np.int32), sentinel[~seen].view(np.int32))
    scale = float(np.abs(ref[seen]).max())
    err_fused, err_old = float(np.abs(fused - ref).max()), float(np.abs(old - ref).max())
    print(f"{H}x{W} C={C} V={V}: worst |fused - f64| {err_fused:.3e}, worst |map path - f64| {err_old:.3e}, "
          f"max |feature| {scale:.3f}")
    assert err_fused <= 2 * err_old + 1e-6 * scale


@pytest.mark.parametrize("H,W,C", [(24, 32, 384), (20, 28, 70), (20, 28, 512)])
def test_grouping_frames_into_calls_keeps_the_bits(device, H, W, C):
    coords, views, intr, _, tokens, sentinel = _inputs(H, W, C, 5, device)
    proj = _projecter(H, W)
    tok_d = torch.from_numpy(tokens).to(device)
    results, counts = [], []
    for groups in ([5], [2, 3], [1, 1, 1, 1, 1]):
        scene = torch.from_numpy(sentinel).to(device)
        total, v0 = torch.zeros(coords.shape[0], dtype=torch.int32, device=device), 0
        for g in groups:
            n_hit, _ = proj.fuse_frames_tokens(scene, tok_d[v0:v0 + g].contiguous(), coords,
                                               views[:, v0:v0 + g].contiguous(), intr)
            total += n_hit
            v0 += g
        results.append(scene.cpu().numpy().view(np.int32))
        counts.append(total.cpu().numpy())
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], counts[2])
    assert not np.array_equal(results[0], sentinel.view(np.int32))


def test_hit_seg_passed_back_equals_a_fresh_cast(device):
    H, W, C, V = 24, 32, 70, 3
    coords, views, intr, _, tokens, sentinel = _inputs(H, W, C, V, device)
    query = torch.from_numpy(np.random.default_rng(7).standard_normal(tokens.shape).astype(F)).to(device)
    proj = _projecter(H, W)
    key_scene = torch.from_numpy(sentinel).to(device)
    n_key, cast = proj.fuse_frames_tokens(key_scene, torch.from_numpy(tokens).to(device), coords, views, intr)
    reused, fresh = torch.from_numpy(sentinel).to(device), torch.from_numpy(sentinel).to(device)
    n_reused, _ = proj.fuse_frames_tokens(reused, query, coords, views, intr, hit_seg=cast)
    n_fresh, _ = proj.fuse_frames_tokens(fresh, query, coords, views, intr)
    assert torch.equal(reused, fresh) and torch.equal(n_reused, n_fresh) and torch.equal(n_reused, n_key)
    assert not torch.equal(reused, key_scene)


def test_arguments_are_checked_before_the_launch(device):
    H, W = 24, 32
    coords, views, intr, _, tokens, sentinel = _inputs(H, W, 6, 3, device)
    proj = _projecter(H, W)
    scene = torch.from_numpy(sentinel).to(device)
    tok_d = torch.from_numpy(tokens).to(device)
    with pytest.raises(RuntimeError, match="view_matrices"):
        proj.fuse_frames_tokens(scene, tok_d[:2].contiguous(), coords, views, intr)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        proj.fuse_frames_tokens(scene[:, :5].contiguous(), tok_d, coords, views, intr)
    wide = torch.zeros((3, 5, 7, 513), device=device)
    with pytest.raises(RuntimeError, match="513 channels"):
        proj.fuse_frames_tokens(torch.zeros((coords.shape[0], 513), device=device), wide, coords, views, intr)
    assert torch.equal(scene, torch.from_numpy(sentinel).to(device))
