"""TEST INFRASTRUCTURE ONLY — float64 restatement of the token-grid projection (usc_project_fuse_tokens,
include/usc3d.h): the bilinear resize `DinoNet._to_image` asks torch for, sampled at the hit pixels only, and the
per-frame running mean of pseudo_masks/unscene3d_pseudo_main.py:311-313.  Everything is float64 with the EXACT scale
gh / H (torch and the kernel round the scale and every product to f32), so it is the yardstick both f32 paths are
measured against.  Shared by tests/test_scans_host.py, tests/test_gpu_token_projection.py and
tests/test_gpu_scene_files.py."""
import numpy as np


def taps(n_out, n_in):
    """Half-pixel-centre source taps of a resize from n_in cells to n_out pixels -> (i0, i1 int[n_out], lam f64[n_out])."""
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), src - i0


def sample(grid, y0, y1, ly, x0, x1, lx):
    """grid f64[gh, gw, C]; taps of the wanted pixels (arrays of one length n) -> f64[n, C]."""
    ly, lx = ly[:, None], lx[:, None]
    return (1 - ly) * ((1 - lx) * grid[y0, x0] + lx * grid[y0, x1]) + ly * ((1 - lx) * grid[y1, x0] + lx * grid[y1, x1])


def resize(grid, H, W):
    """grid [gh, gw, C] -> f64[H, W, C]: F.interpolate(size=(H, W), mode='bilinear') in float64."""
    grid = np.asarray(grid, np.float64)
    y0, y1, ly = taps(H, grid.shape[0])
    x0, x1, lx = taps(W, grid.shape[1])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    return sample(grid, y0[ys], y1[ys], ly[ys], x0[xs], x1[xs], lx[xs]).reshape(H, W, -1)


def fuse_frames(scene, tokens, hit):
    """scene [n, C] (any float), tokens [V, gh, gw, C], hit int[V, H, W] (voxel row, -1 = none) ->
    (scene f64[n, C] after folding the V frames in order, frames_hit int[n], pixels int[V, n]).  Rows no frame hits keep
    their value."""
    scene = np.array(scene, np.float64)
    tokens = np.asarray(tokens, np.float64)
    V, H, W = hit.shape
    n = scene.shape[0]
    y0, y1, ly = taps(H, tokens.shape[1])
    x0, x1, lx = taps(W, tokens.shape[2])
    frames_hit = np.zeros(n, np.int64)
    pixels = np.zeros((V, n), np.int64)
    for v in range(V):
        ys, xs = np.nonzero(hit[v] >= 0)
        if ys.size == 0:
            continue
        rows = hit[v, ys, xs]
        vals = sample(tokens[v], y0[ys], y1[ys], ly[ys], x0[xs], x1[xs], lx[xs])
        total = np.zeros_like(scene)
        np.add.at(total, rows, vals)
        cnt = np.bincount(rows, minlength=n)
        m = cnt > 0
        scene[m] = (scene[m] + total[m] / (cnt[m, None] + 10e-5)) / 2.0
        frames_hit += m
        pixels[v] = cnt
    return scene, frames_hit, pixels
