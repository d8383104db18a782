"""Float64 oracle of the DINO ViT-S/8 extractor tests: an independent restatement, in plain functional torch and numpy,
of what the reference computes (models/encoders_2d/dino.py over third_party/dino_vit/extractor.py, DINO's
VisionTransformer).  It does not import the module under test.

The reference's own extractor cannot be imported where these tests run: `timm` and `torchvision` are not installed.

The position-embedding interpolation is written out by hand (cubic convolution, A = -0.75, source coordinate
(dst + 0.5) / scale - 0.5, taps clamped to the grid): it checks the module's `F.interpolate` call for the scale
convention (the SCALE FACTOR (n + 0.1) / 28 maps the coordinates, not the size ratio n / 28) instead of repeating it."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dino_vits8_state_dict.json")
DIM, HEADS, DEPTH, PATCH, GRID0 = 384, 6, 12, 8, 28


def golden_shapes():
    with open(GOLDEN) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def random_state_dict(seed: int):
    """float64 tensors: normal, std 0.02; LayerNorm weights one, LayerNorm biases zero."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in golden_shapes().items():
        if "norm" in name:
            sd[name] = torch.ones(shape, dtype=torch.float64) if name.endswith("weight") else torch.zeros(shape, dtype=torch.float64)
        else:
            sd[name] = torch.randn(shape, generator=g, dtype=torch.float64) * 0.02
    return sd


def _cubic_taps(n_in: int, n_out: int, scale: float):
    """-> index i64[n_out, 4] (clamped) and weight f64[n_out, 4] of the cubic convolution with A = -0.75."""
    A = -0.75
    idx = np.zeros((n_out, 4), np.int64)
    wgt = np.zeros((n_out, 4), np.float64)
    for o in range(n_out):
        src = (o + 0.5) / scale - 0.5
        i0 = math.floor(src)
        t = src - i0

        def near(x):     # |x| <= 1
            return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

        def far(x):      # 1 < |x| < 2
            return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

        w = (far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t))
        for k in range(4):
            idx[o, k] = min(max(i0 - 1 + k, 0), n_in - 1)
            wgt[o, k] = w[k]
    return idx, wgt


def resize_bicubic_by_scale(grid: np.ndarray, out_h: int, out_w: int, scale_h: float, scale_w: float) -> np.ndarray:
    """grid f64[h, w, c] -> f64[out_h, out_w, c]"""
    ih, wh = _cubic_taps(grid.shape[0], out_h, scale_h)
    iw, ww = _cubic_taps(grid.shape[1], out_w, scale_w)
    rows = (grid[ih] * wh[:, :, None, None]).sum(1)                 # [out_h, w, c]
    return (rows[:, iw] * ww[None, :, :, None]).sum(2)              # [out_h, out_w, c]


def pos_embed(sd, H: int, W: int, stride: int) -> np.ndarray:
    """f64 [1 + gh*gw, 384]; grid rows follow the image height."""
    pe = sd["pos_embed"].double().numpy()[0]
    gh, gw = 1 + (H - PATCH) // stride, 1 + (W - PATCH) // stride
    grid = resize_bicubic_by_scale(pe[1:].reshape(GRID0, GRID0, DIM), gh, gw, (gh + 0.1) / GRID0, (gw + 0.1) / GRID0)
    return np.concatenate([pe[:1], grid.reshape(gh * gw, DIM)], 0)


def qkv_at(sd, images: torch.Tensor, layer: int, stride: int = 4, dtype=torch.float64):
    """images [B, 3, H, W] -> (q, k, v), each [B, heads, T, 64], of block `layer`, everything in `dtype`."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = images.to(dtype)
    B, _, H, W = x.shape
    x = F.conv2d(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=stride)      # [B, 384, gh, gw]
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([p["cls_token"].expand(B, -1, -1), x], 1) + torch.from_numpy(pos_embed(sd, H, W, stride)).to(dtype)
    T = x.shape[1]

    def split(t):        # [B, T, 1152] -> q, k, v [B, heads, T, 64]
        t = t.reshape(B, T, 3, HEADS, DIM // HEADS)
        return tuple(t[:, :, i].transpose(1, 2) for i in range(3))

    for i in range(layer + 1):
        b = f"blocks.{i}."
        y = F.layer_norm(x, (DIM,), p[b + "norm1.weight"], p[b + "norm1.bias"], 1e-6)
        q, k, v = split(F.linear(y, p[b + "attn.qkv.weight"], p[b + "attn.qkv.bias"]))
        if i == layer:
            return q, k, v
        a = torch.softmax(q @ k.transpose(-1, -2) * (DIM // HEADS) ** -0.5, -1) @ v            # [B, heads, T, 64]
        x = x + F.linear(a.transpose(1, 2).reshape(B, T, DIM), p[b + "attn.proj.weight"], p[b + "attn.proj.bias"])
        y = F.layer_norm(x, (DIM,), p[b + "norm2.weight"], p[b + "norm2.bias"], 1e-6)
        y = F.gelu(F.linear(y, p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"]))
        x = x + F.linear(y, p[b + "mlp.fc2.weight"], p[b + "mlp.fc2.bias"])
    raise AssertionError("unreachable")


def _linear_taps(n_in: int, n_out: int, dtype):
    """Bilinear resize to a SIZE, align_corners=False: source (dst + 0.5) * n_in / n_out - 0.5, clamped at 0."""
    src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp(min=0.0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    t = (src - i0).to(dtype)
    return i0, i1, t


def _to_image(tok: torch.Tensor, n: int, H: int, W: int, stride: int) -> torch.Tensor:
    """tokens [n, gh*gw, 384] -> [1, n, H, W, 384], bilinear, written out (rows first, then columns)"""
    gh, gw = 1 + (H - PATCH) // stride, 1 + (W - PATCH) // stride
    g = tok.reshape(n, gh, gw, DIM)
    r0, r1, tr = _linear_taps(gh, H, tok.dtype)
    c0, c1, tc = _linear_taps(gw, W, tok.dtype)
    rows = g[:, r0] * (1 - tr)[None, :, None, None] + g[:, r1] * tr[None, :, None, None]
    out = rows[:, :, c0] * (1 - tc)[None, None, :, None] + rows[:, :, c1] * tc[None, None, :, None]
    return out.reshape(1, n, H, W, DIM)


def dinonet(sd, images: torch.Tensor, feature: str, layer: int, stride: int = 4, dtype=torch.float64):
    """images [1, n, 3, H, W] -> (features, None) for 'descriptors' (column d*6 + head of block `layer`'s key) or
    (keys, queries) for 'attention' (column head*64 + d of the last block), each [1, n, H, W, 384], class token dropped."""
    _, n, _, H, W = images.shape
    q, k, _ = qkv_at(sd, images[0], layer if feature != "attention" else DEPTH - 1, stride, dtype)
    d = DIM // HEADS
    if feature == "attention":
        cols = [(h, e) for h in range(HEADS) for e in range(d)]          # c = head*64 + d
    else:
        cols = [(h, e) for e in range(d) for h in range(HEADS)]          # c = d*6 + head

    def columns(t):      # [n, heads, T, 64] -> [n, T - 1, 384]
        return torch.stack([t[:, h, 1:, e] for h, e in cols], -1)

    key = _to_image(columns(k), n, H, W, stride)
    if feature != "attention":
        return key, None
    return key, _to_image(columns(q), n, H, W, stride)


def attention_f64(q: np.ndarray, k: np.ndarray, v: np.ndarray, scale: float):
    """q, k, v [T, 64] of one head (any float dtype) -> (o f64[T, 64], sum_j p_ij |v_jd| f64[T, 64])."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = (q @ k.T) * scale
    p = np.exp(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return p @ v, p @ np.abs(v)


def rel_l2(a, b) -> float:
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())
