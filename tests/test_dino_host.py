"""DINO ViT-S/8 image encoder on the host (unscene3d_amd/models/encoders_2d): state_dict layout, the module against the
float64 oracle of tests/vit_ref.py, the position-embedding scale convention, and the argument checks of the attention
entry point.  No GPU: on CPU tensors the module is plain torch operators.

The oracle is an independent restatement; the reference's own extractor cannot be imported here (`timm` and
`torchvision` are not installed)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vit_ref as R

H_IMG, W_IMG, N_FRAMES, LAYER = 40, 56, 2, 10       # 9 x 13 patch grid, 118 tokens, not square


def _config(feature):
    return SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_stride=4,
                                                      dino_vit_layer=LAYER, dino_vit_feature=feature))


@functools.lru_cache(maxsize=None)
def _case():
    """weights, images and the oracle's outputs (f64 and f32 runs), computed once and not modified"""
    sd = R.random_state_dict(0)
    images = torch.randn((1, N_FRAMES, 3, H_IMG, W_IMG), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = {"sd": sd, "images": images}
    for feature in ("descriptors", "attention"):
        out[feature, "f64"] = R.dinonet(sd, images, feature, LAYER)
        out[feature, "f32"] = R.dinonet(sd, images, feature, LAYER, dtype=torch.float32)
    return out


def _net(feature, dtype):
    from unscene3d_amd.models.encoders_2d import DinoNet

    net = DinoNet(_config(feature), dataset=None).to(dtype).eval()
    net.vit.load_state_dict(_case()["sd"], strict=True)
    return net


def test_state_dict_is_the_published_layout():
    from unscene3d_amd.models.encoders_2d import DinoViT

    model = DinoViT()
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = R.golden_shapes()
    assert len(want) == 150
    assert got == want
    assert list(got) == list(want) or sorted(got) == sorted(want)
    sd = dict(model.state_dict())
    sd["blocks.0.attn.qkv.weights"] = sd.pop("blocks.0.attn.qkv.weight")       # one wrong key
    with pytest.raises(RuntimeError):
        DinoViT().load_state_dict(sd, strict=True)


@pytest.mark.parametrize("feature", ["descriptors", "attention"])
def test_module_matches_oracle_f64(feature):
    """Same arithmetic in another order: 1e-10 relative.  The oracle builds the columns one by one, so both column orders
    (descriptors d*6 + head, attention head*64 + d) are checked, and its position embedding is the hand-written one."""
    c = _case()
    with torch.no_grad():
        got = _net(feature, torch.float64)(c["images"])
    want = c[feature, "f64"]
    assert got[0].shape == (1, N_FRAMES, H_IMG, W_IMG, 384) and got[0].dtype == torch.float64
    if feature == "descriptors":
        assert got[1] is None
    for g, w in zip(got, want):
        if w is None:
            continue
        assert g.shape == w.shape
        rel = float((g - w).abs().max() / w.abs().max())
        print(f"{feature} f64: max rel {rel:.2e}")
        assert rel <= 1e-10


def test_column_orders_differ_and_are_kept():
    """Descriptor column d*6 + head and attention-mode column head*64 + d of the same block are a fixed permutation."""
    c = _case()
    net = _net("descriptors", torch.float64)
    net.layer = R.DEPTH - 1
    with torch.no_grad():
        desc, _ = net(c["images"])
        net.vit_feature = "attention"
        key, _ = net(c["images"])
    perm = torch.tensor([h * 64 + d for d in range(64) for h in range(6)])
    assert torch.equal(desc, key[..., perm])
    assert not torch.equal(desc, key)


@pytest.mark.parametrize("feature", ["descriptors", "attention"])
def test_module_f32_error_is_the_oracles(feature):
    """f32 module against the f64 oracle: relative L2 no larger than 4x that of the oracle itself run in f32 (the margin
    allows for a different summation order)."""
    c = _case()
    with torch.no_grad():
        got = _net(feature, torch.float32)(c["images"].float())
    for g, w64, w32 in zip(got, c[feature, "f64"], c[feature, "f32"]):
        if w64 is None:
            continue
        assert g.dtype == torch.float32
        err, base = R.rel_l2(g, w64), R.rel_l2(w32, w64)
        print(f"{feature} f32: module {err:.3e}, oracle in f32 {base:.3e}")
        assert err <= 4 * base


def test_two_frames_equal_two_single_frames_bitwise():
    c = _case()
    net = _net("descriptors", torch.float32)
    images = c["images"].float()
    with torch.no_grad():
        both, _ = net(images)
        singles = [net(images[:, i:i + 1])[0] for i in range(N_FRAMES)]
    assert torch.equal(both, torch.cat(singles, 1))


def test_position_embedding_follows_the_scale_factor_not_the_size():
    """Hand-built: channel 0 of the 28x28 embedding is the row index, channel 1 the column index, so the resampled
    embedding shows which source coordinate each grid cell read.  The scale-factor form reads (o + 0.5) * 28 / (n + 0.1)
    - 0.5, the size form (o + 0.5) * 28 / n - 0.5: up to 0.16 source cells apart on the 9-row grid.  The module must equal
    `F.interpolate(scale_factor=)` and the oracle's hand-written cubic convolution, and differ from `size=`."""
    import torch.nn.functional as F

    from unscene3d_amd.models.encoders_2d import DinoViT

    model = DinoViT().double()
    pe = torch.zeros(1, 785, 384, dtype=torch.float64)
    rows, cols = torch.meshgrid(torch.arange(28.0, dtype=torch.float64), torch.arange(28.0, dtype=torch.float64), indexing="ij")
    pe[0, 1:, 0], pe[0, 1:, 1] = rows.reshape(-1), cols.reshape(-1)
    pe[0, 0, :2] = -7.0
    with torch.no_grad():
        model.pos_embed.copy_(pe)
        got = model.interpolated_pos_embed(H_IMG, W_IMG)
    gh, gw = 9, 13
    assert got.shape == (1, 1 + gh * gw, 384)
    assert torch.equal(got[0, 0], pe[0, 0])                                   # class position untouched, in front
    grid = got[0, 1:].reshape(gh, gw, 384)                                    # rows follow the image height
    src = pe[:, 1:].reshape(1, 28, 28, 384).permute(0, 3, 1, 2)
    by_scale = F.interpolate(src, scale_factor=((gh + 0.1) / 28, (gw + 0.1) / 28), mode="bicubic", align_corners=False,
                             recompute_scale_factor=False).permute(0, 2, 3, 1)[0]
    by_size = F.interpolate(src, size=(gh, gw), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)[0]
    assert by_scale.shape == by_size.shape == grid.shape
    assert float((by_size[..., :2] - by_scale[..., :2]).abs().max()) > 0.1    # the two conventions are far apart here
    assert float((grid - by_scale).abs().max()) < 1e-12
    assert float((grid[:, 3, 0] - by_scale[:, 0, 0]).abs().max()) < 1e-12     # channel 0 varies with the ROW only
    assert float((grid[4, :, 1] - by_scale[0, :, 1]).abs().max()) < 1e-12     # channel 1 with the column only
    # the whole resampled embedding equals the oracle's hand-written cubic convolution
    want = R.pos_embed({"pos_embed": pe}, H_IMG, W_IMG, 4)
    assert float(np.abs(got[0].numpy() - want).max()) < 1e-12
    # cached per (H, W): the same tensor comes back
    with torch.no_grad():
        assert model.interpolated_pos_embed(H_IMG, W_IMG) is got


@pytest.mark.parametrize("args, what", [
    (dict(T=0), "T = 0"), (dict(H=0), "H = 0"), (dict(null="qkv"), "null qkv"), (dict(null="o"), "null o"),
    (dict(precision=2), "precision = 2")])
def test_vit_attn_fwd_rejects_bad_arguments_without_a_device(args, what):
    """Validation runs before any HIP call: -1 and the function's name in usc_last_error(), GPU or not."""
    import ctypes

    from unscene3d_amd import _lib

    assert _lib.lib.usc_vit_attn_head_dim() == 64
    buf = (ctypes.c_float * 1024)()                   # a host address: never dereferenced, the call fails before a launch
    addr = (ctypes.addressof(buf) + 15) & ~15
    qkv = None if args.get("null") == "qkv" else addr
    o = None if args.get("null") == "o" else addr
    rc = _lib.lib.usc_vit_attn_fwd(qkv, 1, args.get("T", 1), args.get("H", 1), 0.125, args.get("precision", 0), o, None)
    assert rc == -1, what
    assert "usc_vit_attn_fwd" in _lib.last_error()
