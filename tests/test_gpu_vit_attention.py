"""Fused ViT attention kernel (csrc/vit_attention.hip, usc_vit_attn_fwd) and the DINO encoder on the device.

Kernel: the oracle is float64 attention on the CPU, one head at a time (tests/vit_ref.py::attention_f64).
  f32:  elementwise error <= 2 x the largest error torch's own f32 `softmax(q k^T * scale) v` makes against float64 on
        the same input and device (the arithmetic the reference runs; the 2 covers another summation order).
  bf16: the oracle is float64 attention of the bf16-ROUNDED q, k, v (tests/bf16_ref.py).  What remains is P rounded to
        bf16 (relative 2^-9 per term, in numerator and denominator) plus f32 accumulation:
        |o - oracle|[i, d] <= 2^-7 * sum_j p_ij |v_jd| + the f32 allowance above (derived, margin 2, not tuned).
  o sits between 64 guard rows of a sentinel on both sides, which must stay bit-unchanged; two calls give the same bits.

Encoder (40 x 56 image, 118 tokens) against tests/vit_ref.py in float64.  The reference's own extractor cannot be
imported here (`timm` and `torchvision` are not installed)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vit_ref as R
from bf16_ref import bf16_round

pytestmark = pytest.mark.gpu

D, SCALE, GUARD, SENTINEL = 64, 0.125, 64, -12345.5
SHAPES = [(1, 1, 1), (1, 17, 6), (2, 64, 6), (1, 65, 6), (1, 129, 2), (2, 197, 6), (1, 333, 6), (1, 2962, 6)]


def _inputs(B, T, H):
    """Gaussian q, k, v as one f32 [B, T, 3, H, 64] array.  T = 333: a ramp along one direction u is added to k and q
    is pushed along u, so every key tile raises every query's running max (each rescale branch runs).  T = 197: q is
    scaled until the logits reach +-80."""
    rng = np.random.default_rng(1000 * T + 10 * H + B)
    qkv = rng.standard_normal((B, T, 3, H, D)).astype(np.float32)
    if T == 333:
        u = rng.standard_normal(D)
        u /= np.linalg.norm(u)
        qkv[:, :, 0] += (3.0 * u).astype(np.float32)
        qkv[:, :, 1] += (0.5 * np.arange(T)[None, :, None, None] * u).astype(np.float32)
    if T == 197:
        logits = np.einsum("bthd,bshd->bhts", qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64)) * SCALE
        qkv[:, :, 0] *= np.float32(80.0 / np.abs(logits).max())
    return qkv


def _oracle(qkv):
    """-> o f64 [B, T, H*64], sum_j p |v| in the same layout"""
    B, T, _, H, _ = qkv.shape
    o, pv = np.zeros((B, T, H * D)), np.zeros((B, T, H * D))
    for b in range(B):
        for h in range(H):
            o[b, :, h * D:(h + 1) * D], pv[b, :, h * D:(h + 1) * D] = R.attention_f64(qkv[b, :, 0, h], qkv[b, :, 1, h],
                                                                                    qkv[b, :, 2, h], SCALE)
    return o, pv


def _torch_f32(qkv_dev):
    B, T, _, H, _ = qkv_dev.shape
    q, k, v = qkv_dev.permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-1, -2)) * SCALE, -1) @ v
    return a.transpose(1, 2).reshape(B, T, H * D).cpu().numpy().astype(np.float64)


def _kernel(qkv_dev, precision):
    """-> (o as numpy f32 [B, T, H*64], the guard rows untouched?) through the C entry point, o between guard rows"""
    from unscene3d_amd import _lib

    B, T, _, H, _ = qkv_dev.shape
    buf = torch.full((B * T + 2 * GUARD, H * D), SENTINEL, dtype=torch.float32, device=qkv_dev.device)
    o = buf[GUARD:GUARD + B * T]
    rc = _lib.lib.usc_vit_attn_fwd(qkv_dev.data_ptr(), B, T, H, SCALE, precision, o.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guards_ok = bool((host[:GUARD] == np.float32(SENTINEL)).all() and (host[GUARD + B * T:] == np.float32(SENTINEL)).all())
    return host[GUARD:GUARD + B * T].reshape(B, T, H * D).copy(), guards_ok


@functools.lru_cache(maxsize=None)
def _run(shape):
    """Everything the kernel tests of one shape look at, computed once."""
    dev = torch.device("cuda:0")
    qkv = _inputs(*shape)
    qkv_dev = torch.from_numpy(qkv).to(dev)
    out = {"ref": _oracle(qkv)}
    out["torch_err"] = float(np.abs(_torch_f32(qkv_dev) - out["ref"][0]).max())
    out["f32"] = [_kernel(qkv_dev, 0) for _ in range(2)]
    rounded = bf16_round(qkv)
    out["ref16"] = _oracle(rounded)
    out["torch_err16"] = float(np.abs(_torch_f32(torch.from_numpy(rounded).to(dev)) - out["ref16"][0]).max())
    out["bf16"] = [_kernel(qkv_dev, 1) for _ in range(2)]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-T%d-H%d" % s)
def test_f32_kernel_within_twice_torchs_own_error(device, shape):
    r = _run(shape)
    o, _ = r["f32"][0]
    assert np.isfinite(o).all()
    err = float(np.abs(o.astype(np.float64) - r["ref"][0]).max())
    print(f"vit_attn f32 {shape}: max err {err:.3e}, torch f32 {r['torch_err']:.3e}, ratio {err / max(r['torch_err'], 1e-300):.2f}")
    assert err <= 2 * r["torch_err"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-T%d-H%d" % s)
def test_bf16_kernel_within_the_derived_bound(device, shape):
    r = _run(shape)
    o, _ = r["bf16"][0]
    assert np.isfinite(o).all()
    ref, pv = r["ref16"]
    err = np.abs(o.astype(np.float64) - ref)
    bound = 2.0 ** -7 * pv + 2 * r["torch_err16"]
    print(f"vit_attn bf16 {shape}: max err {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-T%d-H%d" % s)
def test_guard_rows_untouched_and_two_calls_bit_identical(device, shape):
    r = _run(shape)
    for prec in ("f32", "bf16"):
        (a, ga), (b, gb) = r[prec]
        assert ga and gb, f"{prec}: rows outside o[0 : B*T] were written"
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{prec}: two calls differ"


def test_ops_vit_attention_is_the_entry_point(device):
    from unscene3d_amd import ops

    shape = (2, 64, 6)
    qkv_dev = torch.from_numpy(_inputs(*shape)).to(device)
    for prec in ("f32", "bf16"):
        o = ops.vit_attention(qkv_dev, *shape, SCALE, precision=prec)
        assert o.shape == (2, 64, 6 * D)
        assert np.array_equal(o.cpu().numpy(), _run(shape)[prec][0][0])
    with pytest.raises(RuntimeError):
        ops.vit_attention(qkv_dev, *shape, SCALE, precision="f16")
    with pytest.raises(RuntimeError):
        ops.vit_attention(qkv_dev, 2, 65, 6, SCALE)


# ------------------------------------------------------------------ whole encoder, 40 x 56
H_IMG, W_IMG, N_FRAMES, LAYER = 40, 56, 2, 10
BF16_ENCODER_BOUND = 2e-2      # relative L2 against the f64 oracle; see test_encoder_bf16


def _config(feature="descriptors"):
    return SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_stride=4,
                                                      dino_vit_layer=LAYER, dino_vit_feature=feature))


@functools.lru_cache(maxsize=None)
def _encoder_case(seed):
    sd = R.random_state_dict(seed)
    images = torch.randn((1, N_FRAMES, 3, H_IMG, W_IMG), generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float64)
    want64, _ = R.dinonet(sd, images, "descriptors", LAYER)
    want32, _ = R.dinonet(sd, images, "descriptors", LAYER, dtype=torch.float32)
    return sd, images, want64, R.rel_l2(want32, want64)


def _net(seed, precision="f32"):
    from unscene3d_amd.models.encoders_2d import DinoNet

    net = DinoNet(_config(), dataset=None, precision=precision)
    net.vit.load_state_dict({k: v.float() for k, v in _encoder_case(seed)[0].items()}, strict=True)
    return net.to("cuda:0").eval()


@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "USC3D_VIT_ATTN=0"])
def test_encoder_f32_within_four_times_the_f32_oracle(device, monkeypatch, kernel):
    from unscene3d_amd.models.encoders_2d import dino

    monkeypatch.setattr(dino, "VIT_ATTN", kernel)
    _, images, want64, base = _encoder_case(0)
    got, none = _net(0)(images.float().to(device))
    assert none is None and got.shape == (1, N_FRAMES, H_IMG, W_IMG, 384) and got.dtype == torch.float32
    err = R.rel_l2(got.cpu(), want64)
    print(f"encoder f32 ({'kernel' if kernel else 'plain operators'}): rel L2 {err:.3e}, f32 oracle {base:.3e}")
    assert err <= 4 * base


def test_encoder_runs_the_kernel_on_the_device(device, monkeypatch):
    """The f32 device path goes through ops.vit_attention once per block below the layer asked for."""
    from unscene3d_amd import ops

    calls = []
    real = ops.vit_attention
    monkeypatch.setattr(ops, "vit_attention", lambda *a, **k: (calls.append(a[1:4]), real(*a, **k))[1])
    _net(0)(_encoder_case(0)[1].float().to(device))
    assert calls == [(N_FRAMES, 118, 6)] * LAYER


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_encoder_bf16(device, seed):
    """bf16 encoder (bf16 attention kernel, bf16 linears, f32 residual stream) against the f64 oracle.  Measured relative
    L2 on an MI355X: 5.39e-3, 5.78e-3, 5.66e-3 for seeds 0, 1, 2 (ten blocks of bf16 operands at 2^-9 each).
    BF16_ENCODER_BOUND is twice the worst measured value, rounded up to one digit — the treatment test_gpu_bf16_conv.py
    gives the bf16 trunk; the attention kernel's own bf16 bound above is derived, not measured."""
    _, images, want64, base = _encoder_case(seed)
    got, _ = _net(seed, "bf16")(images.float().to(device))
    assert bool(torch.isfinite(got).all())
    err = R.rel_l2(got.cpu(), want64)
    print(f"encoder bf16 seed {seed}: rel L2 {err:.3e} (f32 oracle {base:.3e})")
    assert err <= BF16_ENCODER_BOUND


def test_encode_scene_feats_2d_takes_a_dinonet(device):
    """encode_scene_feats_2d(DinoNet, ...) on a tiny synthetic scene (poses, intrinsics and projecter as
    test_pseudo_mask_pipeline.py::test_encode_scene_feats_2d_running_mean_over_frames; 40 x 56 images, two frames)
    against the same call fed with a stub that returns the f64 oracle's features cast to f32.  A voxel's value is the
    mean of at most two frames' pixel means, so the encoder's relative L2 bound (4 x the f32 oracle's) carries over."""
    from unscene3d_amd import project_features_cuda as P
    from unscene3d_amd.pseudo_masks.pipeline import encode_scene_feats_2d
    from unscene3d_amd.synthetic import camera_views as cameras, room_voxels as room

    _, images, want64, base = _encoder_case(0)
    W, H = W_IMG, H_IMG
    coords = room(21, batch=1)
    raw_views = cameras(9, coords, N_FRAMES)
    intr = np.array([[W * 0.9, W * 0.9, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.4]], np.float32)
    proj = P.Project2DFeaturesCUDA(width=W, height=H, voxel_size=0.02, depth_min=0.1, depth_max=0.9)
    args = (torch.from_numpy(raw_views).to(device), torch.from_numpy(intr).to(device), torch.from_numpy(coords).to(device), proj)
    imgs = images.float().to(device)
    got = encode_scene_feats_2d(_net(0), imgs, *args, attention=False)

    frames = {float(imgs[0, i].flatten()[0]): i for i in range(N_FRAMES)}      # the stub tells the frames apart by a pixel

    def stub(img):
        return want64[:, frames[float(img.flatten()[0])]].unsqueeze(1).float().to(device), None

    want = encode_scene_feats_2d(stub, imgs, *args, attention=False)
    assert got.shape == want.shape == (coords.shape[0], 384)
    assert float(want.abs().sum()) > 0 and int((want.abs().sum(1) > 0).sum()) > 100      # the scene is seen
    err = R.rel_l2(got.cpu(), want.cpu())
    print(f"encode_scene_feats_2d: rel L2 {err:.3e}, bound {4 * base:.3e}")
    assert err <= 4 * base
