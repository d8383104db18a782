"""DINO ViT-S/8 image encoder of the pseudo-mask generator (reference models/encoders_2d/dino.py over
third_party/dino_vit/extractor.py; configuration pseudo_masks/config/default.yaml: `dino_vits8`, stride 4, layer 10,
'descriptors').

`DinoViT` has the state_dict of DINO's VisionTransformer (ViT-S, patch 8: 150 tensors), so the published checkpoint
loads with `load_state_dict(torch.load(path), strict=True)`; the network's weights are not part of this repository.
`DinoNet` has the reference wrapper's interface and column orders.

On the device, without gradients, the attention core of every block is one fused HIP kernel (`ops.vit_attention`,
csrc/vit_attention.hip): the [heads, tokens, tokens] score tensor is never written.  `USC3D_VIT_ATTN=0` runs the plain
operators (`softmax(q k^T * scale) v`) instead — the A/B reference.  With gradients enabled, or on CPU tensors, the
module is plain torch operators in the tensor's dtype.  Everything around the attention core (linears, GELU, LayerNorm,
patch embedding, interpolations) is torch.

precision="bf16" (device, no gradients): the attention kernel rounds q, k, v and the probabilities to bf16, and the four
linears of every block run as bf16 matmuls (input and weight rounded to bf16, the product returned to f32, the bias
added in f32).  The residual stream, LayerNorm and GELU stay f32."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

VIT_ATTN = os.environ.get("USC3D_VIT_ATTN", "1") != "0"     # 0: plain-operator attention (A/B reference)

EMBED_DIM, DEPTH, NUM_HEADS, MLP_DIM, PATCH, TRAIN_GRID = 384, 12, 6, 1536, 8, 28


class _PatchEmbed(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Conv2d(3, EMBED_DIM, kernel_size=PATCH, stride=PATCH)   # the stride in use is DinoViT.stride


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.qkv = nn.Linear(EMBED_DIM, 3 * EMBED_DIM)
        self.proj = nn.Linear(EMBED_DIM, EMBED_DIM)


class _Mlp(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = nn.Linear(EMBED_DIM, MLP_DIM)
        self.fc2 = nn.Linear(MLP_DIM, EMBED_DIM)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1 = nn.LayerNorm(EMBED_DIM, eps=1e-6)
        self.attn = _Attention()
        self.norm2 = nn.LayerNorm(EMBED_DIM, eps=1e-6)
        self.mlp = _Mlp()


def plain_attention(qkv: torch.Tensor, B: int, T: int, H: int, scale: float) -> torch.Tensor:
    """qkv [B, T, 3*H*d] -> [B, T, H*d] with torch's bmm, softmax, bmm: the ViT's own Attention.forward."""
    q, k, v = qkv.reshape(B, T, 3, H, -1).permute(2, 0, 3, 1, 4)
    attn = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, T, -1)


class DinoViT(nn.Module):
    """ViT-S/8 as DINO builds it (pre-norm blocks, LayerNorm eps 1e-6, exact GELU, no dropout), run the way the
    reference's extractor runs it: patch embedding at `stride`, position embedding interpolated to the patch grid."""

    def __init__(self, stride: int = 4, precision: str = "f32"):
        super().__init__()
        if PATCH % stride != 0:
            raise ValueError(f"stride {stride} must divide the patch size {PATCH}")
        if precision not in ("f32", "bf16"):
            raise ValueError(f"precision must be 'f32' or 'bf16', got {precision!r}")
        self.stride, self.precision = int(stride), precision
        self.cls_token = nn.Parameter(torch.zeros(1, 1, EMBED_DIM))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + TRAIN_GRID * TRAIN_GRID, EMBED_DIM))
        self.patch_embed = _PatchEmbed()
        self.blocks = nn.ModuleList([_Block() for _ in range(DEPTH)])
        self.norm = nn.LayerNorm(EMBED_DIM, eps=1e-6)
        self.scale = (EMBED_DIM // NUM_HEADS) ** -0.5
        self._pos_cache = {}     # (H, W) -> (tag of pos_embed, interpolated embedding)
        self._w16 = {}           # id(weight) -> (tag of weight, bf16 copy)

    # ---- pieces
    def grid(self, H: int, W: int):
        return 1 + (H - PATCH) // self.stride, 1 + (W - PATCH) // self.stride

    def interpolated_pos_embed(self, H: int, W: int) -> torch.Tensor:
        """[1, 1 + gh*gw, 384]: the 28x28 patch position embedding resampled bicubically to the patch grid of an HxW image
        by SCALE FACTOR (n + 0.1) / 28 per axis (extractor.py:92-116; the factor, not the size ratio, maps the coordinates),
        class position in front."""
        pe = self.pos_embed
        tag = (pe.data_ptr(), pe._version, pe.dtype, pe.device)
        hit = self._pos_cache.get((H, W))
        if hit is not None and hit[0] == tag and not (torch.is_grad_enabled() and pe.requires_grad):
            return hit[1]
        gh, gw = self.grid(H, W)
        if (gh, gw) == (TRAIN_GRID, TRAIN_GRID):
            out = pe
        else:
            grid = pe[:, 1:].reshape(1, TRAIN_GRID, TRAIN_GRID, EMBED_DIM).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, scale_factor=((gh + 0.1) / TRAIN_GRID, (gw + 0.1) / TRAIN_GRID), mode="bicubic",
                                 align_corners=False, recompute_scale_factor=False)
            if tuple(grid.shape[-2:]) != (gh, gw):
                raise RuntimeError(f"position embedding resampled to {tuple(grid.shape[-2:])}, expected {(gh, gw)}")
            out = torch.cat((pe[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, EMBED_DIM)), dim=1)
        if not (torch.is_grad_enabled() and pe.requires_grad):
            out = out.detach()
            self._pos_cache[(H, W)] = (tag, out)
        return out

    def _fast(self, x: torch.Tensor) -> bool:
        """The device inference path: f32 HIP tensor, no autograd graph."""
        return x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()

    def _linear(self, x: torch.Tensor, lin: nn.Linear) -> torch.Tensor:
        if not (self.precision == "bf16" and self._fast(x)):
            if not x.is_cuda and x.dim() == 3 and x.shape[0] > 1:
                # one GEMM per frame: a CPU BLAS picks its blocking by the row count, and a frame's result must not
                # depend on the frames it shares a call with
                return torch.stack([F.linear(f, lin.weight, lin.bias) for f in x])
            return F.linear(x, lin.weight, lin.bias)
        w = lin.weight
        tag = (w.data_ptr(), w._version)
        hit = self._w16.get(id(w))
        if hit is None or hit[0] != tag:
            hit = (tag, w.detach().to(torch.bfloat16))
            self._w16[id(w)] = hit
        return F.linear(x.to(torch.bfloat16), hit[1]).float() + lin.bias

    def _attention(self, qkv: torch.Tensor) -> torch.Tensor:
        B, T, _ = qkv.shape
        if VIT_ATTN and self._fast(qkv):
            from ... import ops
            return ops.vit_attention(qkv.contiguous(), B, T, NUM_HEADS, self.scale, self.precision)
        return plain_attention(qkv, B, T, NUM_HEADS, self.scale)

    def embed(self, images: torch.Tensor) -> torch.Tensor:
        """images [B, 3, H, W] -> tokens [B, 1 + gh*gw, 384] (class token first, position embedding added)."""
        B, _, H, W = images.shape
        w = self.patch_embed.proj.weight
        cols = F.unfold(images, kernel_size=PATCH, stride=self.stride)              # [B, 3*8*8, gh*gw]
        x = cols.transpose(1, 2) @ w.reshape(EMBED_DIM, -1).t() + self.patch_embed.proj.bias
        x = torch.cat((self.cls_token.expand(B, -1, -1), x), dim=1)
        return x + self.interpolated_pos_embed(H, W)

    def _block(self, blk: _Block, x: torch.Tensor) -> torch.Tensor:
        qkv = self._linear(F.layer_norm(x, (EMBED_DIM,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps), blk.attn.qkv)
        x = x + self._linear(self._attention(qkv), blk.attn.proj)
        h = self._linear(F.layer_norm(x, (EMBED_DIM,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps), blk.mlp.fc1)
        return x + self._linear(F.gelu(h), blk.mlp.fc2)

    # ---- entry points
    def qkv_at(self, images: torch.Tensor, layer: int) -> torch.Tensor:
        """The qkv projection of block `layer`, [B, T, 3, heads, 64]: blocks 0..layer-1, then norm1 and qkv of block
        `layer`.  (The reference runs all twelve blocks and keeps this tensor from a hook; the rest does not feed it.)"""
        if not 0 <= layer < DEPTH:
            raise ValueError(f"layer must be in [0, {DEPTH}), got {layer}")
        x = self.embed(images)
        for blk in self.blocks[:layer]:
            x = self._block(blk, x)
        blk = self.blocks[layer]
        qkv = self._linear(F.layer_norm(x, (EMBED_DIM,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps), blk.attn.qkv)
        return qkv.reshape(qkv.shape[0], qkv.shape[1], 3, NUM_HEADS, EMBED_DIM // NUM_HEADS)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """The whole network: the normalised class token [B, 384], as DINO's VisionTransformer.forward."""
        x = self.embed(images)
        for blk in self.blocks:
            x = self._block(blk, x)
        return F.layer_norm(x, (EMBED_DIM,), self.norm.weight, self.norm.bias, self.norm.eps)[:, 0]


def init_random_weights(vit: DinoViT, seed: int) -> DinoViT:
    """Weights from a seed instead of the published checkpoint (smoke runs, benchmarks, tests: the features mean
    nothing): every tensor N(0, 0.02) from a CPU generator, LayerNorm weights one and biases zero."""
    gen = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        for p in vit.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
        for m in vit.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.fill_(1.0)
                m.bias.zero_()
    return vit


class DinoNet(nn.Module):
    """Interface of the reference's models/encoders_2d/dino.py: forward(images [1, n, 3, H, W]) ->
    (features, None) in 'descriptors' mode, (keys, queries) in 'attention' mode, each [1, n, H, W, 384] after the bilinear
    resize to the image.  The n frames go through the network as one batch.  No normalisation inside: the dataset has
    applied mean and std 0.5.

    Column orders are the reference's: descriptors = key of block `dino_vit_layer`, column d*6 + head
    (extractor.py:301); attention mode = key and query of the last block, column head*64 + d (dino.py:95-96)."""

    def __init__(self, config, dataset=None, precision: str = "f32", **kwargs):
        super().__init__()
        self.config = config
        self.dataset = dataset
        self.backbone = config.image_data.image_backbone
        if self.backbone != "dino_vits8":
            raise ValueError(f"image_backbone {self.backbone!r} is not covered: only 'dino_vits8'")
        self.image_shape = getattr(dataset, "depth_shape", None)
        self.vit_feature = config.image_data.dino_vit_feature
        self.layer = int(config.image_data.dino_vit_layer)
        self.facet = "key"
        self.bin = False
        self.vit = DinoViT(stride=int(config.image_data.dino_vit_stride), precision=precision)
        self.feature_dim = EMBED_DIM

    def _to_image(self, tokens: torch.Tensor, shape) -> torch.Tensor:
        """tokens [n, gh*gw, 384] -> [1, n, H, W, 384]"""
        n, H, W = shape[1], shape[3], shape[4]
        gh, gw = self.vit.grid(H, W)
        maps = tokens.reshape(n, gh, gw, -1).permute(0, 3, 1, 2).contiguous()
        maps = F.interpolate(maps, size=(H, W), mode="bilinear")
        return maps.permute(0, 2, 3, 1).contiguous().view(1, n, H, W, -1)

    def forward_descriptor(self, input_images):
        with torch.no_grad():
            qkv = self.vit.qkv_at(input_images.reshape(-1, *input_images.shape[2:]), self.layer)
            key = qkv[:, 1:, 1]                                                   # [n, tokens, head, d], class token dropped
            return self._to_image(key.permute(0, 1, 3, 2).flatten(-2), input_images.shape), None

    def forward_attention(self, input_images):
        with torch.no_grad():
            qkv = self.vit.qkv_at(input_images.reshape(-1, *input_images.shape[2:]), DEPTH - 1)
            key, query = qkv[:, 1:, 1].flatten(-2), qkv[:, 1:, 0].flatten(-2)
            return self._to_image(key, input_images.shape), self._to_image(query, input_images.shape)

    def forward_tokens(self, input_images):
        """images [1, n, 3, H, W] -> (key_tokens f32[n, gh, gw, 384], query_tokens or None): what `forward` resizes,
        before the resize, in the same column orders ('descriptors': key of block `dino_vit_layer`, column d*6 + head;
        'attention': key and query of the last block, column head*64 + d).  `Project2DFeaturesCUDA.fuse_frames_tokens`
        samples these grids at the hit pixels, so the [n, H, W, 384] maps are never written."""
        n, H, W = input_images.shape[1], input_images.shape[3], input_images.shape[4]
        gh, gw = self.vit.grid(H, W)
        grid = lambda t: t.reshape(n, gh, gw, -1).float().contiguous()
        with torch.no_grad():
            images = input_images.reshape(-1, *input_images.shape[2:])
            if self.vit_feature == "attention":
                qkv = self.vit.qkv_at(images, DEPTH - 1)
                return grid(qkv[:, 1:, 1].flatten(-2)), grid(qkv[:, 1:, 0].flatten(-2))
            qkv = self.vit.qkv_at(images, self.layer)
            return grid(qkv[:, 1:, 1].permute(0, 1, 3, 2).flatten(-2)), None

    def forward(self, input_images):
        if self.vit_feature == "attention":
            return self.forward_attention(input_images)
        return self.forward_descriptor(input_images)
