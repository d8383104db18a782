"""GPU: the decoder's host side (unscene3d_amd/ops.py projections, models/mask3d.py layers) returns the bits it returned
before the attention input projections became one self form and one cross form with one parameter-gradient rule.

tests/golden/decoder_bits.json holds sha256 digests over shape, dtype and bytes of every output and every gradient of
the calls below, recorded twice on the parent commit (both recordings agreed).  No tolerance: the change moved host code
only; the paths the model runs launch the same kernels on the same operands in the same order.  If a digest differs, the
code is wrong, not the file.

Every case goes through entry points that exist on both sides of the change: ops.in_proj, ops.in_proj_q, ops.in_proj_kv,
ops.self_attention, the three layer classes and _DecoderPass.  E = 128, 8 heads, ff = 256, seeded inputs.  "inplace": the
parameters carry non-zero gradient buffers and the kernels add into them (the trainer's mode); "autograd": no buffers,
the gradients come back through autograd.

A  self/...      the model's self-attention projections: one launch each way (usc_linear_fwd_split, usc_qkv_proj_bwd);
                 129 rows: two row tiles of the projection kernels and the second query group of the attention kernels
B  chain/...     the same projections with output gradients that are NOT adjacent in memory: the chained backward
C  cross/...     ops.in_proj with a separate memory: few-row (300) and many-row (1 500) keys
D  pass/...      _DecoderPass on prepared keys, post-norm and pre-norm
E  layer/...     CrossAttentionLayer.forward with the decoder's bool[B, S, L] mask
F  step/...      one training step, eager (both gradient modes) and with captured decoder passes"""
import hashlib
import itertools
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "decoder_bits.json")
E, H, FF = 128, 8, 256
MODES = ("inplace", "autograd")

SELF = [(L, B, pos, mode) for (L, B), pos, mode in itertools.product(((100, 2), (37, 1), (129, 1)), (True, False), MODES)]
CHAIN = [(res, pos, mode) for res, pos, mode in itertools.product((True, False), (True, False), MODES)]
CROSS = [300, 1500]
NORMS = ("post", "pre")
STEPS = ("eager", "graphed")


def _self_name(L, B, pos, mode):
    return f"self/L{L}-B{B}-{'pos' if pos else 'nopos'}-{mode}"


def _chain_name(res, pos, mode):
    return f"chain/{'res' if res else 'nores'}-{'pos' if pos else 'nopos'}-{mode}"


def case_names():
    """Every key the functions below compute (host side: no device needed)."""
    names = [_self_name(*c) for c in SELF] + [_chain_name(*c) for c in CHAIN] + [f"cross/S{S}" for S in CROSS]
    names += [f"pass/{n}" for n in NORMS] + [f"layer/{n}" for n in NORMS]
    keys = {f"{n}/{part}" for n in names for part in ("out", "grads")}
    return keys | {"step/eager-autograd", "step/eager-inplace", "step/graphed"}


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().cpu().contiguous()
        h.update(str(tuple(t.shape)).encode())
        h.update(str(t.dtype).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class _Draw:
    """Seeded host draws moved to the device: the same values whatever ran before."""

    def __init__(self, seed, device):
        self.g, self.device = torch.Generator().manual_seed(seed), device

    def __call__(self, *shape, scale=1.0):
        return (scale * torch.randn(shape, generator=self.g)).to(self.device)

    def leaf(self, *shape):
        return self(*shape).requires_grad_()

    def packed(self, mode):
        """in_proj_weight [3E, E], in_proj_bias [3E]; the gradient buffers are drawn in both modes (same inputs after)."""
        W, b = torch.nn.Parameter(self(3 * E, E, scale=1.0 / math.sqrt(E))), torch.nn.Parameter(self(3 * E, scale=0.1))
        gW, gb = self(3 * E, E), self(3 * E)
        if mode == "inplace":
            W.grad, b.grad = gW, gb
        return W, b


def self_bits(device, L, B, pos, mode):
    from unscene3d_amd import ops
    d = _Draw(7000 + 10 * L + B, device)
    W, b = d.packed(mode)
    x, p = d.leaf(L, B, E), d.leaf(L, B, E)
    go, gr = d(L, B, E), d(L, B, E)
    p = p if pos else None
    q, k, v, res = ops.in_proj(x, x, x, W, b, pos_q=p, pos_k=p, residual=True)
    o = ops.self_attention(q, k, v, H)
    ((o * go).sum() + (res * gr).sum()).backward()
    torch.cuda.synchronize()
    name = _self_name(L, B, pos, mode)
    return {f"{name}/out": _sha(q, k, v, o), f"{name}/grads": _sha(x.grad, None if p is None else p.grad, W.grad, b.grad)}


def chain_bits(device, res, pos, mode):
    from unscene3d_amd import ops
    L, B = 100, 2
    d = _Draw(7100, device)
    W, b = d.packed(mode)
    x, p = d.leaf(L, B, E), d.leaf(L, B, E)
    # the three output gradients lie two tables apart in one buffer: never the adjacent dq | dk | dv of the attention core
    spaced, gr = d(3, 2, L, B, E), d(L, B, E)
    p = p if pos else None
    outs = ops.in_proj(x, x, x, W, b, pos_q=p, pos_k=p, residual=res)
    torch.autograd.backward(list(outs), [spaced[0, 0], spaced[1, 0], spaced[2, 0]] + ([gr] if res else []))
    torch.cuda.synchronize()
    name = _chain_name(res, pos, mode)
    return {f"{name}/out": _sha(*outs[:3]), f"{name}/grads": _sha(x.grad, None if p is None else p.grad, W.grad, b.grad)}


def cross_bits(device, S):
    from unscene3d_amd import ops
    L, B = 100, 2
    d = _Draw(7200 + S, device)
    W, b = d.packed("inplace")
    xq, pq, mem, pk = d.leaf(L, B, E), d.leaf(L, B, E), d.leaf(S, B, E), d.leaf(S, B, E)
    dq, dk, dv, dres = d(L, B, E), d(S, B, E), d(S, B, E), d(L, B, E)
    q, k, v, res = ops.in_proj(xq, mem, mem, W, b, pos_q=pq, pos_k=pk, residual=True)
    torch.autograd.backward([q, k, v, res], [dq, dk, dv, dres])
    torch.cuda.synchronize()
    return {f"cross/S{S}/out": _sha(q, k, v),
            f"cross/S{S}/grads": _sha(xq.grad, pq.grad, mem.grad, pk.grad, W.grad, b.grad)}


def _decoder_pass(device, norm, seed):
    """One (cross, self, ffn) pass with every parameter away from its initial value and a non-zero gradient buffer."""
    from unscene3d_amd.models.mask3d import CrossAttentionLayer, FFNLayer, SelfAttentionLayer, _DecoderPass
    torch.manual_seed(seed)
    pre = norm == "pre"
    layer = _DecoderPass(CrossAttentionLayer(E, H, normalize_before=pre), SelfAttentionLayer(E, H, normalize_before=pre),
                         FFNLayer(E, FF, normalize_before=pre), H)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for _, p in sorted(layer.named_parameters()):
            if p.dim() == 1:                    # biases start at zero and norm weights at one
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    layer = layer.to(device).train()
    for _, p in sorted(layer.named_parameters()):
        p.grad = torch.randn(p.shape, generator=g).to(device)
    return layer


def _key_mask(d, B, K, Q):
    """bool[B, K, Q], True = masked; query 3 is masked at every key and then cleared, as the model's key sampling does."""
    m = torch.rand((B, K, Q), generator=d.g) < 0.5
    m[:, :, 3] = True
    m.permute(0, 2, 1)[m.sum(1) == K] = False
    assert not m[:, :, 3].any() and m.any()
    return m.to(d.device)


def pass_bits(device, norm):
    from unscene3d_amd import ops
    L, K, B = 100, 200, 2
    layer = _decoder_pass(device, norm, 7300)
    d = _Draw(7301, device)
    queries, query_pos, src, pos_k = d.leaf(B, L, E), d.leaf(L, B, E), d.leaf(K, B, E), d(K, B, E)
    go, mask = d(B, L, E), _key_mask(d, B, K, L)
    mha = layer.cross.multihead_attn
    k, v = ops.in_proj_kv(src, mha.in_proj_weight, mha.in_proj_bias, pos=pos_k)
    out = layer(queries, query_pos, k, v, mask)
    out.backward(go)
    torch.cuda.synchronize()
    grads = [queries.grad, query_pos.grad, src.grad] + [p.grad for _, p in sorted(layer.named_parameters())]
    return {f"pass/{norm}/out": _sha(k, v, out), f"pass/{norm}/grads": _sha(*grads)}


def layer_bits(device, norm):
    L, K, B = 100, 200, 2
    cross = _decoder_pass(device, norm, 7400).cross
    d = _Draw(7401, device)
    tgt, query_pos, mem, pos_k = d.leaf(L, B, E), d.leaf(L, B, E), d.leaf(K, B, E), d(K, B, E)
    go, mask = d(L, B, E), _key_mask(d, B, K, L)
    out = cross(tgt, mem, memory_mask_bsl=mask, pos=pos_k, query_pos=query_pos)
    out.backward(go)
    torch.cuda.synchronize()
    grads = [tgt.grad, query_pos.grad, mem.grad] + [p.grad for _, p in sorted(cross.named_parameters())]
    return {f"layer/{norm}/out": _sha(out), f"layer/{norm}/grads": _sha(*grads)}


class _PermSource:
    """k-th call -> torch.randperm(n) from a generator seeded with k (the key sampling's index stream)."""

    def __init__(self):
        self.k = 0

    def __call__(self, n, device=None):
        p = torch.randperm(n, generator=torch.Generator().manual_seed(1000 + self.k))
        self.k += 1
        return p.to(device) if device is not None else p


def step_bits(device, how):
    """The first configuration of tests/test_gpu_parity.py::test_decoder_graph_capture_equals_eager: 12 000 voxels, one
    scene, sample sizes [20, 50, 100, 200, 800].  Digest of the loss and of the concatenated non-backbone gradients.
    eager: one step without gradient buffers, then one with non-zero buffers on every parameter."""
    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.synthetic import SyntheticFreeMaskDataset
    from unscene3d_amd.datasets.utils import FreeMaskVoxelizeCollate
    from unscene3d_amd.trainer.trainer import InstanceSegmentation

    cfg = apply_overrides(default_config(), ["general.num_targets=3", "model.sample_sizes=[20,50,100,200,800]",
                                             "model.use_level_embed=False"])
    batch = [SyntheticFreeMaskDataset(n_scenes=1, target_voxels=12000, seed=3300)[0]]
    collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=0.02, mode="train", device=str(device))
    torch.manual_seed(3)
    module = InstanceSegmentation(cfg).to(device).train()
    if how == "graphed":
        module.model.enable_decoder_graphs(batch_size=1, device=device)

    def step():
        module.model.randperm = _PermSource()
        total, _ = module.training_step(collate(batch))
        total.backward()
        torch.cuda.synchronize()
        return _sha(total, torch.cat([p.grad.reshape(-1) for n, p in module.named_parameters()
                                      if p.grad is not None and "backbone" not in n]))

    if how == "graphed":
        return {"step/graphed": step()}
    bits = {"step/eager-autograd": step()}
    g = torch.Generator().manual_seed(7500)
    for _, p in module.named_parameters():
        p.grad = torch.randn(p.shape, generator=g).to(device)
    bits["step/eager-inplace"] = step()
    return bits


def decoder_bits(device, steps=True):
    bits = {}
    for c in SELF:
        bits.update(self_bits(device, *c))
    for c in CHAIN:
        bits.update(chain_bits(device, *c))
    for S in CROSS:
        bits.update(cross_bits(device, S))
    for n in NORMS:
        bits.update(pass_bits(device, n))
        bits.update(layer_bits(device, n))
    for how in STEPS if steps else ():
        bits.update(step_bits(device, how))
    return bits


def _expect(bits):
    want = json.load(open(GOLDEN))
    assert bits and set(bits) <= set(want), sorted(set(bits) - set(want))
    differ = sorted(k for k in bits if bits[k] != want[k])
    assert not differ, differ


@pytest.mark.gpu
@pytest.mark.parametrize("L,B,pos,mode", SELF)
def test_fused_self_projections_compute_the_recorded_bits(device, L, B, pos, mode):
    _expect(self_bits(device, L, B, pos, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("res,pos,mode", CHAIN)
def test_chained_self_projections_compute_the_recorded_bits(device, res, pos, mode):
    _expect(chain_bits(device, res, pos, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("S", CROSS)
def test_cross_projections_compute_the_recorded_bits(device, S):
    _expect(cross_bits(device, S))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_decoder_pass_computes_the_recorded_bits(device, norm):
    _expect(pass_bits(device, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_cross_attention_layer_computes_the_recorded_bits(device, norm):
    _expect(layer_bits(device, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("how", STEPS)
def test_training_step_computes_the_recorded_bits(device, how):
    _expect(step_bits(device, how))


def test_every_recorded_case_is_still_computed():
    """Host side of the pin: the golden file's names are the cases above and nothing else (a case cannot drop out of the
    comparison by being renamed)."""
    want = json.load(open(GOLDEN))
    assert all(len(v) == 64 for v in want.values())
    assert set(want) == case_names()
    assert len(want) == 2 * (12 + 8 + 2 + 2 + 2) + 3
