"""The fused decoder attention for 129 to 256 queries (csrc/attention.hip, the mask part of usc_sample_keys in
csrc/rows.hip) — the reference's export recipe runs a 100-query checkpoint at `model.num_queries=150`.

Cross attention and self attention against float64 on the CPU (forward and all input gradients, twice the same bits),
the mask rows of `sample_keys` against the steps of the decoder's plain-operator branch, the model at 150 queries
against the oracle's eval forward with a count of the fused calls, and a guard that the <= 128-query path computes the
bits it computed before the limit was raised (tests/golden/attention_bits.json, recorded on the library of the parent
commit)."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.json")
H, HD, E = 8, 16, 128


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _cross_inputs(L, S, B, wide_keys=False):
    g = torch.Generator().manual_seed(L + S)
    q, k, v = torch.randn(L, B, E, generator=g), torch.randn(S, B, E, generator=g), torch.randn(S, B, E, generator=g)
    mask = torch.rand(B, S, L, generator=g) > 0.5
    mask[:, 0, :] = False                                  # every query keeps at least one key
    mask[:, 5, :] = True                                   # a key nobody attends to
    if wide_keys:                                          # a kernel that reads the first group's mask words for the
        mask[:, 7, :128], mask[:, 7, 128:] = True, False   # second group gets keys 7 and 9 wrong
        mask[:, 9, :128], mask[:, 9, 128:] = False, True
    do = torch.randn(L, B, E, generator=g)
    return q, k, v, mask, do


def _cross_device(device, q, k, v, mask, do):
    from unscene3d_amd import ops
    qd, kd, vd = (t.to(device).requires_grad_() for t in (q, k, v))
    out = ops.masked_cross_attention(qd, kd, vd, mask.to(device), H)
    out.backward(do.to(device))
    return out.detach(), qd.grad, kd.grad, vd.grad


def _self_inputs(L, B):
    g = torch.Generator().manual_seed(L * 7 + B)
    return tuple(torch.randn(L, B, E, generator=g) for _ in range(4))


def _self_device(device, q, k, v, do):
    from unscene3d_amd import ops
    qd, kd, vd = (t.to(device).requires_grad_(True) for t in (q, k, v))
    o = ops.self_attention(qd, kd, vd, H)
    o.backward(do.to(device))
    return o.detach(), qd.grad, kd.grad, vd.grad


def _sample_inputs(q, K=37, n_valid=(37, 20), rows=(90, 60)):
    """Two scenes; in scene 0 the columns 3, 127, 128 and q - 1 (those that exist) are masked in every sampled row, in
    scene 1 column 128 (or q - 1 below 129 queries) is masked in all sampled rows but one."""
    g = torch.Generator().manual_seed(1000 + q)
    n = sum(rows)
    mask = torch.rand(n, q, generator=g) < 0.5
    idx, off = [], 0
    for b, (r, nv) in enumerate(zip(rows, n_valid)):
        real = torch.randperm(r, generator=g)[:nv] + off
        idx.append(torch.cat([real, real[:1].expand(K - nv)]))          # padding repeats a real row
        off += r
    for c in (3, 127, 128, q - 1):
        if c < q:
            mask[idx[0][:n_valid[0]], c] = True
    c1 = 128 if q > 128 else q - 1
    mask[idx[1][:n_valid[1]], c1] = True
    mask[idx[1][4], c1] = False
    return mask, torch.cat(idx), K, list(n_valid)


def _sample_reference(mask, gidx, K, n_valid):
    """The steps of the decoder's plain-operator branch (models/mask3d.py): gather, a query whose sampled keys are all
    masked attends to everything, padding keys are masked."""
    n_scenes = len(n_valid)
    ref = torch.stack([mask[gidx[b * K:(b + 1) * K], :] for b in range(n_scenes)])
    ref.permute(0, 2, 1)[ref.sum(1) == K] = False
    pad = torch.stack([torch.arange(K) >= nv for nv in n_valid])
    return torch.logical_or(ref, pad[..., None])


def _sample_device(device, mask, gidx, K, n_valid, outs=None):
    from unscene3d_amd import ops
    return ops.sample_keys(None, mask.to(device), None, gidx.to(device), len(n_valid), K, n_valid, outs=outs)


def narrow_bits(device):
    """sha256 of what the <= 128-query kernels compute on seeded inputs."""
    bits = {}
    for L, S, B in ((100, 3200, 1), (128, 200, 2)):
        bits[f"cross_{L}_{S}_{B}"] = _sha(*_cross_device(device, *_cross_inputs(L, S, B)))
    bits["self_100_2"] = _sha(*_self_device(device, *_self_inputs(100, 2)))
    bits["sample_100"] = _sha(_sample_device(device, *_sample_inputs(100)))
    return bits


def test_narrow_path_computes_the_recorded_bits(device):
    """L <= 128 launches what it launched before 129..256 queries were added: outputs and gradients of the cross
    attention at (100, 3200, 1) and (128, 200, 2), of the self attention at (100, 2) and a `sample_keys` mask result at
    100 queries hash to the values recorded with the library of the parent commit."""
    want = json.load(open(GOLDEN))
    assert narrow_bits(device) == want


@pytest.mark.parametrize("L,S,B", [(129, 200, 1), (150, 3200, 1), (150, 999, 2), (161, 77, 3), (256, 1000, 1)])
def test_cross_attention_wide(device, L, S, B):
    """usc_attn_fwd / _bwd at 129..256 queries against softmax(q k^T / 4 + mask) v in float64 on the CPU: output and dq,
    dk, dv within the project's 1e-5 (the same computation in float32 stays <= 3.5e-7 from float64 on these shapes), and
    a second call with the same bits.  One query in the second group; a tile boundary plus one; the full width; fewer
    keys than the split count allows and no multiple of 32; several batches.  Keys 7 and 9 are masked for one query
    group and open for the other."""
    q, k, v, mask, do = _cross_inputs(L, S, B, wide_keys=True)
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    qh = qr.reshape(L, B * H, HD).transpose(0, 1)
    kh = kr.reshape(S, B * H, HD).transpose(0, 1)
    vh = vr.reshape(S, B * H, HD).transpose(0, 1)
    bias = torch.zeros(B, H, L, S, dtype=torch.float64).masked_fill_(mask.permute(0, 2, 1)[:, None], float("-inf"))
    sc = qh @ kh.transpose(1, 2) / 4.0 + bias.reshape(B * H, L, S)
    ref = (torch.softmax(sc, -1) @ vh).transpose(0, 1).reshape(L, B, E)
    ref.backward(do.double())
    out, dq, dk, dv = _cross_device(device, q, k, v, mask, do)
    errs = [rel_err(out, ref.detach()), rel_err(dq, qr.grad), rel_err(dk, kr.grad), rel_err(dv, vr.grad)]
    print(f"cross attention L={L} S={S} B={B}: rel err o {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert all(e < 1e-5 for e in errs), errs
    for a, b in zip((out, dq, dk, dv), _cross_device(device, q, k, v, mask, do)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("L,B", [(129, 1), (150, 2), (160, 1), (255, 3), (256, 1)])
def test_self_attention_wide(device, L, B):
    """usc_self_attn_fwd / _bwd at 129..256 queries (up to 8 query tiles and 8 key chunks) against softmax(q k^T / 4) v in
    float64 on the CPU: output and all three input gradients; and twice the same bits."""
    q, k, v, do = _self_inputs(L, B)
    qr, kr, vr = (t.clone().double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.reshape(L, B * H, HD).transpose(0, 1) for t in (qr, kr, vr))
    o_ref = (torch.softmax(qh @ kh.transpose(1, 2) / 4.0, dim=-1) @ vh).transpose(0, 1).reshape(L, B, E)
    o_ref.backward(do.double())
    o, dq, dk, dv = _self_device(device, q, k, v, do)
    print(f"self attention L={L} B={B}: rel err o {rel_err(o, o_ref.detach()):.2e} dq {rel_err(dq, qr.grad):.2e} "
          f"dk {rel_err(dk, kr.grad):.2e} dv {rel_err(dv, vr.grad):.2e}")
    assert rel_err(o, o_ref.detach()) < 1e-5
    for got, exp in ((dq, qr.grad), (dk, kr.grad), (dv, vr.grad)):
        assert float((got.double().cpu() - exp).norm()) <= 1e-5 * float(exp.norm()) + 1e-6
    o2, dq2, dk2, dv2 = _self_device(device, q, k, v, do)
    assert torch.equal(o2, o) and torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)


@pytest.mark.parametrize("q", [129, 130, 150, 256])
def test_sample_keys_mask_rows_wide(device, q):
    """The mask part of usc_sample_keys at 129..256 query columns == gather, all-masked-column rule, padding mask of the
    decoder's plain-operator branch, exactly; columns 3, 127, 128 and q - 1 are masked in every sampled row of scene 0
    (cleared in its real rows), column 128 in all but one row of scene 1 (kept); and the call with `outs=`."""
    mask, gidx, K, n_valid = _sample_inputs(q)
    ref = _sample_reference(mask, gidx, K, n_valid)
    got = _sample_device(device, mask, gidx, K, n_valid)
    assert got.dtype == torch.bool and tuple(got.shape) == (2, K, q)
    assert torch.equal(got.cpu(), ref)
    for c in (3, 127, 128, q - 1):
        assert not ref[0, :n_valid[0], c].any()                   # the rule fired (n_valid[0] = K: no padding rows)
    assert int(ref[1, :n_valid[1], 128].sum()) == n_valid[1] - 1 and ref[1, n_valid[1]:, 128].all()
    buf = torch.empty(2, K, q, dtype=torch.bool, device=device)
    got2 = _sample_device(device, mask, gidx, K, n_valid, outs=(None, buf, None))
    assert got2.data_ptr() == buf.data_ptr() and torch.equal(got2, got) and not got2.requires_grad


class _Counts:
    """Counting wrappers around ops.masked_cross_attention / ops.self_attention and the library's two backward entry
    points."""

    def __init__(self, monkeypatch):
        from unscene3d_amd import ops
        self.n = {"cross": 0, "self": 0, "cross_bwd": 0, "self_bwd": 0, "max_L": 0}

        def wrap(fn, key, queries):
            def counted(*a, **kw):
                self.n[key] += 1
                self.n["max_L"] = max(self.n["max_L"], int(queries(a)))
                return fn(*a, **kw)
            return counted

        monkeypatch.setattr(ops, "masked_cross_attention", wrap(ops.masked_cross_attention, "cross", lambda a: a[0].shape[0]))
        monkeypatch.setattr(ops, "self_attention", wrap(ops.self_attention, "self", lambda a: a[0].shape[0]))
        monkeypatch.setattr(ops.lib, "usc_attn_bwd", wrap(ops.lib.usc_attn_bwd, "cross_bwd", lambda a: a[7]))
        monkeypatch.setattr(ops.lib, "usc_self_attn_bwd", wrap(ops.lib.usc_self_attn_bwd, "self_bwd", lambda a: a[6]))

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.n, 0)
        return n


def _model_at_150(device, monkeypatch, fused):
    """Two AdamW steps and eval_step of InstanceSegmentation at model.num_queries=150 on two ~6 k-voxel scenes, with the
    fused-call counts of the training steps and of eval_step."""
    import test_gpu_eval_parity as EP
    from unscene3d_amd.models import mask3d

    monkeypatch.setattr(mask3d, "_FUSED_ATTN_WIDE", fused)
    counts = _Counts(monkeypatch)
    seen = {}
    from unscene3d_amd.trainer.trainer import InstanceSegmentation
    orig_eval = InstanceSegmentation.eval_step
    grads = {}

    def eval_counted(self, *a, **kw):
        grads["query_projection"] = [p.grad.clone() for p in self.model.query_projection.parameters() if p.grad is not None]
        seen["train"] = counts.take()
        res = orig_eval(self, *a, **kw)
        seen["eval"] = counts.take()
        return res

    monkeypatch.setattr(InstanceSegmentation, "eval_step", eval_counted)
    out = EP._train_then_eval(device, 2, 6000, 5150, ("model.num_queries=150",))
    return out, seen, grads


def test_model_at_150_queries_takes_the_fused_path(device, monkeypatch):
    """`model.num_queries=150` (the reference's export recipe): every decoder pass of eval_step runs the fused cross and
    self attention (12 each, 150 queries), the training steps run their backward, the losses are finite and
    query_projection gets a gradient; logits and masks of all 13 levels within 1e-3 of the oracle's eval forward, the
    thresholded attention masks within 1e-4 of the bits."""
    import numpy as np
    import test_gpu_eval_parity as EP

    (cfg, module, data, target, res, dev_masks), seen, grads = _model_at_150(device, monkeypatch, True)
    assert seen["eval"]["cross"] == 12 and seen["eval"]["self"] == 12 and seen["eval"]["max_L"] == 150, seen
    assert seen["eval"]["cross_bwd"] == 0 and seen["eval"]["self_bwd"] == 0
    assert seen["train"]["cross"] >= 24 and seen["train"]["self"] >= 24 and seen["train"]["max_L"] == 150, seen
    assert seen["train"]["cross_bwd"] == seen["train"]["cross"] and seen["train"]["self_bwd"] == seen["train"]["self"], seen
    assert grads["query_projection"] and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
                                             for g in grads["query_projection"])
    assert res is not None and all(np.isfinite(v) for v in res["losses"].values())
    out_ref, ex = EP._oracle_eval(cfg, module, data, target, dev_masks)
    out = res["output"]
    cm = out["backbone_features"].coordinate_manager
    sizes = [max(EP._level_rows(cm, ts)) for ts in (16, 8, 4, 2)]
    assert len(ex.dev) == 12
    for k, m in enumerate(ex.dev):
        assert m.shape == (2, sizes[k % 4], 150), (k, m.shape)
    print(f"150 queries: attention-mask bits differing {ex.diff}/{ex.bits}")
    assert ex.bits > 0 and ex.diff <= 1e-4 * ex.bits, (ex.diff, ex.bits)
    levels_dev = list(out["aux_outputs"]) + [{"pred_logits": out["pred_logits"], "pred_masks": out["pred_masks"]}]
    levels_ref = list(out_ref["aux_outputs"]) + [{"pred_logits": out_ref["pred_logits"],
                                                  "pred_masks": out_ref["pred_masks"]}]
    assert len(levels_dev) == len(levels_ref) == 13
    worst = 0.0
    for ld, lr in zip(levels_dev, levels_ref):
        assert ld["pred_logits"].shape[1] == 150
        errs = [rel_err(ld["pred_logits"], lr["pred_logits"])] + [rel_err(ld["pred_masks"][b], lr["pred_masks"][b])
                                                                  for b in range(2)]
        worst = max(worst, *errs)
        assert all(e < EP.REL_TOL for e in errs), errs
    print(f"150 queries: worst rel err over 13 levels {worst:.2e}")


def test_switch_off_takes_the_plain_operators(device, monkeypatch):
    """USC3D_FUSED_ATTN_WIDE=0 (the module flag): at 150 queries no fused attention call in training or eval_step, and
    eval_step still returns."""
    import numpy as np

    (cfg, module, data, target, res, dev_masks), seen, _ = _model_at_150(device, monkeypatch, False)
    assert all(v == 0 for v in seen["eval"].values()) and all(v == 0 for v in seen["train"].values()), seen
    assert res is not None and len(dev_masks) == 12 and dev_masks[0].shape[2] == 150
    assert all(np.isfinite(v) for v in res["losses"].values())
    assert res["output"]["pred_logits"].shape[1] == 150
