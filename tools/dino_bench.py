#!/usr/bin/env python
"""DINO ViT-S/8 image encoder, per frame at 192 x 256 (stride 4: 47 x 63 patches + class token = 2 962 tokens): the
attention core alone at (B, T, H) = (1, 2962, 6), and the whole encoder (blocks 0..9, then norm1 and qkv of block 10, the
bilinear resize: `DinoNet` in 'descriptors' mode), each as
    plain     torch's bmm, softmax, bmm (USC3D_VIT_ATTN=0: the reference's own operators, the yardstick)
    f32       the fused kernel, f32 operands
    bf16      the fused kernel with bf16 operands (encoder: bf16 linears as well)
The variants alternate inside every round of ONE process (--rounds rounds of --reps back-to-back calls after --warmup
rounds); a round's time is a HIP-event span over its calls.  Reported per variant: median, min and max of the per-call
time over the rounds (the spread), peak device memory above what was allocated before the call, and for the attention
core the achieved FLOP/s (4 * T^2 * 64 * H per call, from the shape) with its fraction of the MFMA peak of the operand
type (157.3 TF f32, 2 500 TF bf16: spec).  Random weights, random (gaussian) data.  Prints one JSON line.

    python tools/dino_bench.py [--rounds 10] [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.models.encoders_2d import DinoNet, dino  # noqa: E402

H_IMG, W_IMG, T, HEADS, D = 192, 256, 2962, 6, 64
PEAK_TF = {"plain": 157.3, "f32": 157.3, "bf16": 2500.0}


def measure(variants, rounds, reps, warmup):
    """variants: name -> callable.  -> name -> {median_ms, min_ms, max_ms, peak_mem_mb}"""
    times = {k: [] for k in variants}
    peak = {}
    for r in range(warmup + rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            if r == 0:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r == 0:
                peak[name] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
            if r >= warmup:
                times[name].append(a.elapsed_time(b) / reps)
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "max_ms": round(float(np.max(v)), 4), "peak_mem_mb": round(peak[k], 1)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dino_bench: no HIP device — nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = {"image": [H_IMG, W_IMG], "tokens": T, "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}

    with torch.no_grad():
        # ---- attention core alone
        qkv = torch.randn((1, T, 3 * HEADS * D), device=dev)
        core = measure({
            "plain": lambda: dino.plain_attention(qkv, 1, T, HEADS, D ** -0.5),
            "f32": lambda: ops.vit_attention(qkv, 1, T, HEADS, D ** -0.5, "f32"),
            "bf16": lambda: ops.vit_attention(qkv, 1, T, HEADS, D ** -0.5, "bf16"),
        }, a.rounds, a.reps, a.warmup)
        flop = 4.0 * T * T * D * HEADS
        for name, r in core.items():
            r["tflops"] = round(flop / (r["median_ms"] * 1e-3) / 1e12, 2)
            r["frac_of_mfma_peak"] = round(r["tflops"] / PEAK_TF[name], 4)
        ref = dino.plain_attention(qkv, 1, T, HEADS, D ** -0.5)
        for name in ("f32", "bf16"):
            got = ops.vit_attention(qkv, 1, T, HEADS, D ** -0.5, name)
            core[name]["max_abs_diff_vs_plain"] = float((got - ref).abs().max())
        out["attention_core"] = core
        out["attention_core_flop"] = flop

        # ---- whole encoder, one frame
        cfg = SimpleNamespace(image_data=SimpleNamespace(image_backbone="dino_vits8", dino_vit_stride=4, dino_vit_layer=10,
                                                         dino_vit_feature="descriptors"))
        nets = {p: DinoNet(cfg, None, precision=p) for p in ("f32", "bf16")}
        for p in nets.values():
            for w in p.parameters():
                torch.nn.init.normal_(w, std=0.02)
            for m in p.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    torch.nn.init.ones_(m.weight)
                    torch.nn.init.zeros_(m.bias)
            p.to(dev).eval()
        nets["bf16"].load_state_dict(nets["f32"].state_dict())
        img = torch.randn((1, 1, 3, H_IMG, W_IMG), device=dev)

        def run(net, kernel):
            def f():
                dino.VIT_ATTN = kernel
                try:
                    return net(img)[0]
                finally:
                    dino.VIT_ATTN = True
            return f

        enc = measure({"plain": run(nets["f32"], False), "f32": run(nets["f32"], True), "bf16": run(nets["bf16"], True)},
                      a.rounds, a.reps, a.warmup)
        base = run(nets["f32"], False)()
        for name, net in (("f32", nets["f32"]), ("bf16", nets["bf16"])):
            got = run(net, True)()
            enc[name]["rel_l2_vs_plain"] = float((got - base).norm() / base.norm())
        out["encoder_frame"] = enc
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
