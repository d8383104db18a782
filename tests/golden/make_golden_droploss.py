#!/usr/bin/env python
"""Golden-vector generator for DropLoss — runs ONLY where /root/reference exists (like make_golden.py, whose stubs it
uses).  Imports the reference's matcher and criterion in place, runs `SetCriterion(use_droploss=True)` on a small
constructed case for the thresholds 0.1 and 0.01 and stores inputs, assignments, losses, per-pair weights and input
gradients in tests/golden/criterion_droploss.npz.  Nothing of the reference is copied; the fixture is data.

    python tests/golden/make_golden_droploss.py

The case: L = 2 levels (final + one aux), B = 2 scenes, S = (60, 48) rows, Q = 12 queries, 6 object classes, bool
targets.  Query t of a scene is built for target t (a peaked class logit on the target's label, weak mask logits, so
the pair's own overlap can be anything), the queries >= T are +8 everywhere and match nothing.  Level 0 holds the pairs
the rule is pinned on; the generator asserts that the reference's own assignment contains them:
    scene 0, target 0   I = 1, U = 10: I/U exactly 1/10 — kept at 0.1 (`>=`)
    scene 0, target 1   I = 2, U = 19: 0.1 <= I/U < 1/9 — kept; |pred| + |target| = 21 in the denominator would drop it
    scene 0, target 2   I = 1, U = 20: dropped at 0.1, kept at 0.01
    scene 0, target 3   I = 0, U = 14: dropped at both
    scene 0, target 4   an ordinary well-predicted pair
    scene 1, target 0   empty target, nothing predicted: U = 0, 0/0 — dropped at every threshold
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference_models  # noqa: E402

L, B, Q, NUM_CLASSES = 2, 2, 12, 7
S, T = [60, 48], [5, 4]
LOSS_WEIGHTS = (2.0, 5.0, 2.0, 0.0)              # loss_ce, loss_mask, loss_dice, loss_noise_robust


def rows(*r):
    m = torch.zeros(max(S), dtype=torch.bool)
    for a, b in r:
        m[a:b] = True
    return m


def build_inputs():
    g = torch.Generator().manual_seed(2024)
    tms, fgs = [], []
    # scene 0: (target rows, predicted-foreground rows) per pair
    pairs0 = [(rows((0, 10)), rows((0, 1))),                      # I 1, F 1, cnt 10 -> U 10
              (rows((10, 22)), rows((20, 29))),                   # I 2, F 9, cnt 12 -> U 19
              (rows((30, 38)), rows((37, 50))),                   # I 1, F 13, cnt 8 -> U 20
              (rows((40, 46)), rows((50, 58))),                   # I 0, F 8, cnt 6 -> U 14
              (rows((52, 60)), rows((52, 59)))]                   # I 7, F 7, cnt 8 -> U 8
    pairs1 = [(rows(), rows()),                                   # empty target, no foreground: U 0
              (rows((0, 16)), rows((2, 18))),                     # I 14, U 18
              (rows((16, 30)), rows((28, 40))),                   # I 2, U 24: dropped at 0.1
              (rows((30, 48)), rows((30, 44)))]                   # I 14, U 18
    labels = [torch.tensor([0, 1, 2, 3, 4]), torch.tensor([5, 0, 1, 2])]
    for b, pairs in enumerate((pairs0, pairs1)):
        tms.append(torch.stack([t[:S[b]] for t, _ in pairs]))
        fgs.append(torch.stack([f[:S[b]] for _, f in pairs]))
    masks, logits = [], []
    for l in range(L):
        per_scene = []
        for b in range(B):
            x = torch.full((S[b], Q), 8.0) + torch.rand(S[b], Q, generator=g)
            amp = 0.25 + 0.5 * torch.rand(S[b], T[b], generator=g)
            fg = fgs[b].T if l == 0 else (tms[b].T ^ (torch.rand(S[b], T[b], generator=g) < 0.3))
            x[:, :T[b]] = torch.where(fg, amp, -amp)
            per_scene.append(x)
        masks.append(per_scene)
        lg = torch.randn(B, Q, NUM_CLASSES, generator=g)
        lg[:, :, NUM_CLASSES - 1] += 4.0
        for b in range(B):
            for t in range(T[b]):
                lg[b, t] = torch.randn(NUM_CLASSES, generator=g)
                lg[b, t, labels[b][t]] += 10.0
        logits.append(lg)
    return tms, labels, masks, logits


def run_reference(mods, tms, labels, masks, logits, thresh):
    crit_mod = mods["criterion"]
    matcher = mods["matcher"].HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, cost_noise_robust=0.0,
                                               num_points=-1)
    wd = dict(zip(("loss_ce", "loss_mask", "loss_dice", "loss_noise_robust"), LOSS_WEIGHTS))
    wd.update({f"{k}_{i}": v for i in range(L - 1) for k, v in list(wd.items())})
    crit = crit_mod.SetCriterion(num_classes=NUM_CLASSES, matcher=matcher, weight_dict=wd, eos_coef=0.1,
                                 losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                                 importance_sample_ratio=0.75, class_weights=-1, use_droploss=True,
                                 droploss_iou_thresh=thresh)
    lg = [x.clone().requires_grad_() for x in logits]
    pm = [[x.clone().requires_grad_() for x in lv] for lv in masks]
    targets = [{"labels": labels[b].clone(), "segment_mask": tms[b].clone()} for b in range(B)]
    outputs = {"pred_logits": lg[0], "pred_masks": pm[0],
               "aux_outputs": [{"pred_logits": lg[i], "pred_masks": pm[i]} for i in range(1, L)]}
    seen = []                                     # the weights the reference hands to its mask loss, in call order
    orig = crit_mod.sigmoid_ce_loss_jit

    def spy(inputs, tgt, num_masks, weights):
        seen.append(weights.detach().clone())
        return orig(inputs, tgt, num_masks, weights)
    crit_mod.sigmoid_ce_loss_jit = spy
    try:
        losses = crit(outputs, targets, mask_type="segment_mask")
    finally:
        crit_mod.sigmoid_ce_loss_jit = orig
    total = sum(losses[k] * wd[k] for k in losses)
    total.backward()
    assert len(seen) == L * B                     # level 0 (final) scene 0, scene 1, then the aux levels
    levels = [outputs] + outputs["aux_outputs"]
    idx = [matcher({k: v for k, v in lv.items() if k != "aux_outputs"}, targets, "segment_mask") for lv in levels]
    return dict(losses={k: v.detach().numpy() for k, v in losses.items()}, total=total.detach().numpy(),
                wts=[[seen[l * B + b].numpy() for b in range(B)] for l in range(L)],
                idx=[[(i.numpy(), j.numpy()) for i, j in lv] for lv in idx],
                glogits=[x.grad.numpy() for x in lg], gmasks=[[x.grad.numpy() for x in lv] for lv in pm])


def main():
    cwd = os.getcwd()
    mods = import_reference_models()
    tms, labels, masks, logits = build_inputs()
    out = {"L": np.int64(L), "B": np.int64(B), "Q": np.int64(Q), "C": np.int64(NUM_CLASSES),
           "eos_coef": np.float32(0.1), "loss_weights": np.array(LOSS_WEIGHTS, np.float32),
           "thresholds": np.array([0.1, 0.01])}
    for l in range(L):
        out[f"logits_{l}"] = logits[l].numpy()
        for b in range(B):
            out[f"masks_{l}_{b}"] = masks[l][b].numpy()
    for b in range(B):
        out[f"tgt_mask_{b}"] = np.packbits(tms[b].numpy(), axis=1)
        out[f"tgt_shape_{b}"] = np.array(tms[b].shape)
        out[f"labels_{b}"] = labels[b].numpy()
    first = None
    for k, thresh in enumerate((0.1, 0.01)):
        r = run_reference(mods, tms, labels, masks, logits, thresh)
        if first is None:
            first = r
            for l in range(L):
                for b in range(B):
                    out[f"match_q_{l}_{b}"], out[f"match_t_{l}_{b}"] = r["idx"][l][b]
        else:                                     # the assignment does not see the weights
            assert all(np.array_equal(a, c) for la, lc in zip(first["idx"], r["idx"]) for pa, pc in zip(la, lc)
                       for a, c in zip(pa, pc))
        for name, v in r["losses"].items():
            out[f"t{k}/loss/{name}"] = v
        out[f"t{k}/total"] = r["total"]
        for l in range(L):
            out[f"t{k}/logits_grad_{l}"] = r["glogits"][l]
            for b in range(B):
                out[f"t{k}/wts_{l}_{b}"] = r["wts"][l][b]
                out[f"t{k}/masks_grad_{l}_{b}"] = r["gmasks"][l][b]
        print("threshold", thresh, "total", float(r["total"]), "weights", [[w.tolist() for w in lv] for lv in r["wts"]])
    # ---- the constructed pairs are among the reference's own matches (level 0)
    def ratio(b, t):
        q, tt = first["idx"][0][b]
        p = int(np.nonzero(tt == t)[0][0])
        fg = masks[0][b][:, int(q[p])] > 0
        i, u = int((fg & tms[b][t]).sum()), int((fg | tms[b][t]).sum())
        return p, i, u, int(fg.sum()) + int(tms[b][t].sum())
    w01, w001 = out["t0/wts_0_0"], out["t1/wts_0_0"]
    p, i, u, _ = ratio(0, 0)
    assert (i, u) == (1, 10) and w01[p] == 1.0, "I/U exactly 1/10 is kept"
    p, i, u, s = ratio(0, 1)
    assert 0.1 <= i / u < 1 / 9 and i / s < 0.1 and w01[p] == 1.0, "0.1 <= I/U < 1/9 is kept (and |pred|+|target| drops it)"
    p, i, u, _ = ratio(0, 2)
    assert 0.01 <= i / u < 0.1 and w01[p] == 0.0 and w001[p] == 1.0, "a dropped pair"
    p, i, u, _ = ratio(0, 3)
    assert i == 0 and u > 0 and w01[p] == 0.0 and w001[p] == 0.0
    p, i, u, _ = ratio(1, 0)
    assert (i, u) == (0, 0) and out["t0/wts_0_1"][p] == 0.0 and out["t1/wts_0_1"][p] == 0.0, "U = 0 is dropped"
    path = os.path.join(HERE, "criterion_droploss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    os.chdir(cwd)


if __name__ == "__main__":
    main()
