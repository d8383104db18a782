"""DropLoss restated on oracle/criterion_ref.py (reference models/criterion.py:194-200), the yardstick of
tests/test_droploss_host.py and tests/test_gpu_droploss.py.  TEST INFRASTRUCTURE ONLY.

The weight of a matched pair (q, t) of a level, with fg[s] = x[s, q] > 0 and the target mask as bits:
    I = sum_s fg[s] & tm[t, s]        U = sum_s fg[s] | tm[t, s] = F + cnt[t] - I,   F = sum_s fg[s]
    w = 1 if U > 0 and float32(I) / float32(U) >= float32(thresh) else 0
(0 / 0 is the reference's NaN, which no threshold admits; torch divides the two int64 sums in float32 and compares with
the threshold cast to float32).  The weights carry no gradient and do not depend on the precision the losses are
computed in: `x > 0` is decided on the float32 inputs, everything after it is integer.

    loss_mask_l = sum_pairs w * bce_pair / T        loss_dice_l = sum_pairs w * dice_pair / T
The per-pair terms are oracle.criterion_ref.loss_masks on one pair at a time (num_masks = 1 there), so they keep the dtype
of the inputs: float32 = the reference's own arithmetic, float64 = the yardstick.  loss_ce does not see the weights.
"""
import numpy as np
import torch

import criterion_cases as CC
from oracle import criterion_ref as CR


def pair_counts(x, tm, src, tid):
    """x [S, >= Q] mask logits, tm bool [T, S], (src, tid) the matched pairs -> int64 (I, F, U) per pair, pair order."""
    fg = (x[:, src.long()] > 0).T                                               # [P, S]
    t = tm[tid.long()].bool()
    inter = (fg & t).sum(1)
    return inter, fg.sum(1), (fg | t).sum(1)


def pair_weights(inter, union, thresh):
    i, u = inter.numpy().astype(np.float32), union.numpy().astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = i / u                                                             # float32; 0 / 0 = NaN
    return torch.from_numpy((iou >= np.float32(thresh)).astype(np.float32))    # NaN >= x is False


def weights_of(case, indices, thresh):
    """-> (wts [L][B] f32 [T_b], counts [L][B] (I, F, U)) under `indices` [L][B] (src, tid)."""
    wts, counts = [], []
    for l in range(case["L"]):
        wl, cl = [], []
        for b in range(case["B"]):
            src, tid = indices[l][b]
            inter, fgn, uni = pair_counts(case["masks"][l][b][:, :case["Q"]], case["tm"][b], src.cpu(), tid.cpu())
            assert torch.equal(uni, fgn + case["tm"][b][tid.cpu().long()].sum(1) - inter)
            wl.append(pair_weights(inter, uni, thresh))
            cl.append((inter, fgn, uni))
        wts.append(wl)
        counts.append(cl)
    return wts, counts


def _fresh_leaves(case):
    """criterion_cases.oracle_inputs turns the case's own float32 logits into autograd leaves (`.to(float32)` is the
    identity): an earlier run's gradient would be added to, and a float64 copy of such a leaf is no leaf at all."""
    for lg in case["logits"]:
        lg.requires_grad_(False)
        lg.grad = None


def weighted_run(case, dtype, indices, thresh=None, wts=None):
    """The weighted criterion in `dtype` under the forced `indices` -> the layout of criterion_cases.oracle_run (losses,
    parts [L][B] [4], table [L, 4], den_tot [L], dlogits [L], dmasks [L][B]) plus wts / counts.  `wts` given: those
    weights are imposed (e.g. all ones = the criterion without DropLoss)."""
    counts = None
    if wts is None:
        wts, counts = weights_of(case, indices, thresh)
    _fresh_leaves(case)
    outputs, targets, levels = CC.oracle_inputs(case, dtype, requires_grad=True)
    losses, parts = {}, []
    for l, lv in enumerate(levels):
        idx = [(s.long().cpu(), t.long().cpu()) for s, t in indices[l]]
        sfx = "" if l == 0 else f"_{l - 1}"
        losses["loss_ce" + sfx] = CR.loss_labels(lv, targets, idx, case["C"] - 1, case["eos_coef"])["loss_ce"]
        ce_parts = CR.loss_parts(lv, targets, idx, CC.MASK_TYPE, case["C"] - 1, case["eos_coef"])
        lm, ldice, pl = [], [], []
        for b, (src, tid) in enumerate(idx):
            T = len(src)
            one = {"pred_masks": [lv["pred_masks"][b]]}
            m = torch.zeros((), dtype=dtype)
            d = torch.zeros((), dtype=dtype)
            for p in range(T):
                if float(wts[l][b][p]) == 0.0:                     # a dropped pair adds exactly 0 (no 0 * inf)
                    continue
                pair = CR.loss_masks(one, [targets[b]], [(src[p:p + 1], tid[p:p + 1])], CC.MASK_TYPE)
                m = m + pair["loss_mask"]
                d = d + pair["loss_dice"]
            lm.append(m / T)
            ldice.append(d / T)
            pl.append(torch.stack([ce_parts[b][0], ce_parts[b][1], lm[-1].detach(), ldice[-1].detach()]))
        losses["loss_mask" + sfx] = torch.sum(torch.stack(lm))
        losses["loss_dice" + sfx] = torch.sum(torch.stack(ldice))
        losses["loss_noise_robust" + sfx] = torch.zeros((), dtype=dtype)
        parts.append(pl)
    total = sum(losses[k] * case["weights"][k] for k in losses)
    total.backward()
    table = torch.stack([torch.stack([sum(p[0] for p in ps) / sum(p[1] for p in ps), sum(p[2] for p in ps),
                                      sum(p[3] for p in ps), torch.zeros((), dtype=dtype)]) for ps in parts])
    den_tot = torch.stack([sum(p[1] for p in ps) for ps in parts])
    zero = torch.zeros_like
    return dict(indices=indices, losses={k: v.detach() for k, v in losses.items()}, parts=parts, table=table,
                den_tot=den_tot, wts=wts, counts=counts,
                dlogits=[lv["pred_logits"].grad if lv["pred_logits"].grad is not None else zero(lv["pred_logits"])
                         for lv in levels],
                dmasks=[[m.grad if m.grad is not None else zero(m) for m in lv["pred_masks"]] for lv in levels])


# ---- the golden fixture as a case of criterion_cases' layout --------------------------------------------------------
def golden_case(z):
    """tests/golden/criterion_droploss.npz -> (case, indices [L][B]); level 0 is the final prediction."""
    L, B, Q, C = (int(z[k]) for k in ("L", "B", "Q", "C"))
    tm = [torch.from_numpy(np.unpackbits(z[f"tgt_mask_{b}"], axis=1)[:, :int(z[f"tgt_shape_{b}"][1])].astype(bool))
          for b in range(B)]
    weights = {}
    for l in range(L):
        for n, w in zip(CC.LOSS_NAMES, z["loss_weights"]):
            weights[n + ("" if l == 0 else f"_{l - 1}")] = float(w)
    case = dict(name="golden-droploss", regime="golden", L=L, B=B, Q=Q, C=C, ld=Q, S=[int(t.shape[1]) for t in tm],
                T=[int(t.shape[0]) for t in tm], eos_coef=float(z["eos_coef"]),
                labels=[torch.from_numpy(z[f"labels_{b}"]) for b in range(B)], tm=tm,
                masks=[[torch.from_numpy(z[f"masks_{l}_{b}"]) for b in range(B)] for l in range(L)],
                logits=[torch.from_numpy(z[f"logits_{l}"]) for l in range(L)], weights=weights)
    indices = [[(torch.from_numpy(z[f"match_q_{l}_{b}"]), torch.from_numpy(z[f"match_t_{l}_{b}"])) for b in range(B)]
               for l in range(L)]
    return case, indices


# ---- the seeded cases the device is tested on -----------------------------------------------------------------------
# a covering selection of criterion_cases._SHAPES (by index): S in {1, 31, 32, 33, 609}, T in {1, 8, 9, 16, 17, 32},
# Q in {32, 63, 100, 128}, ld = Q / between / 128, L in {1, 13, 16}, B in {1, 2, 3}, every regime
GPU_CASES = [0, 1, 6, 10, 13, 17, 18, 19, 23]
# the regimes whose tie threshold (below) is meant to split the matched pairs into kept and dropped ones; in the others
# every pair has the same ratio: 1 on a confidently predicted target, 0 where nothing is foreground
SPLIT_REGIMES = ("random", "ties_dup", "degenerate")


def make_case(index):
    """criterion_cases.make_case(index); in the degenerate regime the query that the float32 oracle matches to the empty
    target 0 is made background on every row (x -> -|x|, at every level and scene), so that the pair has U = 0: the
    reference's 0 / 0.  (A random query has foreground rows, and U = F > 0 on an empty target.)  The change only lowers
    that pair's cost, so the pair stays matched; the tests assert that it does."""
    case = CC.make_case(index)
    if case["regime"] == "degenerate":
        own = CC.oracle_run(case, torch.float32)["own_indices"]
        for l in range(case["L"]):
            for b in range(case["B"]):
                src, tid = own[l][b]
                q = int(src[int((tid == 0).nonzero()[0])])
                case["masks"][l][b][:, q] = -case["masks"][l][b][:, q].abs()
        _fresh_leaves(case)
    return case


def tie_threshold(counts):
    """The float32 I / U of one matched pair of level 0 (the upper median over the scenes' pairs with U > 0), as a
    Python float: a threshold that this pair meets with equality and therefore has to be kept under."""
    r = []
    for inter, _, uni in counts[0]:
        ok = uni > 0
        r.extend((inter[ok].numpy().astype(np.float32) / uni[ok].numpy().astype(np.float32)).tolist())
    assert r, "no pair with U > 0"
    return float(sorted(r)[len(r) // 2])
