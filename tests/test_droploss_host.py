"""CPU: DropLoss (reference models/criterion.py:194-200) against tests/golden/criterion_droploss.npz — the reference's own
`SetCriterion(use_droploss=True)` on a constructed case (tests/golden/make_golden_droploss.py: a pair with I/U exactly
1/10, one with 0.1 <= I/U < 1/9, dropped pairs, a pair with U = 0) for the thresholds 0.1 and 0.01.

  * both operator branches of models/criterion.py (`_batched_losses`, which `forward` takes whenever every level matches
    the same number of targets, and the per-level `get_loss` route) reproduce the golden losses, weights and gradients
    under the golden assignment;
  * the float64 weighted restatement of tests/droploss_ref.py — the yardstick of tests/test_gpu_droploss.py — equals
    the golden too, in float32 and float64;
  * the seeded cases of the GPU tests are what they claim: where a threshold is meant to split the matched pairs, the
    oracle's weights contain kept and dropped ones.
"""
import os

import numpy as np
import pytest
import torch

import criterion_cases as CC
import droploss_ref as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_droploss.npz")


@pytest.fixture
def golden():          # per test: criterion_cases.oracle_inputs makes the case's own float32 logits the autograd leaves
    z = np.load(GOLDEN)
    case, indices = DR.golden_case(z)
    return z, case, indices


def _criterion(case, thresh):
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    matcher = HungarianMatcher(cost_noise_robust=0.0, num_points=-1, **CC.COST_WEIGHTS)
    return SetCriterion(num_classes=case["C"], matcher=matcher, weight_dict=dict(case["weights"]),
                        eos_coef=case["eos_coef"], losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                        importance_sample_ratio=0.75, class_weights=-1, use_droploss=True, droploss_iou_thresh=thresh)


def _run(crit, case, batched):
    outputs, targets, levels = CC.oracle_inputs(case, torch.float32, requires_grad=True)
    if batched:
        losses = crit(outputs, targets, mask_type=CC.MASK_TYPE)
    else:                                             # the per-level route forward takes when the levels cannot be batched
        idx = crit.match_all_levels(levels, targets, CC.MASK_TYPE)
        losses = {}
        for l, lv in enumerate(levels):
            for name in crit.losses:
                d = crit.get_loss(name, lv, targets, idx[l], 1.0, CC.MASK_TYPE)
                losses.update({k + ("" if l == 0 else f"_{l - 1}"): v for k, v in d.items()})
        w = crit.__dict__.pop("_level_drop_weights")
        crit.last_drop_weights = [w[l * case["B"]:(l + 1) * case["B"]] for l in range(case["L"])]
    sum(v * case["weights"][k] for k, v in losses.items()).backward()
    return losses, levels


def _check_against_golden(z, k, case, losses, wts, dlogits, dmasks, rtol_loss=1e-5, atol_grad=1e-6):
    assert sorted(losses) == sorted(n[len(f"t{k}/loss/"):] for n in z.files if n.startswith(f"t{k}/loss/"))
    for name, v in losses.items():
        want = float(z[f"t{k}/loss/{name}"])
        assert abs(float(v) - want) <= rtol_loss * max(1.0, abs(want)), (name, float(v), want)
    for l in range(case["L"]):
        g = z[f"t{k}/logits_grad_{l}"]
        assert np.abs(dlogits[l].numpy() - g).max() <= atol_grad + 1e-4 * np.abs(g).max(), f"dlogits level {l}"
        for b in range(case["B"]):
            assert np.array_equal(np.asarray(wts[l][b], dtype=np.float32), z[f"t{k}/wts_{l}_{b}"]), (l, b)
            g = z[f"t{k}/masks_grad_{l}_{b}"]
            got = dmasks[l][b].numpy()
            assert np.abs(got - g).max() <= atol_grad + 1e-4 * np.abs(g).max(), f"dmasks level {l} scene {b}"
            assert np.array_equal(got == 0, g == 0), "a dropped or unmatched column is exactly zero, and only those"


@pytest.mark.parametrize("k", [0, 1], ids=["thresh0.1", "thresh0.01"])
@pytest.mark.parametrize("batched", [True, False], ids=["batched_losses", "per_level"])
def test_operator_branches_reproduce_the_reference(golden, batched, k):
    """`_batched_losses` formed |pred| + |target| in the denominator before this test existed: the pair with
    0.1 <= I/U < 1/9 (level 0, scene 0, target 1) was dropped where the reference keeps it."""
    z, case, indices = golden
    crit = _criterion(case, float(z["thresholds"][k]))
    crit.forced_indices = indices
    losses, levels = _run(crit, case, batched)
    zero = torch.zeros_like
    _check_against_golden(z, k, case, {n: v.detach() for n, v in losses.items()},
                          [[w.numpy() for w in lv] for lv in crit.last_drop_weights],
                          [lv["pred_logits"].grad for lv in levels],
                          [[m.grad if m.grad is not None else zero(m) for m in lv["pred_masks"]] for lv in levels])


def test_own_assignment_is_the_references(golden):
    z, case, indices = golden
    crit = _criterion(case, 0.1)
    outputs, targets, levels = CC.oracle_inputs(case, torch.float32)
    crit(outputs, targets, mask_type=CC.MASK_TYPE)
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert torch.equal(crit.last_indices[l][b][0], indices[l][b][0])
            assert torch.equal(crit.last_indices[l][b][1], indices[l][b][1])


@pytest.mark.parametrize("k", [0, 1], ids=["thresh0.1", "thresh0.01"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_weighted_restatement_equals_the_golden(golden, dtype, k):
    z, case, indices = golden
    r = DR.weighted_run(case, dtype, indices, thresh=float(z["thresholds"][k]))
    _check_against_golden(z, k, case, r["losses"], [[w.numpy() for w in lv] for lv in r["wts"]],
                          [g.float() for g in r["dlogits"]], [[g.float() for g in lv] for lv in r["dmasks"]])
    inter, fgn, uni = r["counts"][0][0]                 # the constructed pairs, in target order (query t <-> target t)
    order = np.argsort(indices[0][0][1].numpy())
    assert inter.numpy()[order].tolist() == [1, 2, 1, 0, 7] and uni.numpy()[order].tolist() == [10, 19, 20, 14, 8]
    assert tuple(int(c[int(np.argsort(indices[0][1][1].numpy())[0])]) for c in r["counts"][0][1])[::2] == (0, 0)


def test_restatement_with_unit_weights_is_the_plain_oracle(golden):
    z, case, indices = golden
    ones = [[torch.ones(t) for t in case["T"]] for _ in range(case["L"])]
    a = DR.weighted_run(case, torch.float64, indices, wts=ones)
    b = CC.oracle_run(case, torch.float64, indices)
    for name in b["losses"]:
        assert abs(float(a["losses"][name]) - float(b["losses"][name])) <= 1e-12, name
    for l in range(case["L"]):
        for s in range(case["B"]):
            assert float((a["dmasks"][l][s] - b["dmasks"][l][s]).abs().max()) <= 1e-12


@pytest.mark.parametrize("index", DR.GPU_CASES, ids=[CC.case_ids()[i] for i in DR.GPU_CASES])
def test_seeded_cases_split_where_they_are_meant_to(index):
    """Checked with the oracle alone (its own float32 assignment): under the tie threshold the chosen pair is kept, and in
    the regimes meant to split (T >= 2) the weights hold kept and dropped pairs; ties_zero drops every pair at 0.1 and
    0.01; every degenerate case holds a pair with U = 0."""
    case = DR.make_case(index)
    own = CC.oracle_run(case, torch.float32)["own_indices"]
    _, counts = DR.weights_of(case, own, 0.1)
    tie = DR.tie_threshold(counts)
    wts, _ = DR.weights_of(case, own, tie)
    flat = np.concatenate([w.numpy() for lv in wts for w in lv])
    ratios = np.concatenate([(i.numpy().astype(np.float32) / np.maximum(u.numpy(), 1).astype(np.float32))[u.numpy() > 0]
                             for i, _, u in counts[0]])
    assert (ratios == np.float32(tie)).any() and flat.max() == 1.0
    if case["regime"] in DR.SPLIT_REGIMES and max(case["T"]) >= 2:
        assert flat.min() == 0.0 and flat.max() == 1.0, (case["name"], tie)
    if case["regime"] == "ties_zero":
        for thresh in (0.1, 0.01):
            w, _ = DR.weights_of(case, own, thresh)
            assert all(float(x.max()) == 0.0 for lv in w for x in lv)
    if case["regime"] == "degenerate":
        assert all(int(u.min()) == 0 for lv in counts for _, _, u in lv)          # the empty target's pair
