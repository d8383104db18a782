"""oracle/criterion_ref.py (the checker behind the "oracle step" of tests/test_gpu_step_parity.py) pinned by the
reference's own matcher + criterion: tests/golden/criterion.npz was recorded by importing models/matcher.py and
models/criterion.py in the build container (tests/golden/make_golden.py)."""
import os

import numpy as np
import torch

from oracle import criterion_ref as CR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion.npz")
WD = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0, "loss_noise_robust": 0.0}


def _case():
    z = np.load(GOLD)
    n_aux, B = int(z["n_aux"]), 2
    logits = [torch.from_numpy(z[f"logits_{i}"]).requires_grad_() for i in range(n_aux + 1)]
    masks = [[torch.from_numpy(z[f"masks_{i}_{b}"]).requires_grad_() for b in range(B)] for i in range(n_aux + 1)]
    targets = []
    for b in range(B):
        T, S = z[f"tgt_shape_{b}"]
        seg = torch.from_numpy(np.unpackbits(z[f"tgt_mask_{b}"], axis=1)[:, :S].astype(bool))
        targets.append({"labels": torch.ones(int(T), dtype=torch.int64), "segment_mask": seg})
    outputs = {"pred_logits": logits[-1], "pred_masks": masks[-1],
               "aux_outputs": [{"pred_logits": logits[i], "pred_masks": masks[i]} for i in range(n_aux)]}
    return z, outputs, targets, logits, masks


def test_oracle_assignment_matches_reference():
    z, outputs, targets, *_ = _case()
    idx = CR.hungarian_match({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets, "segment_mask")
    for b in range(2):
        assert np.array_equal(idx[b][0].numpy(), z[f"match_q_{b}"])
        assert np.array_equal(idx[b][1].numpy(), z[f"match_t_{b}"])


def test_oracle_losses_and_gradients_match_reference():
    z, outputs, targets, logits, masks = _case()
    info = {}
    losses = CR.set_criterion(outputs, targets, "segment_mask", num_classes=3, eos_coef=0.1, info=info)
    ref_keys = sorted(k[5:] for k in z.files if k.startswith("loss/"))
    assert sorted(losses) == ref_keys
    for k in ref_keys:
        np.testing.assert_allclose(losses[k].detach().numpy(), z["loss/" + k], rtol=1e-5, atol=1e-7)
    wd = dict(WD)
    wd.update({f"{k}_{i}": v for i in range(int(z["n_aux"])) for k, v in WD.items()})
    total = sum(losses[k] * wd[k] for k in losses)
    np.testing.assert_allclose(total.detach().numpy(), z["total"], rtol=1e-5)
    total.backward()
    for i in range(len(logits)):
        np.testing.assert_allclose(logits[i].grad.numpy(), z[f"logits_grad_{i}"], rtol=1e-4, atol=1e-7)
        for b in range(2):
            np.testing.assert_allclose(masks[i][b].grad.numpy(), z[f"masks_grad_{i}_{b}"], rtol=1e-4, atol=1e-8)
    # forced assignments reproduce the same numbers, and `info` carried the oracle's own
    again = CR.set_criterion(outputs, targets, "segment_mask", forced_indices=info["indices"])
    for k in ref_keys:
        assert float(again[k]) == float(losses[k])


def test_oracle_is_independent_of_the_package():
    src = open(CR.__file__).read()
    assert "unscene3d_amd" not in src.split('"""', 2)[2]         # outside the header docstring


# ---- the same oracle in float64: the yardstick of tests/test_gpu_criterion_f64.py -----------------------------------
def _case64():
    z, outputs, targets, logits, masks = _case()
    logits = [t.detach().double().requires_grad_() for t in logits]
    masks = [[m.detach().double().requires_grad_() for m in ms] for ms in masks]
    n_aux = int(z["n_aux"])
    outputs = {"pred_logits": logits[-1], "pred_masks": masks[-1],
               "aux_outputs": [{"pred_logits": logits[i], "pred_masks": masks[i]} for i in range(n_aux)]}
    return z, outputs, targets, logits, masks


def test_float64_oracle_assignment_matches_reference():
    z, outputs, targets, *_ = _case64()
    idx = CR.hungarian_match({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets, "segment_mask")
    for b in range(2):
        assert np.array_equal(idx[b][0].numpy(), z[f"match_q_{b}"])
        assert np.array_equal(idx[b][1].numpy(), z[f"match_t_{b}"])


def test_float64_oracle_losses_and_gradients_match_reference():
    z, outputs, targets, logits, masks = _case64()
    losses = CR.set_criterion(outputs, targets, "segment_mask", num_classes=3, eos_coef=0.1)
    ref_keys = sorted(k[5:] for k in z.files if k.startswith("loss/"))
    assert sorted(losses) == ref_keys
    for k in ref_keys:
        assert losses[k].dtype == torch.float64                                    # nothing fell back to float32
        np.testing.assert_allclose(losses[k].detach().numpy(), z["loss/" + k], rtol=1e-5, atol=1e-7)
    wd = dict(WD)
    wd.update({f"{k}_{i}": v for i in range(int(z["n_aux"])) for k, v in WD.items()})
    total = sum(losses[k] * wd[k] for k in losses)
    np.testing.assert_allclose(total.detach().numpy(), z["total"], rtol=1e-5)
    total.backward()
    for i in range(len(logits)):
        assert logits[i].grad.dtype == torch.float64
        np.testing.assert_allclose(logits[i].grad.numpy(), z[f"logits_grad_{i}"], rtol=1e-4, atol=1e-7)
        for b in range(2):
            np.testing.assert_allclose(masks[i][b].grad.numpy(), z[f"masks_grad_{i}_{b}"], rtol=1e-4, atol=1e-8)


# ---- the generated cases (tests/criterion_cases.py) are what they claim to be -----------------------------------------
import pytest  # noqa: E402

import criterion_cases as CC  # noqa: E402


def test_case_list_covers_the_stated_domain():
    cases = [CC.make_case(i) for i in range(len(CC.case_ids()))]
    seen = lambda f: {v for c in cases for v in f(c)}                              # noqa: E731
    assert seen(lambda c: c["T"]) >= {1, 8, 9, 16, 17, 32}
    assert seen(lambda c: c["S"]) >= {1, 31, 32, 33, 609, 3000}
    assert seen(lambda c: [c["Q"]]) >= {32, 63, 64, 65, 100, 127, 128}
    assert seen(lambda c: [c["C"]]) == {2, 3, 19}
    assert seen(lambda c: [c["L"]]) == {1, 13, 16}
    assert seen(lambda c: [c["B"]]) == {1, 2, 3}
    assert seen(lambda c: [c["eos_coef"]]) == {float(np.float32(0.1)), 1.0}
    kinds = seen(lambda c: ["Q" if c["ld"] == c["Q"] else "128" if c["ld"] == 128 else "mid"])
    assert kinds == {"Q", "mid", "128"}
    assert seen(lambda c: [c["regime"]]) == {"random", "confident", "saturated", "ties_zero", "ties_dup", "degenerate"}
    assert any(253 in lab.tolist() for c in cases for lab in c["labels"])
    for C in (2, 3, 19):                                                           # labels over all object classes
        got = {v for c in cases if c["C"] == C for lab in c["labels"] for v in lab.tolist()} - {253}
        assert got == set(range(C - 1)), (C, got)
    for c in cases:
        if c["B"] > 1:
            assert len(set(zip(c["S"], c["T"]))) == c["B"]                         # different (S, T) per scene
        w = [v for v in c["weights"].values()]
        pos = [v for v in w if v > 0]
        assert len(set(pos)) == len(pos) and 0.0 in w and c["weights"]["loss_noise_robust"] == 0.0


@pytest.mark.parametrize("index", range(len(CC.case_ids())), ids=CC.case_ids())
def test_generated_case_meets_its_conditions(index):
    case = CC.make_case(index)
    L, B, Q, C, ld = case["L"], case["B"], case["Q"], case["C"], case["ld"]
    # every condition of SetCriterion._fused_tables that is a property of the data
    assert 1 <= L <= 16 and Q <= 128 and len(case["logits"]) == L and len(case["masks"]) == L
    for l in range(L):
        assert case["logits"][l].shape == (B, Q, C) and case["logits"][l].dtype == torch.float32
        for b in range(B):
            t = case["masks"][l][b]
            assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and Q <= t.shape[1] == ld <= 128
            assert t.shape[0] == case["tm"][b].shape[1] == case["S"][b]
            assert float(t[:, Q:].abs().sum()) == 0.0
    for b in range(B):
        T = case["tm"][b].shape[0]
        assert T == case["T"][b] and 1 <= T <= min(32, Q) and case["labels"][b].numel() == T
        assert all(v == 253 or 0 <= v < C - 1 for v in case["labels"][b].tolist())
    o64, o32 = CC.oracle_run(case, torch.float64), CC.oracle_run(case, torch.float32)
    for o, dt in ((o64, torch.float64), (o32, torch.float32)):
        assert all(v.dtype == dt and bool(torch.isfinite(v)) for v in o["losses"].values())
        assert all(g.dtype == dt and bool(torch.isfinite(g).all()) for g in o["dlogits"])
        assert all(g.dtype == dt and bool(torch.isfinite(g).all()) for gs in o["dmasks"] for g in gs)
        assert all(bool(torch.isfinite(tb[k]).all()) for ts in o["terms"] for tb in ts for k in tb)
    # the yardstick err(o32, o64) is finite and not zero
    err = max(float((o32["terms"][l][b]["cost"].double() - o64["terms"][l][b]["cost"]).abs().max())
              for l in range(L) for b in range(B))
    assert 0.0 < err < float("inf")
    # the regime is what it claims
    regime = case["regime"]
    for l in range(L):
        for b in range(B):
            T, cm, cost = case["T"][b], o64["terms"][l][b]["cmask"], o64["terms"][l][b]["cost"]
            if regime == "confident":
                assert float(cm.diagonal()[:T].max()) < 1e-3, (l, b, float(cm.diagonal()[:T].max()))
                q, t = o64["own_indices"][l][b]
                assert float(cm[q, t].max()) < 1e-3                                # and those ARE the matched pairs
            if regime == "saturated":                                              # exp(-x) overflows float32 at x < -88.7
                x = case["masks"][l][b][:, :Q]
                assert float(x[:, :T].abs().min()) > 50.0 and float(x.max()) == 100.0 and float(x.min()) == -100.0
            if regime == "ties_zero":
                assert bool((cm == cm[0:1]).all())
            if regime == "ties_dup":
                assert torch.equal(cost[1::2], cost[0:2 * (Q // 2):2])
            if regime == "degenerate":
                assert int(case["tm"][b][0].sum()) == 0 and bool(case["tm"][b][1].all())
