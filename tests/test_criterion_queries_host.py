"""device_max_queries, the opt-in of the device set criterion for 129 .. 256 queries, on the host: the default, the
constructor's range check, the way from the config through the trainer, the workspace size for a query count, the
argument checks that need no device, and that every case of tests/criterion_queries_cases.py is what it claims to be
(as tests/test_criterion_oracle.py does for the <= 128-query cases).  What the setting does on the device is
tests/test_gpu_criterion_queries.py."""
import pytest
import torch

import criterion_cases as CC
import criterion_queries_cases as QC
from unscene3d_amd.config import apply_overrides, default_config


def _criterion(**kw):
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    matcher = HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, cost_noise_robust=0.0, num_points=-1)
    return SetCriterion(num_classes=3, matcher=matcher, weight_dict={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0},
                        eos_coef=0.1, losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                        importance_sample_ratio=0.75, class_weights=-1, **kw)


def test_the_default_is_128_queries():
    assert _criterion().device_max_queries == 128
    assert default_config().loss.device_max_queries == 128


@pytest.mark.parametrize("n", [128, 129, 150, 256])
def test_the_constructor_keeps_a_value_in_range(n):
    crit = _criterion(device_max_queries=n)
    assert crit.device_max_queries == n and crit.device_max_targets == 32


@pytest.mark.parametrize("n", [0, 127, 257, -1, 128.0, "150", None, True])
def test_the_constructor_rejects_everything_else(n):
    with pytest.raises(ValueError, match="device_max_queries"):
        _criterion(device_max_queries=n)


def test_the_trainer_hands_the_config_value_through():
    from unscene3d_amd.trainer.trainer import InstanceSegmentation
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "loss.device_max_queries=256"])
    assert InstanceSegmentation(cfg).criterion.device_max_queries == 256
    cfg = apply_overrides(default_config(), ["general.num_targets=3"])
    assert InstanceSegmentation(cfg).criterion.device_max_queries == 128
    del cfg.loss.device_max_queries                     # a config node written before the setting existed
    assert InstanceSegmentation(cfg).criterion.device_max_queries == 128
    with pytest.raises(ValueError, match="device_max_queries"):
        InstanceSegmentation(apply_overrides(default_config(), ["general.num_targets=3", "loss.device_max_queries=257"]))


@pytest.mark.parametrize("L,S,T", [(1, 1, 1), (13, 609, 17), (13, 3000, 32), (2, 33, 128)])
def test_the_workspace_size_for_a_query_count(L, S, T):
    """Up to 128 queries exactly the size it always was; above, the 256-column stride: twice that."""
    from unscene3d_amd._lib import lib
    old = lib.usc_criterion_ws_bytes(L, S, T)
    for Q in (1, 100, 128):
        assert lib.usc_criterion_ws_bytes_q(L, S, T, Q) == old
    for Q in (129, 256):
        wide = lib.usc_criterion_ws_bytes_q(L, S, T, Q)
        assert wide == 2 * old > old                    # a multiple of 128 columns * 4 bytes: no rounding in either


def test_the_entry_points_check_the_query_bounds_without_a_device():
    """Argument validation happens before any HIP call: Q = 257, ld = 257, ld < Q and T > Q are refused with a message
    that names the function; 256 queries pass the size check (and fail on the null pointers after it)."""
    from unscene3d_amd import _lib
    lib = _lib.lib
    for Q, ld, T in ((257, 257, 17), (256, 257, 17), (150, 149, 17), (40, 160, 41)):
        calls = {
            "usc_criterion_costs": lambda: lib.usc_criterion_costs(
                None, 2, ld, 33, Q, T, 128, None, None, None, Q * 3, 3, 3, None, 5.0, 2.0, 2.0, None, None, None, None, None,
                None, None, 0, None),
            "usc_criterion_drop_counts": lambda: lib.usc_criterion_drop_counts(None, 2, ld, 33, Q, T, 128, None, None, None,
                                                                               None, None),
            "usc_criterion_backward": lambda: lib.usc_criterion_backward(
                None, None, 2, ld, 33, Q, T, 128, None, None, None, None, None, None, None, None, None, None, None, 3, Q * 3,
                3, None, None, None),
        }
        if Q > 256 or T > Q:                                   # this one takes no ld
            calls["usc_criterion_losses"] = lambda: lib.usc_criterion_losses(
                None, None, None, None, None, None, None, 2, Q, T, 128, 3, 2, None, None, None, None, 0.0, None, None)
        for name, call in calls.items():
            assert call() != 0, (name, Q, ld, T)
            msg = _lib.last_error()
            assert name in msg and "256 queries" in msg and "1..128" in msg, (name, Q, ld, T, msg)
    assert lib.usc_criterion_costs(None, 2, 256, 33, 256, 17, 32, None, None, None, 768, 3, 3, None, 5.0, 2.0, 2.0, None, None,
                                   None, None, None, None, None, 0, None) != 0
    assert "bad argument" in _lib.last_error()


def test_case_list_covers_the_stated_domain():
    made = [QC.make(s) for s in QC.QUERY_CASES]
    cases = [m[0] for m in made]
    seen = lambda f: {v for c in cases for v in f(c)}                              # noqa: E731
    assert seen(lambda c: [c["Q"]]) == {129, 150, 160, 255, 256}
    assert seen(lambda c: c["S"]) == {31, 33, 609}
    assert seen(lambda c: c["T"]) == {1, 17, 32, 33, 65, 128}
    assert seen(lambda c: [c["L"]]) == {1, 13}
    assert seen(lambda c: [c["B"]]) == {1, 2, 3}
    assert seen(lambda c: [c["regime"]]) == {"random", "confident", "saturated", "ties_zero", "ties_dup", "degenerate"}
    kinds = seen(lambda c: ["Q" if c["ld"] == c["Q"] else "256" if c["ld"] == 256 and c["Q"] <= 224 else
                            "next32" if c["ld"] == -(-c["Q"] // 32) * 32 else "other"])
    assert kinds == {"Q", "next32", "256"}
    assert any(253 in lab.tolist() for c in cases for lab in c["labels"])
    assert sum(1 for m in made if m[2]) == len(made) // 2                          # DropLoss on half
    assert sum(1 for m in made if m[3] != m[3]) == 1                               # NaN padding in one case
    for case, max_targets, _, _ in made:
        assert max(case["T"]) <= max_targets and (max_targets == 128) == (max(case["T"]) > 32)
        if case["B"] > 1:
            assert len(set(zip(case["S"], case["T"]))) == case["B"]                # ragged
    last = [c for c in cases if c["regime"] == "confident" and c["roll"] == c["Q"] - c["T"][0]]
    assert last                                                                    # confident targets on the last T queries


@pytest.mark.parametrize("index", range(len(QC.QUERY_CASES)), ids=QC.QUERY_IDS)
def test_generated_case_meets_its_conditions(index):
    case, max_targets, drop, pad = QC.make(QC.QUERY_CASES[index])
    L, B, Q, C, ld, roll = case["L"], case["B"], case["Q"], case["C"], case["ld"], case["roll"]
    # every condition of SetCriterion._fused_tables under device_max_queries = 256 that is a property of the data
    assert 1 <= L <= 16 and 128 < Q <= 256 and len(case["logits"]) == L and len(case["masks"]) == L
    for l in range(L):
        assert case["logits"][l].shape == (B, Q, C) and case["logits"][l].dtype == torch.float32
        for b in range(B):
            t = case["masks"][l][b]
            assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and Q <= t.shape[1] == ld <= 256
            assert t.shape[0] == case["tm"][b].shape[1] == case["S"][b]
            assert float(t[:, Q:].abs().sum()) == 0.0
    for b in range(B):
        T = case["tm"][b].shape[0]
        assert T == case["T"][b] and 1 <= T <= min(max_targets, Q) and case["labels"][b].numel() == T
        assert all(v == 253 or 0 <= v < C - 1 for v in case["labels"][b].tolist())
    o64, o32 = CC.oracle_run(case, torch.float64), CC.oracle_run(case, torch.float32)
    for o, dt in ((o64, torch.float64), (o32, torch.float32)):
        assert all(v.dtype == dt and bool(torch.isfinite(v)) for v in o["losses"].values())
        assert all(g.dtype == dt and bool(torch.isfinite(g).all()) for g in o["dlogits"])
        assert all(g.dtype == dt and bool(torch.isfinite(g).all()) for gs in o["dmasks"] for g in gs)
        assert all(bool(torch.isfinite(tb[k]).all()) for ts in o["terms"] for tb in ts for k in tb)
    err = max(float((o32["terms"][l][b]["cost"].double() - o64["terms"][l][b]["cost"]).abs().max())
              for l in range(L) for b in range(B))
    assert 0.0 < err < float("inf")                                                # the yardstick is finite and not zero
    regime, high = case["regime"], 0
    for l in range(L):
        for b in range(B):
            T, cm, cost = case["T"][b], o64["terms"][l][b]["cmask"], o64["terms"][l][b]["cost"]
            q64, t64 = o64["own_indices"][l][b]
            high += int((q64 >= 128).sum())
            # the float32 and float64 oracle runs agree on the assignment wherever the float64 costs are not tied
            if regime not in ("ties_zero", "ties_dup"):
                q32, t32 = o32["own_indices"][l][b]
                assert torch.equal(q32, q64) and torch.equal(t32, t64), (l, b)
            if regime == "confident":
                pairs = cm[roll + torch.arange(T), torch.arange(T)]
                assert float(pairs.max()) < 1e-3, (l, b, float(pairs.max()))
                assert torch.equal(q64, roll + torch.arange(T)) and float(cm[q64, t64].max()) < 1e-3
            if regime == "saturated":                                              # exp(-x) overflows float32 at x < -88.7
                x = case["masks"][l][b][:, :Q]
                assert float(x[:, roll:roll + T].abs().min()) > 50.0 and float(x.max()) == 100.0 and float(x.min()) == -100.0
            if regime == "ties_zero":
                # all-zero mask logits: every query has the same mask cost.  The oracle's matrix product may add the S
                # equal terms of one row in another order than those of the next (255 rows are no multiple of a BLAS
                # row block), so its rows agree to the last bits of float64, not necessarily in all of them
                assert not bool(case["masks"][l][b].any())
                assert float((cm - cm[0:1]).abs().max()) <= 4 * 2.0 ** -52 * float(cm.abs().max())
            if regime == "ties_dup":                                               # exact ties, in both precisions
                x, lg = case["masks"][l][b][:, :Q], case["logits"][l][b]
                assert torch.equal(x[:, 1::2], x[:, 0:2 * (Q // 2):2]) and torch.equal(lg[1::2], lg[0:2 * (Q // 2):2])
                assert torch.equal(cost[1::2], cost[0:2 * (Q // 2):2])
                c32 = o32["terms"][l][b]["cost"]
                assert torch.equal(c32[1::2], c32[0:2 * (Q // 2):2])
            if regime == "degenerate":
                assert int(case["tm"][b][0].sum()) == 0 and bool(case["tm"][b][1].all())
    assert high > 0, "no query of the second column group is matched"
