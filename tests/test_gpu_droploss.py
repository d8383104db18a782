"""DropLoss inside the device set criterion (csrc/criterion.hip: usc_criterion_drop_counts and the DropLoss arguments of
usc_criterion_losses and usc_criterion_backward, driven by criterion_device.py under models/criterion.py::_FusedCriterion when `use_droploss`
is set) against the weighted float64 restatement of tests/droploss_ref.py, which tests/test_droploss_host.py pins on the
reference's golden.

Cases: droploss_ref.GPU_CASES, a covering selection of criterion_cases._SHAPES (S in {1, 31, 32, 33, 609}, T in {1, 8,
9, 16, 17, 32}, Q in {32, 63, 100, 128}, ld = Q / between / 128, L in {1, 13, 16}, B up to 3, every regime; the
degenerate case carries a pair with U = 0, droploss_ref.make_case).  Thresholds per case: 0.1, 0.01 and the float32 I / U
of one matched pair of level 0 — a tie, which `>=` keeps.

Exact: the counts I and F (an integer torch restatement under the device's own assignment), the weights (the float32
rule, bit for bit), the columns of dropped pairs (bitwise zero), `part` of the mask and dice losses (the kernel's own
sums restated: float64 / float32 accumulation of the stored pair terms in pair order, dropped pairs left out).  Bounded:
parts, table, losses and gradients by test_gpu_criterion_f64's  err(dev, o64) <= 4 err(o32, o64) + floor  with the same
floors, both oracles being the weighted restatement under the device's assignment.
"""
import warnings

import numpy as np
import pytest
import torch

import criterion_cases as CC
import droploss_ref as DR
import test_gpu_criterion_f64 as F64

pytestmark = pytest.mark.gpu

IDS = [CC.case_ids()[i] for i in DR.GPU_CASES]
KINDS = ("0.1", "0.01", "tie")


def entry_points(case, dev, thresh, pad=0.0):
    """test_gpu_criterion_f64.device_entry_points with a DropLoss threshold (the argument order the tests below use)."""
    return F64.device_entry_points(case, dev, pad, thresh)


def _indices(run, case):
    return [[(sc["src"][l], sc["tid"][l]) for sc in run["scenes"]] for l in range(case["L"])]


@pytest.fixture(scope="module", params=DR.GPU_CASES, ids=IDS)
def base(request, device):
    """Per case: the case, today's entry points (no DropLoss) and the three thresholds (the tie from the device's own
    level-0 assignment).  The assignment does not see the weights, so it is the same in every run of the case."""
    case = DR.make_case(request.param)
    plain = F64.device_entry_points(case, device)
    forced = _indices(plain, case)
    _, counts = DR.weights_of(case, forced, 0.1)
    from oracle import criterion_ref as CR
    DR._fresh_leaves(case)
    _, targets, levels = CC.oracle_inputs(case, torch.float64)
    plain["terms64"] = [CR.cost_terms(lv, targets, CC.MASK_TYPE, **CC.COST_WEIGHTS) for lv in levels]
    return case, plain, forced, {"0.1": 0.1, "0.01": 0.01, "tie": DR.tie_threshold(counts)}


@pytest.fixture(scope="module", params=KINDS)
def entry(request, device, base):
    case, plain, forced, thr = base
    thresh = thr[request.param]
    run = entry_points(case, device, thresh)
    return (case, plain, forced, thresh, run, DR.weighted_run(case, torch.float32, forced, thresh),
            DR.weighted_run(case, torch.float64, forced, thresh))


def _part_restated(cmask, cdice, src, tid, w, T):
    """crit_loss_kernel's own sums on the stored pair terms: float64 / float32 accumulation in pair order."""
    lm, ld = np.float64(0.0), np.float32(0.0)
    for p in range(T):
        if w[p] != 0:
            lm += np.float64(cmask[src[p], tid[p]])
            ld = np.float32(ld + cdice[src[p], tid[p]])
    return np.float32(lm / np.float64(T)), np.float32(ld / np.float32(T))


def test_entry_points(device, entry):
    case, plain, forced, thresh, run, o32, o64 = entry
    L, B, Q, ld = case["L"], case["B"], case["Q"], case["ld"]
    assert F64._same_bits(run, entry_points(case, device, thresh)), "two runs of the same case differ in some bit"
    J = F64.Judge(case["regime"], f"{case['name']} thresh {thresh:.6g}")
    kept = dropped = 0
    for b, sc in enumerate(run["scenes"]):
        S, T = case["S"][b], case["T"][b]
        # everything before the counts is today's: the same bits as the entry points without DropLoss
        for k in ("bits", "cnt", "cost", "cmask", "cdice", "nmat", "ssum", "logp", "src", "tid", "status", "tcls"):
            assert F64._same_bits(sc[k], plain["scenes"][b][k]), k
        assert int(sc["status"].abs().sum()) == 0
        xmax = max(float(case["masks"][l][b].abs().max()) for l in range(L))
        for l in range(L):
            where = f"level {l} scene {b}"
            src, tid = sc["src"][l].numpy(), sc["tid"][l].numpy()
            inter, fgn, uni = o64["counts"][l][b]
            assert np.array_equal(sc["counts"][0, l].numpy(), inter.numpy().astype(np.int32)), where
            assert np.array_equal(sc["counts"][1, l].numpy(), fgn.numpy().astype(np.int32)), where
            w = o64["wts"][l][b].numpy()
            assert F64._bits(sc["wts"][l]) == w.tobytes(), (where, sc["wts"][l], w, inter, uni)
            kept, dropped = kept + int(w.sum()), dropped + int((w == 0).sum())
            lm, ldice = _part_restated(sc["cmask"][l].numpy(), sc["cdice"][l].numpy(), src, tid, w, T)
            assert run["parts"][b, l, 2].numpy().tobytes() == lm.tobytes(), where
            assert run["parts"][b, l, 3].numpy().tobytes() == ldice.tobytes(), where
            assert F64._same_bits(run["parts"][b, l, :2], plain["parts"][b, l, :2]), where     # loss_ce: no weights
            for j, (name, inter_) in enumerate((("part num", 0.0), ("part den", 0.0), ("part mask", 0.0), ("part dice", 1.0))):
                J.check(name, run["parts"][b, l, j], o32["parts"][l][b][j], o64["parts"][l][b][j], inter_, where,
                        xmax if j == 2 else 0.0)
            dm = sc["dmasks"][l]
            J.check("dmasks", dm[:, :Q], o32["dmasks"][l][b], o64["dmasks"][l][b], 0.0, where)
            zero_cols = np.concatenate([np.setdiff1d(np.arange(ld), src), src[w == 0]])
            z = dm[:, zero_cols].numpy()
            assert z.size == 0 or not z.view(np.uint32).any(), f"{where}: a dropped / unmatched column is not +0"
            # a kept column is today's gradient, bit for bit
            assert F64._same_bits(dm[:, src[w != 0]], plain["scenes"][b]["dmasks"][l][:, src[w != 0]]), where
    for l in range(L):
        for j, (name, inter_) in enumerate((("table ce", 0.0), ("table mask", 0.0), ("table dice", 1.0))):
            J.check(name, run["table"][l, j], o32["table"][l, j], o64["table"][l, j], inter_, f"level {l}",
                    sum(float(m.abs().max()) for m in case["masks"][l]) if j == 1 else 0.0)
        assert float(run["table"][l, 3]) == 0.0
    assert F64._same_bits(run["dlogits"], plain["dlogits"]) and F64._same_bits(run["den_tot"], plain["den_tot"])
    print(f"  [{case['name']}] thresh {thresh:.6g}: {kept} pairs kept, {dropped} dropped")
    if case["regime"] == "ties_zero" and thresh > 0:     # nothing is foreground: every pair dropped, exact zeros
        assert kept == 0 and not run["parts"][:, :, 2:].numpy().view(np.uint32).any()
        assert not run["table"][:, 1:3].numpy().view(np.uint32).any()
        assert all(not sc["dmasks"].numpy().view(np.uint32).any() for sc in run["scenes"])
    if case["regime"] == "degenerate":
        assert all(int(o64["counts"][l][b][2].min()) == 0 for l in range(L) for b in range(B)), "the U = 0 pair"
    J.finish()


def _criterion(case, dev, drop, thresh=0.1):
    crit = F64._criterion(case, dev)
    crit.use_droploss, crit.droploss_iou_thresh = drop, thresh
    return crit


def test_set_criterion(device, entry):
    case, plain, forced, thresh, run, o32, o64 = entry
    crit = _criterion(case, device, True, thresh)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")       # leaving the device path fails
        got = F64._forward_backward(crit, case, device)
    assert crit.last_indices[0][0][0].is_cuda and crit.last_drop_weights[0][0].is_cuda
    crit.check_lsap_status(wait=True)
    assert F64._same_bits(got, F64._forward_backward(crit, case, device)), "two runs differ in some bit"
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert torch.equal(got["indices"][l][b][0], forced[l][b][0]) and torch.equal(got["indices"][l][b][1], forced[l][b][1])
            assert F64._bits(crit.last_drop_weights[l][b]) == o64["wts"][l][b].numpy().tobytes()
            assert F64._same_bits(got["dmasks"][l][b], run["scenes"][b]["dmasks"][l])      # the entry points' bits
    assert F64._bits(torch.stack([got["losses"][k] for k in got["losses"]])) == F64._bits(run["table"].reshape(-1))
    J = F64.Judge(case["regime"], f"{case['name']} thresh {thresh:.6g} e2e")
    cost_dev = [[plain["scenes"][b]["cost"][l].numpy() for b in range(case["B"])] for l in range(case["L"])]
    F64._judge_end_to_end(J, case, got, o32, dict(o64, terms=plain["terms64"]), cost_dev)
    J.finish()


def test_without_droploss_nothing_changes(device, base):
    """use_droploss=False: the loss vector and the gradients are the bits of today's entry points."""
    case, plain, forced, _ = base
    crit = _criterion(case, device, False)
    got = F64._forward_backward(crit, case, device)
    assert crit.last_drop_weights is None
    assert F64._bits(torch.stack([got["losses"][k] for k in got["losses"]])) == F64._bits(plain["table"].reshape(-1))
    for l in range(case["L"]):
        assert F64._same_bits(got["dlogits"][l], plain["dlogits"][l])
        for b in range(case["B"]):
            assert F64._same_bits(got["dmasks"][l][b], plain["scenes"][b]["dmasks"][l])


def test_padding_columns_are_never_read(device):
    case = DR.make_case(DR.GPU_CASES[-1])
    assert case["Q"] < case["ld"] and case["regime"] == "degenerate"
    a = entry_points(case, device, 0.1, pad=0.0)
    b = entry_points(case, device, 0.1, pad=float("nan"))
    c = entry_points(case, device, 0.1, pad=7.0)              # foreground, were it read
    assert F64._same_bits(a, b) and F64._same_bits(a, c)


def test_threshold_zero_drops_only_the_pair_without_union(device):
    """thresh = 0: I / U >= 0 holds for every pair with U > 0, so the result differs from the criterion without DropLoss
    only through the U = 0 pair (the empty target of the degenerate case, one per level and scene)."""
    case = DR.make_case(DR.GPU_CASES[-1])
    plain = F64.device_entry_points(case, device)
    run = entry_points(case, device, 0.0)
    for b, sc in enumerate(run["scenes"]):
        T = case["T"][b]
        for l in range(case["L"]):
            src, tid = sc["src"][l].numpy(), sc["tid"][l].numpy()
            inter, fgn = sc["counts"][0, l].numpy(), sc["counts"][1, l].numpy()
            uni = fgn + sc["cnt"].numpy()[tid] - inter
            w = sc["wts"][l].numpy()
            assert np.array_equal(w, (uni > 0).astype(np.float32)) and int((w == 0).sum()) == 1 and tid[w == 0][0] == 0
            lm, ldice = _part_restated(sc["cmask"][l].numpy(), sc["cdice"][l].numpy(), src, tid, w, T)
            assert run["parts"][b, l, 2].numpy().tobytes() == lm.tobytes()
            assert run["parts"][b, l, 3].numpy().tobytes() == ldice.tobytes()
            q0 = src[w == 0]
            other = np.setdiff1d(np.arange(case["ld"]), q0)
            assert F64._same_bits(sc["dmasks"][l][:, other], plain["scenes"][b]["dmasks"][l][:, other])
            assert not sc["dmasks"][l][:, q0].numpy().view(np.uint32).any()
            assert plain["scenes"][b]["dmasks"][l][:, q0].abs().max() > 0
    assert F64._same_bits(run["dlogits"], plain["dlogits"])
    assert F64._same_bits(run["table"][:, 0], plain["table"][:, 0])


def test_33_targets_with_droploss_take_the_operator_path(device):
    """T = 33 with DropLoss: the operator path (with its warning).  On the 32-target sub-case the device applies, and the
    operator path under the device's assignment gives the same weights, bit for bit."""
    case = CC.make_case(shape=CC.FALLBACK_SHAPE)
    crit = _criterion(case, device, True)
    with pytest.warns(UserWarning, match="torch-operator path"):
        got = F64._forward_backward(crit, case, device)
    want, _ = DR.weights_of(case, got["indices"], 0.1)
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert torch.equal(crit.last_drop_weights[l][b].cpu(), want[l][b])
    assert all(bool(torch.isfinite(v)) for v in got["losses"].values())
    sub = dict(case, T=[32, case["T"][1]], tm=[case["tm"][0][:32], case["tm"][1]],
               labels=[case["labels"][0][:32], case["labels"][1]])
    # a threshold that splits the sub-case's pairs (at 0.1 every pair of these random logits is kept): the float32 I / U
    # of one of them, under the assignment of the device, which does not depend on the threshold
    dev_crit = _criterion(sub, device, True)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")
        dgot = F64._forward_backward(dev_crit, sub, device)
        tie = DR.tie_threshold(DR.weights_of(sub, dgot["indices"], 0.1)[1])
        dev_crit.droploss_iou_thresh = tie
        again = F64._forward_backward(dev_crit, sub, device)
    assert F64._same_bits(again["indices"], dgot["indices"])
    host_crit = _criterion(sub, torch.device("cpu"), True, tie)
    host_crit.forced_indices = dgot["indices"]
    outputs, targets, _ = CC.oracle_inputs(sub, torch.float32)
    host_crit(outputs, targets, mask_type=CC.MASK_TYPE)
    flat = []
    for l in range(sub["L"]):
        for b in range(sub["B"]):
            assert torch.equal(dev_crit.last_drop_weights[l][b].cpu(), host_crit.last_drop_weights[l][b])
            flat.append(host_crit.last_drop_weights[l][b])
    flat = torch.cat(flat)
    assert float(flat.min()) == 0.0 and float(flat.max()) == 1.0            # the comparison saw both kinds


def test_training_step_with_droploss(device):
    """One step of the product's training step on the small synthetic scenes of test_gpu_step_parity with
    loss.use_droploss=True: the device criterion runs (no operator-path warning), the loss is finite, parameters move."""
    from test_gpu_step_parity import _setup
    cfg, batch, collate, module = _setup(device, False, overrides=["loss.use_droploss=True"])
    assert module.criterion.use_droploss
    opt = torch.optim.SGD(module.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in module.named_parameters()}
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")
        total, losses = module.training_step(collate(batch))
    total.backward()
    opt.step()
    assert bool(torch.isfinite(total)) and all(bool(torch.isfinite(v)) for v in losses.values())
    w = module.criterion.last_drop_weights
    assert w is not None and w[0][0].is_cuda and set(torch.cat([x for lv in w for x in lv]).tolist()) <= {0.0, 1.0}
    changed = sum(int(not torch.equal(before[n], p.detach())) for n, p in module.named_parameters())
    assert changed > 100, changed
