"""The device set criterion (csrc/criterion.hip: usc_criterion_* and usc_lsap_batch, driven by criterion_device.py
under models/criterion.py::_FusedCriterion) against oracle/criterion_ref.py in float64, over tests/criterion_cases.py.

The bound is relative to the reference's own float32 arithmetic, not a constant: with
    dev = the device, o32 = the oracle in float32 on the CPU, o64 = the oracle in float64, all on the same inputs,
every compared quantity has to meet
    err(dev, o64) <= 4 * err(o32, o64) + floor,      floor = 8 * 2^-24 * (largest intermediate of the reference's formula)
4x = two bits: the kernels add up to 3000 terms in 32-row chunks where torch uses blocked / pairwise sums, which may
cost a small constant factor and not an order of magnitude.  The intermediate is 1 for the dice terms (the reference
forms 1 - ratio as well), the value's own magnitude for BCE / CE / logp, the array's max-abs for matrices; the floor
keeps the ratio of two one-ulp errors from deciding a test.  Scalars (losses, part, table) are compared one by one
(|a - b| <= ... is the relative form multiplied by |o64|), arrays by max-abs; the matched-pair entries of cmask / cdice
are also compared on their own, because in the confident regimes they are orders of magnitude below the unmatched
entries.  Assignments are never compared across precisions: the solver is checked exactly against scipy on the device's
own float32 cost matrix, and end to end the device's assignment has to be optimal in float64 to within 2 T eps,
eps = max |cost_dev - cost_f64| of that problem (each of the two assignments has T entries, each within eps).

One term is added to the floor of the BCE quantities, because the float64 yardstick is not exact either: the reference's
BCE is torch's `(1 - y) x + max(-x, 0) + log1p(exp(-|x|))`, which forms +-|x| and cancels it, so each float64 term
carries an absolute error of up to an ulp of |x| in float64 (at x = -60, y = 0 the term is e^-60 = 8.8e-27 and both
oracle precisions return exactly 0: measured on the saturated cases, device 1.44e-26 = the directly evaluated
softplus, float64 oracle 3e-27).  So those quantities get + 8 * 2^-53 * max |mask logit| (8.9e-14 at |x| = 100), the same
8 ulps at the yardstick's own precision; it is 1e-9 of the matched-pair BCE of the confident regime and decides
nothing there.

Every test prints its figures (`pytest -s`); test_report_worst_ratios prints the worst err(dev, o64) / err(o32, o64)
per regime and quantity, the numbers quoted in DESIGN.md section 3.10.
"""
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import criterion_cases as CC

pytestmark = pytest.mark.gpu

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
MARGIN, FLOOR_ULPS = 4.0, 8.0
WORST = {}                       # (regime, quantity) -> [worst err_dev / err_32, worst err_dev / bound]
IDS = CC.case_ids()


def _np64(x):
    return x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


class Judge:
    """Collects err(dev, o64) <= 4 err(o32, o64) + floor over the quantities of one test; prints every figure."""

    def __init__(self, regime, label):
        self.regime, self.label, self.failures, self.seen = regime, label, [], {}

    def check(self, name, dev, o32, o64, intermediate=0.0, where="", yardstick=0.0):
        dev, o32, o64 = _np64(dev), _np64(o32), _np64(o64)
        assert dev.shape == o32.shape == o64.shape, (name, dev.shape, o32.shape, o64.shape)
        if dev.size == 0:
            return
        if not np.isfinite(dev).all():
            self.failures.append(f"{name} {where}: non-finite device value")
            return
        e_dev, e_32 = float(np.abs(dev - o64).max()), float(np.abs(o32 - o64).max())
        floor = FLOOR_ULPS * (EPS32 * max(float(np.abs(o64).max()), intermediate) + EPS64 * yardstick)
        bound = MARGIN * e_32 + floor
        ratio = e_dev / e_32 if e_32 > 0 else (0.0 if e_dev == 0 else float("inf"))
        used = e_dev / bound if bound > 0 else (0.0 if e_dev == 0 else float("inf"))
        w = WORST.setdefault((self.regime, name), [0.0, 0.0])
        if e_dev > floor:                   # a ratio of two errors below the floor says nothing
            w[0] = max(w[0], ratio)
        w[1] = max(w[1], used)
        s = self.seen.setdefault(name, [0.0, 0.0, 0.0, 0.0])
        if used >= s[3]:
            s[:] = [e_dev, e_32, floor, used]
        if not e_dev <= bound:
            self.failures.append(f"{name} {where}: err(dev,o64) {e_dev:.3e} > 4 * err(o32,o64) {e_32:.3e} + floor "
                                 f"{floor:.3e} (ratio {ratio:.2f})")

    def finish(self):
        for name, (e_dev, e_32, floor, used) in self.seen.items():
            print(f"  [{self.label}] {name:14s} worst: err(dev,o64) {e_dev:.3e}  err(o32,o64) {e_32:.3e}  floor "
                  f"{floor:.3e}  fraction of the bound {used:.3f}")
        assert not self.failures, "\n".join([f"{len(self.failures)} quantities outside the bound"] + self.failures[:40])


def _bits(a):
    return a.detach().cpu().contiguous().numpy().tobytes()


def _same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    return _bits(a) == _bits(b)


# ---- the entry-point layer ------------------------------------------------------------------------------------------
_POISON = {torch.float32: float("nan"), torch.int32: -1, torch.uint8: 0xFF}          # 0xFF bytes: NaN as float32


def device_entry_points(case, dev, pad=0.0, thresh=None, max_targets=32):
    """criterion_device.scene_forward -> table -> scene_backward, the functions _FusedCriterion.forward / backward call,
    every intermediate kept (CPU tensors).  thresh: the DropLoss threshold (None: no DropLoss, no `counts` / `wts`).
    Outputs and the workspace start out as NaN / -1, so an element a kernel does not write shows.  pad: the value of the
    table columns Q <= col < ld.  max_targets: handed to scene_forward / scene_backward."""
    from unscene3d_amd import criterion_device as D
    L, B, Q, NC = case["L"], case["B"], case["Q"], case["C"]

    def poisoned(shape, dtype):
        return torch.full(shape, _POISON[dtype], dtype=dtype, device=dev)
    logits = torch.stack(case["logits"]).to(dev).contiguous()                                   # [L, B, Q, C]
    class_w = torch.ones(NC, dtype=torch.float32)
    class_w[-1] = case["eos_coef"]
    class_w = class_w.to(dev)
    g = CC.gtable(case).to(dev).reshape(-1).contiguous()
    weights = tuple(CC.COST_WEIGHTS[k] for k in ("cost_mask", "cost_class", "cost_dice"))
    parts = poisoned((B, L, 4), torch.float32)
    tabs, states = [], []
    for b in range(B):
        tabs.append([])
        for l in range(L):
            t = case["masks"][l][b].clone()
            t[:, Q:] = pad
            tabs[b].append(t.to(dev).contiguous())
        tm8 = case["tm"][b].to(dev).contiguous().view(torch.uint8)
        labels = case["labels"][b].to(dev).contiguous()
        states.append(D.scene_forward(tabs[b], tm8, labels, logits, b, weights, class_w, NC - 1, parts[b], thresh,
                                      alloc=poisoned, max_targets=max_targets))
    table, den_tot = D.table(parts, alloc=poisoned)
    dlogits = poisoned((L, B, Q, NC), torch.float32)
    scenes = []
    for b, st in enumerate(states):
        assert (st.S, st.T, st.ld) == (case["S"][b], case["T"][b], case["ld"])
        sc = {k: v for k, v in st._asdict().items() if torch.is_tensor(v)}
        sc["dmasks"] = D.scene_backward(st, tabs[b], b, class_w, g, den_tot, dlogits, alloc=poisoned,
                                        max_targets=max_targets)
        scenes.append(sc)
    torch.cuda.synchronize()
    return dict(scenes=[{k: v.cpu() for k, v in sc.items()} for sc in scenes], parts=parts.cpu(), table=table.cpu(),
                den_tot=den_tot.cpu(), dlogits=dlogits.cpu())


@pytest.fixture(scope="module", params=range(len(IDS)), ids=IDS)
def entry(request, device):
    """The entry-point run of a case and both oracles under the device's assignment, computed once per case (a
    module-scoped parametrised fixture: pytest runs the tests of one case back to back)."""
    case = CC.make_case(request.param)
    run = device_entry_points(case, device)
    forced = [[(sc["src"][l], sc["tid"][l]) for sc in run["scenes"]] for l in range(case["L"])]
    return case, run, CC.oracle_run(case, torch.float32, forced), CC.oracle_run(case, torch.float64, forced)


def test_entry_points_against_the_float64_oracle(device, entry):
    case, run, o32, o64 = entry
    L, B, Q, NC, ld = case["L"], case["B"], case["Q"], case["C"], case["ld"]
    assert _same_bits(run, device_entry_points(case, device)), "two runs of the same case differ in some bit"
    J = Judge(case["regime"], case["name"])
    for b, sc in enumerate(run["scenes"]):
        S, T = case["S"][b], case["T"][b]
        tm = case["tm"][b].numpy()
        want_bits = (tm.astype(np.uint64) << np.arange(T, dtype=np.uint64)[:, None]).sum(0).astype(np.uint32)
        assert np.array_equal(sc["bits"].numpy().view(np.uint32), want_bits)
        assert np.array_equal(sc["cnt"].numpy(), tm.sum(1).astype(np.int32))
        assert int(sc["status"].abs().sum()) == 0
        labels = case["labels"][b].numpy()
        for l in range(L):
            where = f"level {l} scene {b}"
            # the solver alone: exactly scipy's answer on the device's own float32 cost matrix, ties included
            q, t = linear_sum_assignment(sc["cost"][l].numpy())
            src, tid = sc["src"][l].numpy(), sc["tid"][l].numpy()
            assert np.array_equal(src, q) and np.array_equal(tid, t), where
            want_tcls = np.full(Q, NC - 1, dtype=np.int32)
            want_tcls[src] = labels[tid]
            assert np.array_equal(sc["tcls"][l].numpy(), want_tcls), where
            t32, t64 = o32["terms"][l][b], o64["terms"][l][b]
            xmax = float(case["masks"][l][b].abs().max())            # the float64 BCE's own intermediate (docstring)
            for name, inter, ys in (("cmask", 0.0, xmax), ("cdice", 1.0, 0.0), ("nmat", 0.0, 0.0), ("ssum", 0.0, 0.0),
                                    ("logp", 0.0, 0.0), ("cost", 0.0, CC.COST_WEIGHTS["cost_mask"] * xmax)):
                J.check(name, sc[name][l], t32[name], t64[name], inter, where, ys)
            J.check("cmask matched", sc["cmask"][l][src, tid], t32["cmask"][src, tid], t64["cmask"][src, tid], 0.0, where, xmax)
            J.check("cdice matched", sc["cdice"][l][src, tid], t32["cdice"][src, tid], t64["cdice"][src, tid], 1.0, where)
            for j, (name, inter) in enumerate((("part num", 0.0), ("part den", 0.0), ("part mask", 0.0), ("part dice", 1.0))):
                J.check(name, run["parts"][b, l, j], o32["parts"][l][b][j], o64["parts"][l][b][j], inter, where,
                        xmax if j == 2 else 0.0)
            # gradients of the mask logits: float64 autograd under the device's assignment; exact zeros elsewhere
            dm = sc["dmasks"][l]
            J.check("dmasks", dm[:, :Q], o32["dmasks"][l][b], o64["dmasks"][l][b], 0.0, where)
            unmatched = np.setdiff1d(np.arange(ld), src)
            z = dm[:, unmatched].numpy()
            assert z.size == 0 or (np.abs(z).max() == 0.0 and not np.isnan(z).any()), where
    for l in range(L):
        for j, (name, inter) in enumerate((("table ce", 0.0), ("table mask", 0.0), ("table dice", 1.0))):
            J.check(name, run["table"][l, j], o32["table"][l, j], o64["table"][l, j], inter, f"level {l}",
                    sum(float(m.abs().max()) for m in case["masks"][l]) if j == 1 else 0.0)
        assert float(run["table"][l, 3]) == 0.0
        J.check("den_tot", run["den_tot"][l], o32["den_tot"][l], o64["den_tot"][l], 0.0, f"level {l}")
        J.check("dlogits", run["dlogits"][l], o32["dlogits"][l], o64["dlogits"][l], 0.0, f"level {l}")
    J.finish()


def test_padding_columns_are_never_read(device):
    """The table columns Q <= col < ld belong to nobody: zero or NaN there, every output has the same bits."""
    case = CC.make_case(IDS.index("22-degenerate-L13-Q100-C3"))
    assert case["Q"] < case["ld"]
    a = device_entry_points(case, device, pad=0.0)
    b = device_entry_points(case, device, pad=float("nan"))
    assert _same_bits(a, b)
    for sc in b["scenes"]:
        assert float(sc["dmasks"][:, :, case["Q"]:].abs().max()) == 0.0


# ---- end to end through SetCriterion --------------------------------------------------------------------------------
def _criterion(case, dev):
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    matcher = HungarianMatcher(cost_noise_robust=0.0, num_points=-1, **CC.COST_WEIGHTS)
    return SetCriterion(num_classes=case["C"], matcher=matcher, weight_dict=dict(case["weights"]),
                        eos_coef=case["eos_coef"], losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                        importance_sample_ratio=0.75, class_weights=-1).to(dev)


def _forward_backward(crit, case, dev):
    Q = case["Q"]
    logits = [lg.to(dev).requires_grad_(True) for lg in case["logits"]]
    tables = [[t.to(dev).requires_grad_(True) for t in ts] for ts in case["masks"]]

    def view(t):
        v = t[:, :Q]
        if t.shape[1] > Q:
            v._usc_padded = t
        return v
    levels = [{"pred_logits": lg, "pred_masks": [view(t) for t in ts]} for lg, ts in zip(logits, tables)]
    targets = [{"labels": case["labels"][b].to(dev), CC.MASK_TYPE: case["tm"][b].to(dev)} for b in range(case["B"])]
    losses = crit(dict(levels[0], aux_outputs=levels[1:]), targets, mask_type=CC.MASK_TYPE)
    total = sum(v * case["weights"][k] for k, v in losses.items())
    total.backward()
    zero = torch.zeros_like
    return dict(losses={k: v.detach().cpu() for k, v in losses.items()},
                dlogits=[(lg.grad if lg.grad is not None else zero(lg)).cpu() for lg in logits],
                dmasks=[[(t.grad if t.grad is not None else zero(t)).cpu() for t in ts] for ts in tables],
                indices=[[(s.cpu(), t.cpu()) for s, t in lv] for lv in crit.last_indices])


def _judge_end_to_end(J, case, got, o32, o64, cost_dev):
    L, B, Q = case["L"], case["B"], case["Q"]
    assert sorted(got["losses"]) == sorted(o64["losses"]) and len(got["losses"]) == 4 * L
    for k in got["losses"]:
        lvl = 0 if k[-1] not in "0123456789" else int(k.rsplit("_", 1)[1]) + 1
        J.check(k.rstrip("_0123456789"), got["losses"][k], o32["losses"][k], o64["losses"][k],
                1.0 if "dice" in k else 0.0, k,
                sum(float(m.abs().max()) for m in case["masks"][lvl]) if "mask" in k else 0.0)
    for l in range(L):
        J.check("dlogits", got["dlogits"][l], o32["dlogits"][l], o64["dlogits"][l], 0.0, f"level {l}")
        for b in range(B):
            where = f"level {l} scene {b}"
            dm = got["dmasks"][l][b]
            J.check("dmasks", dm[:, :Q], o32["dmasks"][l][b], o64["dmasks"][l][b], 0.0, where)
            src, tid = got["indices"][l][b][0].numpy(), got["indices"][l][b][1].numpy()
            z = dm[:, np.setdiff1d(np.arange(dm.shape[1]), src)].numpy()
            assert z.size == 0 or np.abs(z).max() == 0.0, where
            # the assignment is optimal in float64 to within 2 T eps, eps = max |cost_dev - cost_f64| of this problem
            c64 = o64["terms"][l][b]["cost"].numpy()
            eps = float(np.abs(cost_dev[l][b].astype(np.float64) - c64).max())
            T = case["T"][b]
            assert len(src) == T and len(set(src.tolist())) == T and sorted(tid.tolist()) == list(range(T)), where
            qo, to = linear_sum_assignment(c64)
            excess = float(c64[src, tid].sum() - c64[qo, to].sum())
            print(f"  [{case['name']}] {where}: eps {eps:.3e}  float64 cost above the optimum {excess:.3e}  "
                  f"allowed {2 * T * eps:.3e}")
            assert np.isfinite(eps) and excess <= 2 * T * eps, (where, excess, eps)


def test_set_criterion_against_the_float64_oracle(device, entry):
    case, run, o32, o64 = entry
    crit = _criterion(case, device)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")       # leaving the device path fails
        got = _forward_backward(crit, case, device)
    assert hasattr(crit, "last_indices") and crit.last_indices[0][0][0].is_cuda        # the device path really ran
    crit.check_lsap_status(wait=True)
    assert _same_bits(got, _forward_backward(crit, case, device)), "two runs of the same case differ in some bit"
    # the same kernels as the entry-point layer: the same assignment, which is the one both oracles were given
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert torch.equal(got["indices"][l][b][0], run["scenes"][b]["src"][l])
            assert torch.equal(got["indices"][l][b][1], run["scenes"][b]["tid"][l])
    J = Judge(case["regime"], case["name"] + " e2e")
    cost_dev = [[run["scenes"][b]["cost"][l].numpy() for b in range(case["B"])] for l in range(case["L"])]
    _judge_end_to_end(J, case, got, o32, o64, cost_dev)
    J.finish()


def test_more_than_32_targets_take_the_operator_path(device):
    """T = 33: SetCriterion leaves the device kernels, says so once, and its operator path meets the same bounds."""
    case = CC.make_case(shape=CC.FALLBACK_SHAPE)
    crit = _criterion(case, device)
    seen = []
    solve = crit.matcher.solve

    def spy(c_cpu):                                                 # the cost matrices the product solved
        seen.append(c_cpu.clone().numpy())
        return solve(c_cpu)
    crit.matcher.solve = spy
    with pytest.warns(UserWarning, match="torch-operator path"):
        got = _forward_backward(crit, case, device)
    L, B = case["L"], case["B"]
    assert len(seen) == L * B
    cost_dev = [[seen[l * B + b] for b in range(B)] for l in range(L)]
    forced = got["indices"]
    o32, o64 = CC.oracle_run(case, torch.float32, forced), CC.oracle_run(case, torch.float64, forced)
    J = Judge("fallback", case["name"])
    for l in range(L):
        for b in range(B):
            J.check("cost", cost_dev[l][b], o32["terms"][l][b]["cost"], o64["terms"][l][b]["cost"], 0.0, f"level {l} scene {b}",
                    CC.COST_WEIGHTS["cost_mask"] * float(case["masks"][l][b].abs().max()))
    _judge_end_to_end(J, case, got, o32, o64, cost_dev)
    J.finish()


# ---- the solver on its own ------------------------------------------------------------------------------------------
def _lsap_problems(P, nr, nc, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(P, nr, nc, generator=g)
    k = P // 3
    c[:k] = torch.randint(0, 4, (k, nr, nc), generator=g).float()                  # small integers: exact ties
    inf = torch.rand(P - 2 * k, nr, nc, generator=g) < 0.3                          # +inf entries; i -> i stays finite
    d = torch.arange(min(nr, nc))
    inf[:, d, d] = False
    c[2 * k:][inf] = float("inf")
    return c


@pytest.mark.parametrize("P,nr,nc", [(7, 128, 32), (7, 127, 32), (6, 128, 128), (7, 129, 5), (7, 5, 129), (6, 120, 125),
                                     (402, 100, 17)])
def test_lsap_batch_equals_scipy(device, P, nr, nc):
    """Both kernels, both orientations, the register-resident limit of 128 columns and one past it; 120 x 125 does
    not fit the 60 KB LDS budget staged and is solved from global memory; ties and +inf entries; a large batch."""
    from unscene3d_amd import ops
    c = _lsap_problems(P, nr, nc, seed=nr * 1000 + nc)
    row, col, status = ops.lsap_batch(c.to(device))
    row2, col2, status2 = ops.lsap_batch(c.to(device))
    assert _same_bits([row, col, status], [row2, col2, status2])
    assert int(status.abs().sum()) == 0
    row, col = row.cpu().numpy(), col.cpu().numpy()
    for p in range(P):
        i, j = linear_sum_assignment(c[p].numpy())
        assert np.array_equal(row[p], i) and np.array_equal(col[p], j), p


def test_report_worst_ratios():
    """Not a check: prints the worst err(dev, o64) / err(o32, o64) per regime and quantity seen by the tests above
    (only where the device error is above the floor), and the largest fraction of the bound that was used."""
    print()
    for (regime, name), (ratio, used) in sorted(WORST.items()):
        print(f"  worst {regime:10s} {name:14s} err(dev,o64)/err(o32,o64) {ratio:8.3f}   fraction of the bound {used:.3f}")
