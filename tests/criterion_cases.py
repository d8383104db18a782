"""Seeded cases for the set criterion (csrc/criterion.hip against oracle/criterion_ref.py in float64), shared by
tests/test_criterion_oracle.py (CPU: every case is what it claims to be) and tests/test_gpu_criterion_f64.py.

A case is (L, B, Q, C, ld, [S_b], [T_b], labels, target masks, mask logits, class logits, per-loss weights).  Every
number is generated in float32, so the device, the float32 oracle and the float64 oracle see identical inputs.

Regimes of the mask logits:
  random      randn * 3 (what every older criterion test uses)
  confident   query t carries (2 tm[t] - 1) * 10 + randn for t < T, the other queries randn * 3: the matched pairs of
              a trained model (BCE of the pair ~1e-4, where a difference of two large sums cancels)
  saturated   the same with +-60 and a few entries at +-100: expf(-x) overflows, softplus is its linear branch
  ties_zero   all-zero mask logits: every query has the same mask cost
  ties_dup    query 2k+1 is a bit-identical copy of query 2k (mask and class logits): exact cost ties
  degenerate  target 0 is empty, target 1 covers every row, the rest are ordinary
Class logits are randn * 2, with +-50 added to one entry of a few queries.

The shape list covers, between its cases: T in {1, 8, 9, 16, 17, 32}; S in {1, 31, 32, 33, 609, 3000}; Q in {32, 63,
64, 65, 100, 127, 128}; ld = Q, strictly between Q and 128, and 128; C in {2, 3, 19} with labels over all object
classes; the ignore label 253 (every target is matched, T <= Q, so a 253 target always is); eos_coef in {0.1, 1.0};
L in {1, 13, 16}; B in {1, 2, 3} with different (S, T) per scene.  The factors are independent, so the list is a
covering selection and not the product.
"""
import numpy as np
import torch

LOSS_NAMES = ("loss_ce", "loss_mask", "loss_dice", "loss_noise_robust")
MASK_TYPE = "segment_mask"
COST_WEIGHTS = dict(cost_class=2.0, cost_mask=5.0, cost_dice=2.0)        # the shipped matcher

# (regime, L, Q, C, ld kind, eos_coef, [(S, T) per scene], number of targets labelled 253 per scene)
_SHAPES = [
    ("random", 13, 100, 3, "128", 0.1, [(609, 17)], 0),
    ("random", 1, 32, 2, "Q", 1.0, [(1, 1), (31, 8)], 0),
    ("random", 16, 63, 19, "mid", 0.1, [(32, 9), (33, 16), (3000, 32)], 1),
    ("random", 13, 64, 19, "128", 1.0, [(3000, 32), (1, 1)], 2),
    ("random", 1, 65, 3, "mid", 0.1, [(33, 17)], 1),
    ("random", 16, 127, 2, "Q", 1.0, [(31, 1), (32, 8)], 0),
    ("random", 13, 128, 19, "128", 0.1, [(609, 9), (33, 32), (32, 16)], 1),
    ("confident", 13, 100, 3, "128", 0.1, [(609, 17), (3000, 25)], 0),
    ("confident", 1, 32, 19, "mid", 1.0, [(31, 32)], 1),
    ("confident", 16, 64, 2, "Q", 0.1, [(3000, 8), (609, 9)], 0),
    ("confident", 13, 128, 3, "128", 1.0, [(32, 16), (33, 17), (31, 1)], 1),
    ("confident", 1, 127, 19, "128", 0.1, [(3000, 32)], 2),
    ("confident", 16, 65, 3, "128", 1.0, [(609, 1), (3000, 16)], 0),
    ("saturated", 13, 63, 3, "Q", 1.0, [(609, 8), (33, 9)], 1),
    ("saturated", 1, 100, 19, "mid", 0.1, [(3000, 17), (32, 32), (31, 16)], 0),
    ("saturated", 16, 128, 2, "128", 0.1, [(33, 1)], 0),
    ("saturated", 13, 32, 19, "128", 0.1, [(3000, 9), (609, 32)], 1),
    ("ties_zero", 1, 64, 3, "mid", 1.0, [(32, 8), (1, 1)], 0),
    ("ties_zero", 13, 100, 19, "Q", 0.1, [(31, 17)], 1),
    ("ties_dup", 16, 65, 19, "Q", 0.1, [(609, 16), (31, 9)], 0),
    ("ties_dup", 1, 128, 3, "128", 1.0, [(33, 32), (3000, 8), (32, 17)], 1),
    ("ties_dup", 13, 127, 2, "128", 0.1, [(1, 9), (609, 1)], 0),
    ("degenerate", 13, 100, 3, "mid", 0.1, [(609, 8), (3000, 17)], 1),
    ("degenerate", 1, 63, 2, "128", 1.0, [(33, 9), (32, 16), (31, 32)], 0),
    ("degenerate", 16, 32, 3, "Q", 1.0, [(3000, 32)], 0),
]
# more than 32 targets: SetCriterion leaves the device path (and warns); the operator path meets the same bounds
FALLBACK_SHAPE = ("random", 13, 100, 3, "128", 0.1, [(609, 33), (300, 5)], 0)


def _ld(Q, kind):
    if kind == "128" or Q == 128:
        return 128
    if kind == "mid" and Q < 127:
        return Q + max(1, (128 - Q) // 2)
    return Q


def case_ids():
    return [f"{i:02d}-{s[0]}-L{s[1]}-Q{s[2]}-C{s[3]}" for i, s in enumerate(_SHAPES)]


def make_case(index=None, shape=None):
    """-> dict(name, regime, L, B, Q, C, ld, S, T, eos_coef, labels [B][T] i64, tm [B][T, S] bool,
    masks [L][B] f32 [S, ld] (columns >= Q are zero padding), logits [L] f32 [B, Q, C], weights {loss name: float})."""
    regime, L, Q, C, ldk, eos, st, n253 = _SHAPES[index] if shape is None else shape
    seed = 1000 + (index if index is not None else 999)
    g = torch.Generator().manual_seed(seed)
    B, ld = len(st), _ld(Q, ldk)
    nobj = C - 1
    labels, tms = [], []
    for b, (S, T) in enumerate(st):
        assert 1 <= T <= Q
        tm = torch.rand(T, S, generator=g) < 0.2
        tm[:, 0] = True
        if regime == "degenerate":
            tm[0] = False
            tm[1] = True
        lab = (torch.arange(T) + b) % nobj
        lab = lab[torch.randperm(T, generator=g)]
        for k in range(min(n253, T)):
            lab[(3 * k + b) % T] = 253
        labels.append(lab.to(torch.int64))
        tms.append(tm)
    amp = {"confident": 10.0, "saturated": 60.0}.get(regime)
    masks, logits = [], []
    for l in range(L):
        per_scene = []
        for b, (S, T) in enumerate(st):
            x = torch.randn(S, Q, generator=g) * 3
            if regime == "ties_zero":
                x.zero_()
            if amp is not None:
                sign = tms[b].T.to(torch.float32) * 2 - 1                          # [S, T]
                x[:, :T] = sign * amp + torch.randn(S, T, generator=g)
                if regime == "saturated":
                    n = min(6, S * Q)
                    pos = torch.randperm(S * Q, generator=g)[:n]
                    x.view(-1)[pos] = torch.tensor([100.0, -100.0] * 3)[:n]
            if regime == "ties_dup":
                x[:, 1::2] = x[:, 0:2 * (Q // 2):2]
            t = torch.zeros(S, ld)
            t[:, :Q] = x
            per_scene.append(t)
        masks.append(per_scene)
        lg = torch.randn(B, Q, C, generator=g) * 2
        for k in range(3):                                                         # a few saturated class logits
            q = int(torch.randint(Q, (1,), generator=g))
            lg[k % B, q, k % C] += 50.0 if k % 2 == 0 else -50.0
        if regime == "ties_dup":
            lg[:, 1::2] = lg[:, 0:2 * (Q // 2):2]
        logits.append(lg)
    # per-loss weights: distinct multiples of 1/8 (exact in float32), a few zeros; the reference's noise-robust term
    # is off, so its weight is 0 where SetCriterion looks at it and arbitrary elsewhere (the loss is the constant 0)
    perm = torch.randperm(4 * L, generator=g) + 1
    w = perm.to(torch.float32) / 8
    w[torch.randperm(4 * L, generator=g)[:max(1, L // 4)]] = 0.0
    weights = {}
    for l in range(L):
        for j, n in enumerate(LOSS_NAMES):
            weights[n + ("" if l == 0 else f"_{l - 1}")] = float(w[4 * l + j])
    weights["loss_noise_robust"] = 0.0
    name = case_ids()[index] if index is not None else "fallback-T33"
    return dict(name=name, regime=regime, L=L, B=B, Q=Q, C=C, ld=ld, S=[s for s, _ in st], T=[t for _, t in st],
                eos_coef=float(np.float32(eos)), labels=labels, tm=tms, masks=masks, logits=logits, weights=weights)


def oracle_inputs(case, dtype, requires_grad=False):
    """The case as the oracle's (outputs, targets): level 0 is the final prediction, levels 1.. the aux outputs."""
    levels = []
    for l in range(case["L"]):
        lg = case["logits"][l].to(dtype).requires_grad_(requires_grad)
        pm = [m[:, :case["Q"]].to(dtype).requires_grad_(requires_grad) for m in case["masks"][l]]
        levels.append({"pred_logits": lg, "pred_masks": pm})
    targets = [{"labels": case["labels"][b].clone(), MASK_TYPE: case["tm"][b].clone()} for b in range(case["B"])]
    outputs = dict(levels[0], aux_outputs=levels[1:])
    return outputs, targets, levels


def gtable(case):
    """The per-loss weights as the [L, 4] table the device criterion differentiates against."""
    w = case["weights"]
    return torch.tensor([[w[n + ("" if l == 0 else f"_{l - 1}")] for n in LOSS_NAMES] for l in range(case["L"])],
                        dtype=torch.float32)


def oracle_run(case, dtype, forced_indices=None):
    """oracle/criterion_ref.py on the case in `dtype` -> dict(terms [L][B] of cost_terms, indices [L][B] (the oracle's
    own, or the forced ones), losses {name: 0-d}, parts [L][B] [4], table [L, 4], den_tot [L], dlogits [L] [B, Q, C],
    dmasks [L][B] [S, Q]): losses, parts and gradients under `forced_indices` when given."""
    from scipy.optimize import linear_sum_assignment
    from oracle import criterion_ref as CR
    outputs, targets, levels = oracle_inputs(case, dtype, requires_grad=True)
    terms = [CR.cost_terms(lv, targets, MASK_TYPE, **COST_WEIGHTS) for lv in levels]
    own = [[tuple(torch.as_tensor(i, dtype=torch.int64) for i in linear_sum_assignment(tb["cost"])) for tb in ts]
           for ts in terms]                                                        # == CR.hungarian_match per level
    idx = forced_indices if forced_indices is not None else own
    losses = CR.set_criterion(outputs, targets, MASK_TYPE, num_classes=case["C"], eos_coef=case["eos_coef"],
                              forced_indices=idx, **COST_WEIGHTS)
    total = sum(losses[k] * case["weights"][k] for k in losses)
    total.backward()
    parts = [CR.loss_parts(lv, targets, [(s.long().cpu(), t.long().cpu()) for s, t in idx[l]], MASK_TYPE,
                           case["C"] - 1, case["eos_coef"]) for l, lv in enumerate(levels)]
    table = torch.stack([torch.stack([sum(p[0] for p in ps) / sum(p[1] for p in ps), sum(p[2] for p in ps),
                                      sum(p[3] for p in ps), torch.zeros((), dtype=dtype)]) for ps in parts])
    den_tot = torch.stack([sum(p[1] for p in ps) for ps in parts])
    zero = torch.zeros_like
    return dict(terms=terms, indices=idx, own_indices=own, losses={k: v.detach() for k, v in losses.items()},
                parts=parts, table=table, den_tot=den_tot,
                dlogits=[lv["pred_logits"].grad if lv["pred_logits"].grad is not None else zero(lv["pred_logits"])
                         for lv in levels],
                dmasks=[[m.grad if m.grad is not None else zero(m) for m in lv["pred_masks"]] for lv in levels])
