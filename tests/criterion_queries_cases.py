"""Cases for the device set criterion at 129 .. 256 queries (csrc/criterion.hip: the second group of 128 query columns;
SetCriterion(device_max_queries=N)), shared by tests/test_criterion_queries_host.py (CPU: every case is what it claims
to be) and tests/test_gpu_criterion_queries.py.

The generator is criterion_cases.make_case, not restated: a case is built with ld kind "Q" (criterion_cases._ld cannot
produce ld > 128) and its tables are then re-padded with zero columns to the case's own ld.  Two more steps, both on the
float32 inputs that the device and both oracles share:

  roll    the confident / saturated regimes put target t on query t, all of them below 128.  The query axis of the mask
          and class logits is rotated by `roll`, so the confident targets sit on the queries roll .. roll + T - 1: across
          the group boundary, or on the last T queries (roll = Q - T).
  pad     the value the entry-point run writes into the padding columns Q <= col < ld (zero, or NaN in one case).

The list covers, between its cases: Q in {129, 150, 160, 255, 256}; ld = Q, the next multiple of 32 and 256; S in
{31, 33, 609}; T in {1, 17, 32, 33, 65, 128}, above 32 with max_targets = 128; L in {1, 13}; up to 3 ragged scenes; all
six regimes; DropLoss on half; the label 253."""
import torch

import criterion_cases as CC

# (regime, L, Q, C, eos_coef, [(S, T) per scene], targets labelled 253 per scene), ld, max_targets, DropLoss, roll, pad
QUERY_CASES = [
    (("random", 13, 150, 3, 0.1, [(609, 17), (33, 32), (31, 1)], 1), 160, 32, False, 0, 0.0),
    (("confident", 1, 129, 19, 1.0, [(31, 1)], 0), 129, 32, True, 128, 0.0),
    (("confident", 13, 256, 3, 0.1, [(33, 128)], 0), 256, 128, False, 128, 0.0),          # the last T queries
    (("saturated", 1, 160, 2, 0.1, [(33, 33), (609, 65)], 1), 160, 128, True, 120, 0.0),
    (("ties_zero", 1, 255, 3, 1.0, [(33, 17)], 0), 256, 32, False, 0, 0.0),
    (("ties_dup", 13, 150, 19, 0.1, [(31, 32), (33, 17)], 0), 256, 32, True, 0, float("nan")),
    (("degenerate", 1, 256, 3, 1.0, [(609, 65), (31, 33)], 1), 256, 128, True, 0, 0.0),
    (("random", 1, 255, 2, 1.0, [(33, 128)], 0), 255, 128, False, 0, 0.0),
]


def case_id(spec):
    (regime, L, Q, C, _, st, _), ld, _, drop, roll, pad = spec
    return (f"{regime}-L{L}-Q{Q}-ld{ld}-C{C}-T{'_'.join(str(t) for _, t in st)}" + ("-drop" if drop else "")
            + (f"-roll{roll}" if roll else "") + ("-nanpad" if pad != pad else ""))


QUERY_IDS = [case_id(s) for s in QUERY_CASES]


def repad(case, ld):
    """The case with its [S, Q] tables zero-extended to [S, ld]."""
    Q = case["Q"]
    assert case["ld"] == Q <= ld
    masks = []
    for per_scene in case["masks"]:
        out = []
        for t in per_scene:
            p = torch.zeros(t.shape[0], ld)
            p[:, :Q] = t
            out.append(p)
        masks.append(out)
    return dict(case, ld=ld, masks=masks)


def make_shape(regime, L, Q, C, eos, st, n253, ld=None, roll=0, name=None):
    """criterion_cases.make_case at Q queries (ld kind "Q"), rotated by `roll` queries and re-padded to ld columns."""
    case = CC.make_case(shape=(regime, L, Q, C, "Q", eos, st, n253))
    if roll:
        case["masks"] = [[torch.roll(t, roll, dims=1).contiguous() for t in ts] for ts in case["masks"]]
        case["logits"] = [torch.roll(lg, roll, dims=1).contiguous() for lg in case["logits"]]
    case = repad(case, Q if ld is None else ld)
    case["name"] = name or f"{regime}-L{L}-Q{Q}-ld{case['ld']}"
    return case


def make(spec):
    """-> (case, max_targets, DropLoss, pad) of one QUERY_CASES entry; case["roll"] is where the regime's first target
    sits."""
    shape, ld, max_targets, drop, roll, pad = spec
    case = make_shape(*shape, ld=ld, roll=roll, name=case_id(spec))
    case["roll"] = roll
    return case, max_targets, drop, pad


def columns(case, lo, hi, ld=None):
    """The case restricted to the queries lo .. hi-1 (tables of hi - lo columns, or ld with zero padding): what the
    same targets cost against those queries alone."""
    Q = hi - lo
    masks = [[t[:, lo:hi].contiguous() for t in ts] for ts in case["masks"]]
    logits = [lg[:, lo:hi].contiguous() for lg in case["logits"]]
    sub = dict(case, Q=Q, ld=Q, masks=masks, logits=logits)
    return repad(sub, Q if ld is None else ld)
