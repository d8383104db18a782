"""The device set criterion with 129 .. 256 queries (csrc/criterion.hip: above 128 queries or table columns the
usc_criterion_* launches take a second group of 128 columns and crit_loss a 256-slot tree; SetCriterion is given
`device_max_queries` above 128, config `loss.device_max_queries`).

The yardsticks are the ones of the <= 128-query path and are imported, not restated: criterion_cases.make_case builds
the cases (criterion_queries_cases.py re-pads them to ld > 128), oracle/criterion_ref.py (and tests/droploss_ref.py
with DropLoss) is the float64 oracle, test_gpu_criterion_f64.device_entry_points drives the entry points as it stands,
and every bounded quantity goes through test_gpu_criterion_f64.Judge:  err(dev, o64) <= 4 err(o32, o64) + floor  with
that file's floors.  The per-case checks themselves are the functions of tests/test_gpu_criterion_wide.py, called on
the cases of this file.

No other floor is needed.  The one sum that is longer than on the <= 128-query path is the cross entropy of a level
(part num = sum_q w_q nll_q, part den = sum_q w_q): a fixed pairwise tree over 256 slots instead of 128.  All its terms
are >= 0 (w >= 0, nll >= 0), so every partial sum is at most the result, and a tree of depth log2(256) = 8 rounds a term
at most 8 times: |error| <= 8 * 2^-24 * result, which is the floor Judge already grants (FLOOR_ULPS = 8 ulps of the
value), before the 4 err(o32, o64) that torch's own float32 sum of the same 256 terms earns.  The float64 pair sum of
crit_loss still has at most 128 terms (T <= 128), and every other kernel sums over rows, per column, as before.

Exact, with no tolerance: a query's entries do not depend on the other queries (the outputs of a 200-query run are the
bits of a 128-query and a 72-query run), device_max_queries changes nothing up to 128 queries, the <= 128-query path
computes the bits recorded with the library from before the second column group (tests/golden/criterion_bits.json),
the assignment is scipy's on the device's own float32 cost matrix, unmatched / dropped / padding gradient columns are
+0, two runs give the same bits.

Shapes: the smallest that cross the group boundary.  Q in {129, 150, 160, 200, 255, 256}, ld = Q, the next multiple of
32 and 256, S in {31, 33, 609} around the 32-row chunk, T in {1, 17, 32, 33, 65, 128}, L in {1, 2, 13}."""
import ctypes
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import criterion_cases as CC
import criterion_queries_cases as QC
import test_gpu_criterion_f64 as F
import test_gpu_criterion_wide as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_bits.json")


# ---- 1. a query's entries do not depend on the other queries --------------------------------------------------------
@pytest.mark.parametrize("Q,ld,S,T,max_targets", [(200, 224, 33, 17, 32), (129, 129, 31, 1, 32), (256, 256, 33, 128, 128)])
def test_column_groups_are_a_run_on_their_queries_alone(device, Q, ld, S, T, max_targets):
    """cost / cmask / cdice / nmat / ssum / logp of a Q-query run: rows 0 .. 127 = a run on the first 128 table columns
    alone (Q = 128, ld = 128), rows 128 .. Q-1 = a run on those Q - 128 columns alone, bit for bit."""
    case = QC.make_shape("random", 2, Q, 3, 0.1, [(S, T)], 1 if T > 1 else 0, ld=ld)
    whole = F.device_entry_points(case, device, max_targets=max_targets)["scenes"][0]
    for lo, hi in ((0, 128), (128, Q)):
        assert T <= hi - lo
        part = F.device_entry_points(QC.columns(case, lo, hi), device, max_targets=max_targets)["scenes"][0]
        for k in ("cost", "cmask", "cdice", "nmat"):
            assert whole[k].shape == (2, Q, T) and part[k].shape == (2, hi - lo, T)
            assert F._bits(whole[k][:, lo:hi]) == F._bits(part[k]), (k, lo, hi)
        for k in ("ssum", "logp"):
            assert F._bits(whole[k][:, lo:hi]) == F._bits(part[k]), (k, lo, hi)


# ---- 2. the opt-in changes nothing up to 128 queries ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["04-random-L1-Q65-C3", "21-ties_dup-L13-Q127-C2", "10-confident-L13-Q128-C3"])
def test_device_max_queries_changes_nothing_up_to_128_queries(device, name):
    case = CC.make_case(F.IDS.index(name))
    assert case["Q"] <= 128 and case["ld"] <= 128
    runs = []
    for n in (128, 256):
        crit = F._criterion(case, device)
        assert crit.device_max_queries == 128
        crit.device_max_queries = n
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*torch-operator path.*")
            runs.append(F._forward_backward(crit, case, device))
        crit.check_lsap_status(wait=True)
    for k in ("losses", "indices", "dlogits", "dmasks"):
        assert F._same_bits(runs[0][k], runs[1][k]), k


# ---- 3. the narrow path computes the recorded bits ------------------------------------------------------------------
def _sha(x, h=None):
    top = h is None
    h = h or hashlib.sha256()
    if isinstance(x, dict):
        for k in sorted(x):
            h.update(k.encode())
            _sha(x[k], h)
    elif isinstance(x, (list, tuple)):
        h.update(str(len(x)).encode())
        for v in x:
            _sha(v, h)
    else:
        h.update(f"{tuple(x.shape)}{x.dtype}".encode())
        h.update(F._bits(x))
    return h.hexdigest() if top else None


def narrow_bits(device):
    """sha256 over shapes and bytes of everything device_entry_points returns (forward and backward) on two <= 128-query
    cases: Q = 100, ld = 128, L = 13, and the DropLoss case of tests/test_gpu_criterion_wide.py with 65 targets."""
    bits = {}
    case = CC.make_case(F.IDS.index("00-random-L13-Q100-C3"))
    assert (case["Q"], case["ld"], case["L"]) == (100, 128, 13)
    bits[case["name"]] = _sha(F.device_entry_points(case, device))
    shape, drop = W.WIDE_CASES[3]
    case = W._make(shape, drop)
    assert drop and 65 in case["T"] and case["Q"] <= 128
    bits[case["name"]] = _sha(F.device_entry_points(case, device, thresh=W.DROP_THRESH, max_targets=128))
    return bits


def test_narrow_path_computes_the_recorded_bits(device):
    """Up to 128 queries and columns the grid, the block size, the workspace layout and every summation order are what
    they were: the outputs hash to the values recorded with the library of the parent commit."""
    want = json.load(open(GOLDEN))
    assert narrow_bits(device) == want


# ---- 4. against the float64 oracle ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=range(len(QC.QUERY_CASES)), ids=QC.QUERY_IDS)
def entry(request, device):
    """The entry-point run of a case and both oracles under the device's assignment, once per case: the tuple the
    checks of tests/test_gpu_criterion_wide.py take, plus the case's max_targets and padding value."""
    case, max_targets, drop, pad = QC.make(QC.QUERY_CASES[request.param])
    assert case["Q"] > 128
    thresh = W.DROP_THRESH if drop else None
    run = F.device_entry_points(case, device, pad=pad, thresh=thresh, max_targets=max_targets)
    again = F.device_entry_points(case, device, pad=pad, thresh=thresh, max_targets=max_targets)
    forced = [[(sc["src"][l], sc["tid"][l]) for sc in run["scenes"]] for l in range(case["L"])]
    return (case, drop, run, W._oracle(case, torch.float32, forced, drop), W._oracle(case, torch.float64, forced, drop)), \
        again, max_targets


def test_entry_points_against_the_float64_oracle(device, entry):
    """Every check of the wide-targets file (bits, counts, scipy's assignment on the device's own cost matrix, target
    classes, cost terms, matched pairs, DropLoss counts and weights, parts, table, gradients, +0 in every unmatched,
    dropped and padding column below ld) on outputs that started poisoned, and: two runs give the same bits, a query of
    the second column group is matched."""
    wide_entry, again, _ = entry
    case, drop, run = wide_entry[:3]
    assert F._same_bits(run, again), "two runs of the same case differ in some bit"
    high = sum(int((sc["src"] >= 128).sum()) for sc in run["scenes"])
    print(f"  [{case['name']}] matched queries at index >= 128: {high}")
    assert high > 0
    if case["regime"] == "confident":                     # the planted pairs, across the boundary / on the last T queries
        for b, sc in enumerate(run["scenes"]):
            assert torch.equal(sc["src"], (case["roll"] + torch.arange(case["T"][b])).expand(case["L"], -1))
    for sc in run["scenes"]:
        assert sc["dmasks"].shape[2] == case["ld"] and not bool(torch.isnan(sc["dmasks"]).any())
    W.test_entry_points_against_the_float64_oracle(device, wide_entry)


def test_set_criterion_against_the_float64_oracle(device, entry, monkeypatch):
    """SetCriterion(device_max_queries=256) end to end, by the check of the wide-targets file: the device path (no
    warning, the host solver idle), the entry points' assignment and gradient bits, losses and gradients inside the
    bound, the assignment optimal in float64 to within 2 T eps."""
    wide_entry = entry[0]
    make = F._criterion

    def criterion(case, dev):
        crit = make(case, dev)
        crit.device_max_queries = 256
        return crit
    monkeypatch.setattr(F, "_criterion", criterion)
    # (SetCriterion reads the case's tables, whose padding is zero; where the entry-point run had NaN there, the check's
    #  comparison of the gradient bits with that run shows once more that the padding is never read)
    W.test_set_criterion_against_the_float64_oracle(device, wide_entry)


# ---- 5. the assignment shapes the criterion can now reach -----------------------------------------------------------
@pytest.mark.parametrize("P,nr,nc", [(5, 256, 128), (7, 150, 17), (6, 129, 128), (6, 255, 1), (5, 256, 32), (5, 128, 256),
                                     (7, 17, 150)])
def test_lsap_shapes_of_the_wide_criterion_equal_scipy(device, P, nr, nc):
    """[Q queries, T targets] up to 256 x 128 (solved from global memory: it does not fit the LDS staging) and 150 x 17
    (staged; lsap_kernel, because the wider side is above the register-resident 128 columns), both orientations; ties
    and +inf entries."""
    from unscene3d_amd import ops
    c = F._lsap_problems(P, nr, nc, seed=nr * 1000 + nc)
    row, col, status = ops.lsap_batch(c.to(device))
    row2, col2, status2 = ops.lsap_batch(c.to(device))
    assert F._same_bits([row, col, status], [row2, col2, status2])
    assert int(status.abs().sum()) == 0
    row, col = row.cpu().numpy(), col.cpu().numpy()
    for p in range(P):
        i, j = linear_sum_assignment(c[p].numpy())
        assert np.array_equal(row[p], i) and np.array_equal(col[p], j), p


# ---- 6. bounds ------------------------------------------------------------------------------------------------------
def _bound_calls(device, L, ld, S, Q, T, C, max_targets, ws_bytes=None):
    """(name -> a call of that function, the zeroed buffers the calls point into: large enough for every size used
    below, though nothing may launch)."""
    from unscene3d_amd._lib import lib
    z32 = torch.zeros(4 * L * 260 * 130 + 260 * 40, dtype=torch.float32, device=device)      # every float argument
    zi = torch.zeros(4 * 260 * 40, dtype=torch.int64, device=device)                          # every integer argument
    n = int(lib.usc_criterion_ws_bytes_q(L, S, min(max(T, 1), 128), 256)) if ws_bytes is None else ws_bytes
    ws = torch.zeros(n, dtype=torch.uint8, device=device)
    ptrs = (ctypes.c_void_p * L)(*[z32.data_ptr()] * L)
    f, i, m = z32.data_ptr(), zi.data_ptr(), max_targets
    return {
        "usc_criterion_costs": lambda: lib.usc_criterion_costs(
            ptrs, L, ld, S, Q, T, m, i, i, f, Q * C, C, C, i, 5.0, 2.0, 2.0, f, f, f, f, f, f, ws.data_ptr(), ws.numel(), None),
        "usc_criterion_drop_counts": lambda: lib.usc_criterion_drop_counts(ptrs, L, ld, S, Q, T, m, i, i, i, i, None),
        "usc_criterion_losses": lambda: lib.usc_criterion_losses(
            f, f, f, i, i, i, f, L, Q, T, m, C, C - 1, i, f, None, None, 0.0, None, None),
        "usc_criterion_backward": lambda: lib.usc_criterion_backward(
            ptrs, ptrs, L, ld, S, Q, T, m, i, i, i, i, f, f, f, i, f, f, f, C, Q * C, C, f, None, None),
    }, (z32, zi, ws)


@pytest.mark.parametrize("Q,ld,T", [(257, 257, 17), (256, 257, 17), (150, 149, 17), (40, 160, 41)])
def test_entry_points_reject_sizes_outside_their_bounds(device, Q, ld, T):
    """Q = 257, ld = 257, ld < Q and T > Q: an error code and a message that names the function, before anything is
    launched (the poisoned outputs stay untouched and the device has nothing to report)."""
    from unscene3d_amd._lib import last_error
    calls, (z32, zi, ws) = _bound_calls(device, 2, ld, 33, Q, T, 3, 128)
    if Q <= 256 and T <= Q:                                               # usc_criterion_losses takes no ld
        del calls["usc_criterion_losses"]
    for name, call in calls.items():
        assert call() != 0, name
        msg = last_error()
        assert name in msg and "1..128" in msg, (name, msg)
    torch.cuda.synchronize()
    assert not bool(z32.any()) and not bool(zi.any()) and not bool(ws.any())


def test_a_workspace_of_the_128_column_size_is_refused_at_150_queries(device):
    from unscene3d_amd._lib import last_error, lib
    L, S, Q, T = 2, 33, 150, 17
    small = int(lib.usc_criterion_ws_bytes(L, S, T))
    assert small < int(lib.usc_criterion_ws_bytes_q(L, S, T, Q))
    calls, (z32, zi, ws) = _bound_calls(device, L, 160, S, Q, T, 3, 32, ws_bytes=small)
    assert calls["usc_criterion_costs"]() != 0
    assert "usc_criterion_costs" in last_error()
    torch.cuda.synchronize()
    assert not bool(z32.any()) and not bool(ws.any())
    calls, _buffers = _bound_calls(device, L, 128, S, 100, T, 3, 32, ws_bytes=small)          # enough for 100 queries
    assert calls["usc_criterion_costs"]() == 0
    torch.cuda.synchronize()


# ---- 7. SetCriterion end to end at 150 queries ----------------------------------------------------------------------
def test_set_criterion_at_150_queries_with_and_without_the_opt_in(device):
    """Q = 150 in padded tables of ld = 160 that carry `_usc_padded` (what models.mask3d._mask_logits hands over).
    device_max_queries = 256: the device path, no operator-path warning.  The default: the warning, which names the
    setting, and the operator path; with the device's assignment imposed on it (`forced_indices`, the mechanism of
    match_all_levels) its losses and the device's both meet the Judge rule against the float64 oracle."""
    case = QC.make_shape("random", 13, 150, 3, 0.1, [(609, 17), (33, 5)], 1, ld=160)
    crit = F._criterion(case, device)
    crit.device_max_queries = 256
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")
        dev = F._forward_backward(crit, case, device)
    assert crit.last_indices[0][0][0].is_cuda
    crit.check_lsap_status(wait=True)
    assert max(int(s.max()) for lv in dev["indices"] for s, _ in lv) >= 128

    default = F._criterion(case, device)
    assert default.device_max_queries == 128
    with pytest.warns(UserWarning, match="torch-operator path") as rec:
        own = F._forward_backward(default, case, device)
    assert any("device_max_queries" in str(w.message) for w in rec)
    assert not default.last_indices[0][0][0].is_cuda

    forced = F._criterion(case, device)
    forced.forced_indices = dev["indices"]
    with pytest.warns(UserWarning, match="torch-operator path"):
        ops_run = F._forward_backward(forced, case, device)
    assert F._same_bits(ops_run["indices"], dev["indices"])
    o32 = CC.oracle_run(case, torch.float32, dev["indices"])
    o64 = CC.oracle_run(case, torch.float64, dev["indices"])
    for label, got in (("device", dev), ("operators, the device's assignment", ops_run)):
        J = F.Judge(case["regime"], f"{case['name']} {label}")
        assert sorted(got["losses"]) == sorted(o64["losses"])
        for k in got["losses"]:
            lvl = 0 if k[-1] not in "0123456789" else int(k.rsplit("_", 1)[1]) + 1
            J.check(k.rstrip("_0123456789"), got["losses"][k], o32["losses"][k], o64["losses"][k],
                    1.0 if "dice" in k else 0.0, k,
                    sum(float(m.abs().max()) for m in case["masks"][lvl]) if "mask" in k else 0.0)
        J.finish()
    # the operator path's own assignment is the same wherever float32 costs do not tie: not required, printed
    same = sum(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for la, lb in zip(own["indices"], dev["indices"])
               for a, b in zip(la, lb))
    print(f"  [{case['name']}] operator path's own assignment equals the device's in {same} of {13 * 2} problems")


# ---- 8. the model, short --------------------------------------------------------------------------------------------
def test_training_steps_at_150_queries_stay_on_the_device_criterion(device):
    """Two AdamW steps and eval_step of InstanceSegmentation at model.num_queries=150 with loss.device_max_queries=256:
    the criterion never leaves the device path (its warning is an error), in training and in the labelled validation
    step; losses are finite, the query projection has a gradient, no assignment problem was infeasible."""
    import test_gpu_eval_parity as EP
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-operator path.*")
        cfg, module, data, target, res, _ = EP._train_then_eval(device, 2, 6000, 5150,
                                                               ("model.num_queries=150", "loss.device_max_queries=256"))
    assert module.criterion.device_max_queries == 256 and cfg.model.num_queries == 150
    assert module.criterion.last_indices[0][0][0].is_cuda and len(module.criterion.last_indices) == 13
    assert res is not None and all(np.isfinite(v) for v in res["losses"].values())
    g = [p.grad for p in module.model.query_projection.parameters()]
    assert g and all(x is not None and bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in g)
    module.criterion.check_lsap_status(wait=True)
    assert all(int(s.abs().sum()) == 0 for s in module.criterion.last_lsap_status)
