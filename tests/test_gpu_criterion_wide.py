"""The device set criterion with 33 .. 128 targets per scene (csrc/criterion.hip: the usc_criterion_* functions with
`max_targets` above 32, which criterion_device.py passes when SetCriterion is given `device_max_targets` above 32).

The yardsticks are the ones of the <= 32-target path and are imported, not restated: criterion_cases.make_case builds the
cases, oracle/criterion_ref.py (and tests/droploss_ref.py with DropLoss) is the float64 oracle, and every bounded
quantity goes through test_gpu_criterion_f64.Judge:  err(dev, o64) <= 4 err(o32, o64) + floor  with that file's floors.
The wide path adds no longer sum than the <= 128-term float64 pair sum of crit_loss, so the rule is used as it stands.

Exact, with no tolerance: a pair's cost entries do not depend on the other targets (the outputs under max_targets = 128
are the bits of a max_targets = 32 run on each 32-target word alone), device_max_targets changes nothing up to 32
targets, the assignment is scipy's on the device's own float32 cost matrix, unmatched / dropped / padding gradient
columns are +0.

Shapes: word boundaries T in {33, 64, 65, 96, 97, 128} with a partial last word, the 32-row chunk S in {31, 33, 609},
Q in {64, 100, 128} with ld = Q and 128, L in {1, 13}, up to three ragged scenes with a <= 32-target scene next to a wide
one.  T = Q = 128 is the one assignment shape that does not fit the solver's LDS staging and runs from global memory.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import criterion_cases as CC
import droploss_ref as DR
import test_gpu_criterion_f64 as F

pytestmark = pytest.mark.gpu

DROP_THRESH = 0.1                      # the shipped droploss_iou_thresh

# (regime, L, Q, C, ld kind, eos_coef, [(S, T) per scene], targets labelled 253 per scene), DropLoss
WIDE_CASES = [
    (("random", 13, 100, 3, "128", 0.1, [(609, 64), (33, 17)], 1), False),
    (("random", 1, 64, 19, "Q", 1.0, [(31, 33)], 0), True),
    (("confident", 13, 128, 3, "128", 0.1, [(33, 128)], 0), False),
    (("confident", 1, 100, 19, "128", 1.0, [(609, 65), (31, 96), (33, 8)], 2), True),
    (("saturated", 1, 128, 2, "Q", 0.1, [(33, 97)], 0), False),
    (("saturated", 13, 64, 3, "128", 1.0, [(31, 64)], 1), True),
    (("ties_zero", 1, 100, 3, "Q", 0.1, [(33, 65)], 0), False),
    (("ties_dup", 13, 128, 19, "128", 0.1, [(609, 96), (31, 33)], 0), False),
    (("ties_dup", 1, 64, 2, "Q", 1.0, [(33, 64)], 0), True),
    (("degenerate", 13, 100, 3, "128", 0.1, [(33, 97), (609, 32)], 1), False),
    (("degenerate", 1, 128, 19, "128", 1.0, [(31, 128)], 0), True),
]


def _case_id(shape, drop):
    regime, L, Q, C, ldk, _, st, _ = shape
    return f"{regime}-L{L}-Q{Q}-ld{ldk}-T{'_'.join(str(t) for _, t in st)}" + ("-drop" if drop else "")


WIDE_IDS = [_case_id(s, d) for s, d in WIDE_CASES]


def _make(shape, drop=False):
    case = CC.make_case(shape=shape)
    case["name"] = _case_id(shape, drop)
    return case


def _sub_case(case, lo, hi):
    """Scene 0 of a one-scene case with only its targets lo .. hi-1."""
    return dict(case, T=[hi - lo], tm=[case["tm"][0][lo:hi]], labels=[case["labels"][0][lo:hi]])


def _want_bits(tm):
    """bool [T, S] -> u32 [W, S], word-major."""
    T, S = tm.shape
    W = (T + 31) // 32
    out = np.zeros((W, S), dtype=np.uint32)
    for t in range(T):
        out[t // 32] |= tm[t].astype(np.uint32) << np.uint32(t % 32)
    return out


# ---- 1. a pair's entries do not depend on the other targets ---------------------------------------------------------
@pytest.mark.parametrize("Q,T", [(64, 40), (128, 65)])
def test_words_are_a_32_target_run_on_32_targets_each(device, Q, T):
    """cost / cmask / cdice / nmat of a max_targets = 128 run, columns 32w .. 32w+31 = a max_targets = 32 run on those
    targets alone (the last word as a problem of T - 32w targets), bit for bit; ssum and logp are that run's too."""
    case = _make(("random", 2, Q, 3, "Q", 0.1, [(33, T)], 1))
    wide = F.device_entry_points(case, device, max_targets=128)["scenes"][0]
    assert wide["bits"].shape == ((T + 31) // 32, 33)
    assert np.array_equal(wide["bits"].numpy().view(np.uint32), _want_bits(case["tm"][0].numpy()))
    assert np.array_equal(wide["cnt"].numpy(), case["tm"][0].numpy().sum(1).astype(np.int32))
    for lo in range(0, T, 32):
        hi = min(lo + 32, T)
        sub = _sub_case(case, lo, hi)
        assert hi - lo <= 32 and hi - lo <= Q
        old = F.device_entry_points(sub, device, max_targets=32)["scenes"][0]
        for k in ("cost", "cmask", "cdice", "nmat"):
            assert wide[k].shape == (2, Q, T)
            assert F._bits(wide[k][:, :, lo:hi]) == F._bits(old[k]), (k, lo, hi)
        for k in ("ssum", "logp"):
            assert F._bits(wide[k]) == F._bits(old[k]), (k, lo, hi)
        assert F._bits(wide["cnt"][lo:hi]) == F._bits(old["cnt"])
        assert F._bits(wide["bits"][lo // 32]) == F._bits(old["bits"])


# ---- 2. the opt-in changes nothing up to 32 targets -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["04-random-L1-Q65-C3", "21-ties_dup-L13-Q127-C2", "23-degenerate-L1-Q63-C2"])
def test_device_max_targets_changes_nothing_up_to_32_targets(device, name):
    case = CC.make_case(F.IDS.index(name))
    assert max(case["T"]) <= 32
    runs = []
    for n in (32, 128):
        crit = F._criterion(case, device)
        assert crit.device_max_targets == 32
        crit.device_max_targets = n
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*torch-operator path.*")
            runs.append(F._forward_backward(crit, case, device))
        crit.check_lsap_status(wait=True)
    for k in ("losses", "indices", "dlogits", "dmasks"):
        assert F._same_bits(runs[0][k], runs[1][k]), k


# ---- 3. against the float64 oracle ----------------------------------------------------------------------------------
def _terms(case, dtype):
    from oracle import criterion_ref as CR
    DR._fresh_leaves(case)
    _, targets, levels = CC.oracle_inputs(case, dtype)
    return [CR.cost_terms(lv, targets, CC.MASK_TYPE, **CC.COST_WEIGHTS) for lv in levels]


def _oracle(case, dtype, forced, drop):
    DR._fresh_leaves(case)
    if drop:
        return dict(DR.weighted_run(case, dtype, forced, DROP_THRESH), terms=_terms(case, dtype))
    return CC.oracle_run(case, dtype, forced)


@pytest.fixture(scope="module", params=range(len(WIDE_CASES)), ids=WIDE_IDS)
def entry(request, device):
    """The entry-point run of a wide case and both oracles under the device's assignment, once per case."""
    shape, drop = WIDE_CASES[request.param]
    case = _make(shape, drop)
    assert max(case["T"]) > 32
    run = F.device_entry_points(case, device, thresh=DROP_THRESH if drop else None, max_targets=128)
    forced = [[(sc["src"][l], sc["tid"][l]) for sc in run["scenes"]] for l in range(case["L"])]
    return case, drop, run, _oracle(case, torch.float32, forced, drop), _oracle(case, torch.float64, forced, drop)


def test_entry_points_against_the_float64_oracle(device, entry):
    case, drop, run, o32, o64 = entry
    L, B, Q, NC, ld = case["L"], case["B"], case["Q"], case["C"], case["ld"]
    J = F.Judge(case["regime"], case["name"])
    for b, sc in enumerate(run["scenes"]):
        S, T = case["S"][b], case["T"][b]
        tm = case["tm"][b].numpy()
        want = _want_bits(tm)
        assert np.array_equal(sc["bits"].numpy().view(np.uint32), want if T > 32 else want[0])
        assert np.array_equal(sc["cnt"].numpy(), tm.sum(1).astype(np.int32))
        assert int(sc["status"].abs().sum()) == 0
        labels = case["labels"][b].numpy()
        for l in range(L):
            where = f"level {l} scene {b}"
            # the solver: exactly scipy's answer on the device's own float32 cost matrix, ties included
            q, t = linear_sum_assignment(sc["cost"][l].numpy())
            src, tid = sc["src"][l].numpy(), sc["tid"][l].numpy()
            assert np.array_equal(src, q) and np.array_equal(tid, t), where
            want_tcls = np.full(Q, NC - 1, dtype=np.int32)
            want_tcls[src] = labels[tid]
            assert np.array_equal(sc["tcls"][l].numpy(), want_tcls), where
            t32, t64 = o32["terms"][l][b], o64["terms"][l][b]
            xmax = float(case["masks"][l][b].abs().max())
            for name, inter, ys in (("cmask", 0.0, xmax), ("cdice", 1.0, 0.0), ("nmat", 0.0, 0.0), ("ssum", 0.0, 0.0),
                                    ("logp", 0.0, 0.0), ("cost", 0.0, CC.COST_WEIGHTS["cost_mask"] * xmax)):
                J.check(name, sc[name][l], t32[name], t64[name], inter, where, ys)
            J.check("cmask matched", sc["cmask"][l][src, tid], t32["cmask"][src, tid], t64["cmask"][src, tid], 0.0, where, xmax)
            J.check("cdice matched", sc["cdice"][l][src, tid], t32["cdice"][src, tid], t64["cdice"][src, tid], 1.0, where)
            if drop:                                                  # counts and weights: integers, exact
                inter, fgn, _ = o64["counts"][l][b]
                assert np.array_equal(sc["counts"][0, l].numpy(), inter.numpy().astype(np.int32)), where
                assert np.array_equal(sc["counts"][1, l].numpy(), fgn.numpy().astype(np.int32)), where
                w = o64["wts"][l][b].numpy()
                assert F._bits(sc["wts"][l]) == w.tobytes(), where
            else:
                w = np.ones(T, dtype=np.float32)
            for j, (name, inter) in enumerate((("part num", 0.0), ("part den", 0.0), ("part mask", 0.0), ("part dice", 1.0))):
                J.check(name, run["parts"][b, l, j], o32["parts"][l][b][j], o64["parts"][l][b][j], inter, where,
                        xmax if j == 2 else 0.0)
            dm = sc["dmasks"][l]
            J.check("dmasks", dm[:, :Q], o32["dmasks"][l][b], o64["dmasks"][l][b], 0.0, where)
            zero_cols = np.concatenate([np.setdiff1d(np.arange(ld), src), src[w == 0]])
            z = np.ascontiguousarray(dm[:, zero_cols].numpy())
            assert z.size == 0 or not z.view(np.uint32).any(), f"{where}: an unmatched / dropped / padding column is not +0"
    for l in range(L):
        for j, (name, inter) in enumerate((("table ce", 0.0), ("table mask", 0.0), ("table dice", 1.0))):
            J.check(name, run["table"][l, j], o32["table"][l, j], o64["table"][l, j], inter, f"level {l}",
                    sum(float(m.abs().max()) for m in case["masks"][l]) if j == 1 else 0.0)
        assert float(run["table"][l, 3]) == 0.0
        J.check("den_tot", run["den_tot"][l], o32["den_tot"][l], o64["den_tot"][l], 0.0, f"level {l}")
        J.check("dlogits", run["dlogits"][l], o32["dlogits"][l], o64["dlogits"][l], 0.0, f"level {l}")
    J.finish()


def test_set_criterion_against_the_float64_oracle(device, entry):
    """SetCriterion(device_max_targets=128) end to end: the device path (no warning, matcher.solve never called), the
    entry points' assignment, and the losses and gradients inside the bound."""
    case, drop, run, o32, o64 = entry
    crit = F._criterion(case, device)
    crit.device_max_targets = 128
    crit.use_droploss, crit.droploss_iou_thresh = drop, DROP_THRESH
    solved = []
    solve = crit.matcher.solve

    def spy(c_cpu):                                                 # the host solver: must stay idle
        solved.append(tuple(c_cpu.shape))
        return solve(c_cpu)
    crit.matcher.solve = spy
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*SetCriterion.*")              # leaving the device path fails
        got = F._forward_backward(crit, case, device)
    assert not solved, solved
    assert crit.last_indices[0][0][0].is_cuda
    crit.check_lsap_status(wait=True)
    assert all(int(s.abs().sum()) == 0 for s in crit.last_lsap_status)
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert torch.equal(got["indices"][l][b][0], run["scenes"][b]["src"][l])
            assert torch.equal(got["indices"][l][b][1], run["scenes"][b]["tid"][l])
            assert F._same_bits(got["dmasks"][l][b], run["scenes"][b]["dmasks"][l])          # the entry points' bits
            if drop:
                assert F._bits(crit.last_drop_weights[l][b]) == o64["wts"][l][b].numpy().tobytes()
    assert F._bits(torch.stack([got["losses"][k] for k in got["losses"]])) == F._bits(run["table"].reshape(-1))
    J = F.Judge(case["regime"], case["name"] + " e2e")
    cost_dev = [[run["scenes"][b]["cost"][l].numpy() for b in range(case["B"])] for l in range(case["L"])]
    F._judge_end_to_end(J, case, got, o32, o64, cost_dev)
    J.finish()


def test_the_default_still_takes_the_operator_path(device):
    """Without the opt-in a 64-target scene is not the device path's: the warning names the setting."""
    case = _make(("random", 1, 64, 3, "Q", 0.1, [(31, 64)], 0))
    crit = F._criterion(case, device)
    with pytest.warns(UserWarning, match="device_max_targets"):
        F._forward_backward(crit, case, device)
    assert not crit.last_indices[0][0][0].is_cuda


# ---- 4. exact zeros, padding never read -----------------------------------------------------------------------------
def test_unmatched_dropped_and_padding_columns_are_exact_zeros(device):
    case = _make(("random", 2, 100, 3, "128", 0.1, [(33, 97)], 1), True)
    Q, ld = case["Q"], case["ld"]
    assert Q < ld
    a = F.device_entry_points(case, device, pad=0.0, thresh=DROP_THRESH, max_targets=128)
    b = F.device_entry_points(case, device, pad=float("nan"), thresh=DROP_THRESH, max_targets=128)
    c = F.device_entry_points(case, device, pad=7.0, thresh=DROP_THRESH, max_targets=128)     # foreground, were it read
    assert F._same_bits(a, b) and F._same_bits(a, c)
    sc = b["scenes"][0]
    kept = dropped = 0
    for l in range(case["L"]):
        src, w = sc["src"][l].numpy(), sc["wts"][l].numpy()
        kept, dropped = kept + int((w == 1).sum()), dropped + int((w == 0).sum())
        dm = sc["dmasks"][l].numpy()
        zero_cols = np.concatenate([np.setdiff1d(np.arange(Q), src), src[w == 0], np.arange(Q, ld)])
        assert len(zero_cols) == ld - int((w == 1).sum())
        assert not np.ascontiguousarray(dm[:, zero_cols]).view(np.uint32).any(), l
        assert np.abs(dm[:, src[w == 1]]).max(0).min() > 0, l               # a kept column has a gradient
    print(f"  [{case['name']}] {kept} pairs kept, {dropped} dropped")
    assert kept > 0 and dropped > 0, "the case is meant to have both kinds of pair"
    # without DropLoss: unmatched and padding columns
    p = F.device_entry_points(case, device, pad=float("nan"), max_targets=128)["scenes"][0]
    for l in range(case["L"]):
        zero_cols = np.setdiff1d(np.arange(ld), p["src"][l].numpy())
        assert not np.ascontiguousarray(p["dmasks"][l].numpy()[:, zero_cols]).view(np.uint32).any(), l


# ---- 5. the assignment shapes the criterion can now reach -----------------------------------------------------------
@pytest.mark.parametrize("nr,nc", [(128, 128), (100, 100), (100, 64), (128, 33), (65, 64)])
def test_lsap_shapes_of_the_wide_criterion_equal_scipy(device, nr, nc):
    """[Q queries, T targets] up to 128 x 128 (which is solved from global memory: it does not fit the LDS staging);
    the four matrix kinds of test_gpu_parity.test_device_lsap_equals_scipy_including_ties."""
    from unscene3d_amd import ops
    rng = np.random.default_rng(1000 * nr + nc)
    mats = [rng.standard_normal((nr, nc)), rng.integers(0, 3, (nr, nc)), np.zeros((nr, nc)),
            rng.integers(0, 6, (nr, nc)) * 0.25 + (rng.random((nr, 1)) < 0.3)]
    mats = [c.astype(np.float32) for c in mats]
    cost = torch.from_numpy(np.stack(mats)).to(device)
    row, col, status = ops.lsap_batch(cost)
    assert int(status.abs().sum()) == 0
    row, col = row.cpu().numpy(), col.cpu().numpy()
    for k, c in enumerate(mats):
        a, b = linear_sum_assignment(c)
        assert np.array_equal(row[k], a) and np.array_equal(col[k], b), (nr, nc, k)


# ---- 6. bounds ------------------------------------------------------------------------------------------------------
def _bound_calls(device, L, S, Q, T, C, max_targets):
    """(name -> a call of that function, the zeroed buffers the calls point into: large enough for every size used
    below, though nothing may launch)."""
    from unscene3d_amd._lib import lib
    n = max(T, 1)
    z32 = torch.zeros(4 * 128 * 33 + L * 128 * 130, dtype=torch.float32, device=device)      # every float argument
    zi = torch.zeros(4 * 128 * 33, dtype=torch.int64, device=device)                          # every integer argument
    ws = torch.zeros(max(int(lib.usc_criterion_ws_bytes(L, S, min(n, 128))), 256), dtype=torch.uint8, device=device)
    ptrs = (ctypes.c_void_p * L)(*[z32.data_ptr()] * L)
    f, i, m = z32.data_ptr(), zi.data_ptr(), max_targets
    return {
        "usc_criterion_target_bits": lambda: lib.usc_criterion_target_bits(i, T, m, S, i, i, None),
        "usc_criterion_costs": lambda: lib.usc_criterion_costs(
            ptrs, L, 128, S, Q, T, m, i, i, f, Q * C, C, C, i, 5.0, 2.0, 2.0, f, f, f, f, f, f, ws.data_ptr(), ws.numel(), None),
        "usc_criterion_drop_counts": lambda: lib.usc_criterion_drop_counts(ptrs, L, 128, S, Q, T, m, i, i, i, i, None),
        "usc_criterion_losses": lambda: lib.usc_criterion_losses(
            f, f, f, i, i, i, f, L, Q, T, m, C, C - 1, i, f, None, None, 0.0, None, None),
        "usc_criterion_backward": lambda: lib.usc_criterion_backward(
            ptrs, ptrs, L, 128, S, Q, T, m, i, i, i, i, f, f, f, i, f, f, f, C, Q * C, C, f, None, None),
    }, (z32, zi, ws)


@pytest.mark.parametrize("Q,T", [(64, 0), (128, 129), (40, 41)])
def test_wide_entry_points_reject_sizes_outside_their_bounds(device, Q, T):
    """max_targets = 128 and T = 0, T = 129, T > Q: an error code and a message that names the function and the bound,
    before anything is launched."""
    from unscene3d_amd._lib import last_error
    calls, _buffers = _bound_calls(device, 2, 33, Q, T, 3, 128)
    if T > Q:                                                             # this one has no Q to compare with
        del calls["usc_criterion_target_bits"]
    for name, call in calls.items():
        assert call() != 0, name
        msg = last_error()
        assert name in msg and "128" in msg, (name, msg)
    torch.cuda.synchronize()


def test_the_existing_entry_points_keep_rejecting_more_than_32_targets(device):
    """max_targets = 32 (the default training path) refuses a 33-target scene in the library and in the driver; a
    max_targets outside 32 .. 128 is refused by all five functions.  33 targets, S = 33, Q = 64, L = 1: the smallest
    shape that crosses the word boundary."""
    from unscene3d_amd import criterion_device as D
    from unscene3d_amd._lib import last_error, lib
    z = torch.zeros(64 * 64, dtype=torch.int64, device=device)
    assert lib.usc_criterion_target_bits(z.data_ptr(), 33, 32, 33, z.data_ptr(), z.data_ptr(), None) != 0
    assert "1..32" in last_error()
    ptrs = (ctypes.c_void_p * 1)(z.data_ptr())
    assert lib.usc_criterion_drop_counts(ptrs, 1, 64, 33, 64, 33, 32, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                         z.data_ptr(), None) != 0
    assert "1..32" in last_error()
    for m in (31, 129):
        calls, _buffers = _bound_calls(device, 1, 33, 64, 33, 3, m)
        for name, call in calls.items():
            assert call() != 0, (name, m)
            assert name in last_error(), (name, m, last_error())
    torch.cuda.synchronize()
    # the driver: ValueError before any allocation or launch
    case = _make(("random", 1, 64, 3, "Q", 0.1, [(33, 33)], 0))
    allocated = []

    def alloc(shape, dtype):
        allocated.append(shape)
        return torch.empty(shape, dtype=dtype, device=device)
    tabs = [case["masks"][0][0].to(device).contiguous()]
    tm8 = case["tm"][0].to(device).contiguous().view(torch.uint8)
    logits = torch.stack(case["logits"]).to(device).contiguous()
    part = torch.full((1, 4), float("nan"), device=device)
    with pytest.raises(ValueError, match="33 targets, the caller allows 32"):
        D.scene_forward(tabs, tm8, case["labels"][0].to(device), logits, 0, (5.0, 2.0, 2.0),
                        torch.ones(3, device=device), 2, part, alloc=alloc, max_targets=32)
    torch.cuda.synchronize()
    assert not allocated and bool(torch.isnan(part).all())


def test_set_criterion_rejects_device_max_targets_above_128():
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    matcher = HungarianMatcher(cost_noise_robust=0.0, num_points=-1, **CC.COST_WEIGHTS)
    with pytest.raises(ValueError, match="device_max_targets"):
        SetCriterion(num_classes=3, matcher=matcher, weight_dict={}, eos_coef=0.1, losses=["labels", "masks"],
                     num_points=-1, oversample_ratio=3.0, importance_sample_ratio=0.75, class_weights=-1,
                     device_max_targets=129)
