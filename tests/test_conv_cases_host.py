"""The case table of tests/conv_cases.py is what it claims to be (no GPU: the planning entry points do not touch the
device): every case reaches the plan written next to it, the table reaches every kernel variant the planners can
choose, the exact cases are exact, the comparators reject planted errors and accept an f32 evaluation on the CPU.

Instantiations that are compiled and that no shape reaches (nothing in the table can run them; DESIGN.md lists them):
  wgrad_full_kernel<2,3>, <1,3>   three column blocks need cin / 32 divisible by 3 (-> <3,3>) or by 4 (-> <4,3>); every
                                  other cin goes to wgrad_kernel
  wgrad_kernel<1,true>, <2,true>  an aligned shape leaves wgrad_full_kernel only with cout a multiple of 96, where
                                  pick_nb gives 3 or 4
"""
import pytest
import torch

import conv_cases as cc
from unscene3d_amd._lib import lib

# every kernel variant usc_spconv_plan can answer with, kind 0 (row-order / stem / tile-compacted) and kind 2 (wgrad)
FORWARD_VARIANTS = {"al1", "al2", "al3", "al4", "un1", "un2", "un3", "un4", "stem", "ct1", "ct2", "ct3"}
WGRAD_VARIANTS = {"full1x1", "full1x2", "full1x4", "full2x1", "full2x2", "full2x4", "full3x1", "full3x2", "full3x3",
                  "full4x1", "full4x2", "full4x3", "wg3a", "wg4a", "wg1u", "wg2u", "wg3u", "wg4u"}
SWEEP_CHANNELS = sorted({1, 2, 3, 4, 20, 40, 50, 100} | set(range(32, 513, 32)))
SWEEP_ROWS = (1, 700, 4096, 24575, 24576, 49153, 65537, 150000)
SWEEP_K = (1, 8, 27)
CPU_COST = 3e8                    # multiply-adds of a reference the CPU tests run per case (well under a second)


def test_case_names_are_unique():
    for fam, cases in cc.CASES.items():
        names = [c.name for c in cases]
        assert len(names) == len(set(names)), fam


@pytest.mark.parametrize("family", list(cc.CASES))
def test_every_case_reaches_the_plan_written_next_to_it(family):
    wrong = [(c.name, c.plan, cc.decoded_plan(lib, c)) for c in cc.CASES[family] if cc.decoded_plan(lib, c) != c.plan]
    assert not wrong, wrong
    for c in cc.CASES[family]:
        if family == "compact":
            assert c.tm == cc.compact_tm(c.n, int(c.plan[2])) and c.K <= 27 and c.cin >= 64 and c.n >= 24576
        if family == "group":
            assert lib.usc_spconv_wgrad_group_max() >= c.n


def test_compact_cases_sit_on_the_tile_height_steps():
    tms = {(c.n, int(c.plan[2])): c.tm for c in cc.CASES["compact"]}
    assert tms[(24576, 1)] == 96 and tms[(24577, 1)] == 100 and tms[(49153, 1)] == 196
    assert tms[(65536, 2)] == 256 and tms[(65537, 2)] == 132 and tms[(49153, 3)] == 100 and tms[(24577, 3)] == 100


def test_the_table_reaches_every_variant_the_planners_choose():
    fwd = {cc.variant(c.plan) for f in ("row", "stem", "compact") for c in cc.CASES[f]}
    wg = {cc.variant(c.plan) for c in cc.CASES["wgrad"]}
    assert fwd == FORWARD_VARIANTS
    assert wg == WGRAD_VARIANTS
    swept_fwd, swept_wg = set(), set()
    for cin in SWEEP_CHANNELS:
        for cout in SWEEP_CHANNELS:
            for n in SWEEP_ROWS:
                for K in SWEEP_K:
                    swept_fwd.add(cc.variant(cc.plan_string(0, lib.usc_spconv_plan(0, n, cin, cout, K))))
                    swept_wg.add(cc.variant(cc.plan_string(2, lib.usc_spconv_plan(2, n, cin, cout, K))))
    assert swept_fwd == FORWARD_VARIANTS           # a planner change that opens a variant without a case fails here
    assert swept_wg == WGRAD_VARIANTS
    # the list form (kind 1) and the mask-sorted kernel: every width of their tiles has a case
    assert {c.plan for c in cc.CASES["pairs"]} == {"al1", "al2", "al3", "al4", "un2"}
    assert {cc.variant(c.plan) for c in cc.CASES["sorted"]} == {"s1", "s2", "s3", "s4"}
    assert {c.plan.split("/")[1] == "G1" for c in cc.CASES["sorted"]} == {True, False}


def test_sorted_selection_covers_every_size_the_issue_names():
    cs = cc.CASES["sorted"]
    assert {2, 8, 27, 32} <= {c.K for c in cs}
    assert {1, 31, 33, 255, 257, 700, 4095, 4096} <= {c.n for c in cs}
    assert {32, 64, 96, 128, 160} <= {c.cout for c in cs}
    assert {32, 96, 4096} <= {c.cin for c in cs}
    assert any(c.slices for c in cs) and any(c.wt for c in cs)
    assert any(c.bias and c.acc and c.plan.endswith("G1") for c in cs)
    assert any(c.bias and c.acc and not c.plan.endswith("G1") for c in cs)


def test_exact_rows_workspace_never_exceeds_the_bound():
    for cin in SWEEP_CHANNELS:
        for cout in SWEEP_CHANNELS:
            for K in SWEEP_K:
                hi = lib.usc_spconv_wgrad_ws_bytes(K, cin, cout)
                for n in SWEEP_ROWS + (2 << 20, 5 << 20):
                    lo = lib.usc_spconv_wgrad_ws_bytes_rows(K, cin, cout, n)
                    assert K * cin * cout * 4 <= lo <= hi, (K, cin, cout, n)


def test_every_exact_case_stays_below_two_to_the_24():
    for c in cc.all_cases():
        assert cc.exactness_bound(c) < cc.EXACT_LIMIT, c.name


def _cpu_forward(c, mode, dtype=torch.float64, **over):
    t = cc.forward_inputs(c, mode)
    t.update(over)
    return t, cc.ref_forward(t["x"], t["W"], t["nbr"], c.n, t["bias"], t["before"], c.wt, dtype, exact=mode == "exact")


def _small_forward_cases():
    return [c for f in ("row", "stem", "compact", "sorted") for c in cc.CASES[f] if cc.forward_cost(c) <= CPU_COST]


@pytest.mark.parametrize("mode", cc.MODES)
def test_comparators_accept_an_f32_evaluation_of_the_forward_reference(mode):
    """Exact inputs: f32 arithmetic in any order gives the float64 result bit for bit.  Bounded inputs: a blocked f32
    evaluation stays inside 2**-20 * mag."""
    worst = 0.0
    cases = _small_forward_cases()
    assert len(cases) > 150
    for c in cases:
        t, (ref, mag) = _cpu_forward(c, mode)
        y32, _ = cc.ref_forward(t["x"], t["W"], t["nbr"], c.n, t["bias"], t["before"], c.wt, torch.float32)
        assert cc.accepts(mode, y32, ref, mag), (c.family, c.name)
        if mode == "bounded":
            worst = max(worst, cc.bounded_ratios(y32, ref, mag)[0])
    print(f"forward, f32 on the CPU, {mode}: {len(cases)} cases, worst fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("mode", cc.MODES)
def test_comparators_accept_an_f32_evaluation_of_the_other_references(mode):
    ex = mode == "exact"
    for c in cc.CASES["pairs"]:
        if sum(c.counts) * c.cin * c.cout > CPU_COST:
            continue
        t = cc.pairs_inputs(c, mode)
        ref, mag, written = cc.ref_pairs(t["x"], t["W"], t["rows_in"], t["rows_out"], t["koff"], c.n, exact=ex)
        y32, _, w32 = cc.ref_pairs(t["x"], t["W"], t["rows_in"], t["rows_out"], t["koff"], c.n, dtype=torch.float32)
        assert cc.accepts(mode, y32, ref, mag) and int(written.sum()) == sum(c.counts) and bool((written == w32).all())
    for c in cc.CASES["wgrad"]:
        t = cc.wgrad_inputs(c, mode)
        ref, mag = cc.ref_wgrad(t["a"], t["b"], c.K, t["a_idx"], t["b_idx"], t["koff"], t["before"], exact=ex)
        y32, _ = cc.ref_wgrad(t["a"], t["b"], c.K, t["a_idx"], t["b_idx"], t["koff"], t["before"], dtype=torch.float32)
        assert cc.accepts(mode, y32, ref, mag), c.name
    for c in cc.CASES["stem_wgrad"]:
        t = cc.stem_wgrad_inputs(c, mode)
        ref, mag = cc.ref_wgrad_table(t["x"], t["dy"], t["nbr"], t["before"], exact=ex)
        y32, _ = cc.ref_wgrad_table(t["x"], t["dy"], t["nbr"], t["before"], dtype=torch.float32)
        assert cc.accepts(mode, y32, ref, mag), c.name


def test_pair_lists_have_the_tails_the_pipelines_care_about():
    seen = {n for c in cc.CASES["wgrad"] for n in c.counts}
    assert {0, 1, 7, 8, 9, 15, 16, 17, 31, 33} <= seen
    assert any(c.counts and c.counts[0] == 0 and c.counts[-1] == 0 for c in cc.CASES["wgrad"])
    assert any(c.capacity > sum(c.counts) for c in cc.CASES["wgrad"])
    assert {0, 1, 31, 32, 33, 64, 5} <= {n for c in cc.CASES["pairs"] for n in c.counts}


# ------------------------------------------------------------------------------------ planted errors
def _rejects(mode, y64, ref, mag):
    return not cc.accepts(mode, y64.float(), ref, mag)


@pytest.mark.parametrize("mode", cc.MODES)
def test_comparators_reject_planted_errors_in_the_largest_forward_case(mode):
    c = max((c for f in ("row", "compact", "sorted") for c in cc.CASES[f]), key=cc.forward_cost)
    g = torch.Generator().manual_seed(5)
    bias = torch.randint(-2, 3, (c.cout,), generator=g).float() if mode == "exact" else torch.randn(c.cout, generator=g)
    t, (ref, mag) = _cpu_forward(c, mode, bias=bias)
    assert cc.accepts(mode, ref.float(), ref, mag)
    We = cc.effective_weights(t["W"], c.wt).double()
    K = c.K
    k = 3
    o = int(torch.nonzero(t["nbr"][k] >= 0).flatten()[c.n // 2 // 2])
    r = int(t["nbr"][k, o])
    contrib = t["x"][r].double() @ We[k]
    assert float(contrib.abs().max()) > 0
    dropped, doubled = ref.clone(), ref.clone()
    dropped[o] -= contrib
    doubled[o] += contrib
    assert _rejects(mode, dropped, ref, mag), "one pair dropped"
    assert _rejects(mode, doubled, ref, mag), "one pair counted twice"
    swapped, _ = cc.ref_forward(t["x"], t["W"].flip(0), t["nbr"], c.n, bias, None, c.wt)
    assert K > 1 and _rejects(mode, swapped, ref, mag), "weights of offsets k and K-1-k swapped"
    moved = ref.clone()
    moved[o + 1] = ref[o]
    moved[o] = bias.double()
    assert _rejects(mode, moved, ref, mag), "one output row stored one row further"
    assert _rejects(mode, ref + bias.double(), ref, mag), "bias added twice"
    if mode == "bounded":
        terms = t["x"][r].double() * We[k][:, 0]
        ch = int(terms.abs().argmax())
        less = ref.clone()
        less[o, 0] -= terms[ch]
        assert _rejects(mode, less, ref, mag), "one product term removed from one element"
        print(f"removed term / bound = {float(terms[ch].abs() / (cc.BOUND * mag[o, 0])):.1f}")


@pytest.mark.parametrize("mode", cc.MODES)
def test_comparators_reject_planted_errors_in_the_largest_weight_gradient_case(mode):
    c = max((c for c in cc.CASES["wgrad"] if c.table), key=lambda c: (sum(c.counts), c.cin * c.cout, c.acc))
    assert c.acc and sum(c.counts) >= 12288
    t = cc.wgrad_inputs(c, mode)
    ref, mag = cc.ref_wgrad(t["a"], t["b"], c.K, t["a_idx"], t["b_idx"], t["koff"], t["before"], exact=mode == "exact")
    assert cc.accepts(mode, ref.float(), ref, mag)
    k = 3
    p = int(t["koff"][k]) + 11
    av, bv = t["a"][int(t["a_idx"][p])].double(), t["b"][int(t["b_idx"][p])].double()
    outer = av[:, None] * bv[None, :]
    assert float(outer.abs().max()) > 0
    dropped, doubled = ref.clone(), ref.clone()
    dropped[k] -= outer
    doubled[k] += outer
    assert _rejects(mode, dropped, ref, mag), "one pair dropped"
    assert _rejects(mode, doubled, ref, mag), "one pair counted twice"
    plain, _ = cc.ref_wgrad(t["a"], t["b"], c.K, t["a_idx"], t["b_idx"], t["koff"])
    assert _rejects(mode, plain.flip(0) + t["before"].double(), ref, mag), "offsets k and K-1-k swapped"
    flat = ref.reshape(c.K * c.cin, c.cout)
    moved = flat.clone()
    row = k * c.cin + 5
    moved[row + 1] = flat[row]
    moved[row] = t["before"].reshape(c.K * c.cin, c.cout)[row].double()
    assert _rejects(mode, moved.reshape(ref.shape), ref, mag), "one row of dW stored one row further"
    assert _rejects(mode, ref + t["before"].double(), ref, mag), "the pre-existing gradient added twice"
    if mode == "bounded":
        ci = int(av.abs().argmax())
        less = ref.clone()
        co = int(bv.abs().argmax())
        less[k, ci, co] -= av[ci] * bv[co]
        assert _rejects(mode, less, ref, mag), "one product term removed from one element"
