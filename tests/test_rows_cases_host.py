"""The case table of tests/rows_cases.py is what it claims to be (no GPU: usc_bn_plan launches nothing): every case
reaches the form written next to it, a sweep of usc_bn_plan answers with no form that lacks a case, the condition cap of
the one-pass variance holds for every case, the comparators accept an evaluation in the kernels' arithmetic (f64 one-pass
sums, f32 finalisation, f32 element-wise passes) and reject planted errors.

Compiled and out of reach of the table: nothing in the statistics forms.  bn_small_kernel also takes widths above 1024
(any multiple of 4) at its row counts; the table stops at 1024, the widest batch norm of the models."""
import pytest
import torch

import rows_cases as rc
from unscene3d_amd._lib import lib

STAT_FORMS = {"refused", "small/x0", "small/x1", "two4", "two1"}
SWEEP_ROWS = (1, 1024, 1025, 4096, 4097, 65537, 150000)
SWEEP_CHANNELS = (1, 3, 4, 32, 100, 256, 258, 1024)
F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------- the table
def test_case_names_are_unique():
    for fam, cases in rc.BN_CASES.items():
        names = [c.name for c in cases]
        assert len(names) == len(set(names)), fam
    for cases in (rc.POOL_CASES, rc.MOVE_CASES, rc.SEG_CASES):
        assert len({c.name for c in cases}) == len(cases)


@pytest.mark.parametrize("family", list(rc.BN_CASES))
def test_every_case_reaches_the_plan_written_next_to_it(family):
    wrong = [(c.name, c.plan, rc.decoded_plan(lib, c)) for c in rc.BN_CASES[family] if rc.decoded_plan(lib, c) != c.plan]
    assert not wrong, wrong


def test_plan_refuses_bad_sizes():
    assert lib.usc_bn_plan(0, 32, 0) == -1 and lib.usc_bn_plan(5, 0, 1) == -1


def test_the_table_reaches_every_form_the_plan_answers_with():
    for back, fam in ((0, "fwd"), (1, "bwd")):
        have = {rc.stat_form(c.plan) for c in rc.BN_CASES[fam]}
        assert have == STAT_FORMS, (fam, have)
        swept = {rc.stat_form(rc.stat_plan_string(lib.usc_bn_plan(n, c, back))) for n in SWEEP_ROWS for c in SWEEP_CHANNELS}
        assert swept <= have, (fam, swept - have)               # a threshold change that opens a form without a case
        assert swept == STAT_FORMS
    # the block cap of the two-launch form from both sides, in both directions
    for fam in ("fwd", "bwd"):
        blocks = {int(c.plan.split("/B")[1]) for c in rc.BN_CASES[fam] if "/B" in c.plan}
        assert 1024 in blocks and 1 in blocks and any(1 < b < 1024 for b in blocks)
    # tile geometry: both tile heights at the 2048 / 2049 step, one tile, 64 tiles, and maps the units leave alone
    tiles = {c.plan for c in rc.BN_CASES["tile"]}
    assert {"t32x64/u", "t64x33/u", "t32x1/u", "t64x64/u"} <= tiles and any(not p.endswith("/u") for p in tiles)
    for n in SWEEP_ROWS:
        for c in SWEEP_CHANNELS:
            p = rc.decode_plan(lib.usc_bn_plan(n, c, 0))
            assert p["tile_ok"] == int(c % 32 == 0) and p["units"] == int(c % 32 == 0 and n <= lib.usc_bn_tile_max_rows())
            if p["tile_ok"]:
                assert 1 <= p["ntiles"] <= 64 and p["tr"] % 32 == 0 and (p["ntiles"] - 1) * p["tr"] < n <= p["ntiles"] * p["tr"]


def test_the_table_covers_the_sizes_the_kernels_branch_on():
    fwd, bwd, tile = (rc.BN_CASES[f] for f in ("fwd", "bwd", "tile"))
    small = [c for c in fwd if c.plan.startswith("small")]
    assert {1, 2, 255, 256, 257, 1023, 1024, 1025, 4096} <= {c.n for c in small}
    assert {4, 32, 36, 96, 100, 256, 1024} <= {c.c for c in small}
    assert {1, 255, 1024} <= {c.n for c in bwd if c.plan.startswith("small")}
    assert {c.n for c in fwd if c.plan.startswith("two4")} >= {4097, 12000, 70001, 16401}
    assert {c.c for c in fwd if c.plan.startswith("two4")} >= {4, 100, 516, 1024}
    assert {(c.n, c.c) for c in fwd if c.plan.startswith("two1")} == {(n, c) for n in (1, 33, 5000) for c in (1, 3, 19, 255)}
    assert 1025 in {c.n for c in bwd if c.plan.startswith("two")} and 12000 in {c.n for c in bwd}
    assert {c.n for c in tile} == {1, 31, 32, 33, 2047, 2048, 2049, 4096, 4097, 12000}
    assert {c.c for c in tile} == {32, 64, 96, 256, 1024} and {c.G for c in tile} == {0, 1, 7, 8, 9, 16, 27}
    for cases in (fwd, bwd):
        for form in {rc.stat_form(c.plan) for c in cases} - {"refused"}:
            assert any(c.shift for c in cases if rc.stat_form(c.plan) == form), form      # 4-byte aligned parameters
    assert any(c.shift for c in tile)
    for flag in ("res", "relu", "acc", "slice_acc"):
        assert {getattr(c, flag) for c in tile} == {False, True}, flag
    assert {c.training for c in tile} == {0, 1} and {c.training for c in bwd} == {0, 1}
    assert {(c.relu, c.dres) for c in bwd} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c.res, c.relu) for c in fwd if c.plan != "refused"} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.G > 0 and not c.dres for c in tile) and any(c.G == 0 and not c.dres for c in tile)
    assert any((c.n * c.c // (4 if c.c % 4 == 0 else 1)) % 256 for c in fwd)               # a ragged last workgroup


def test_condition_cap_holds_for_every_case():
    worst = 0.0
    for c in rc.all_bn_cases():
        if c.plan == "refused":
            continue
        k = rc.condition(rc.bn_inputs(c)["x"])
        worst = max(worst, k)
        assert k <= rc.CONDITION_CAP, (c.family, c.name, k)
    print(f"largest E[x^2] / (var + eps) of the table: 2**{torch.log2(torch.tensor(worst)).item():.1f}")
    # every recipe is present in a case with eight columns or more
    x = rc.recipe_table(507, 16, 3).double()
    assert bool((x.var(0) == 0).any()) and float(x.mean(0).abs().max()) > 900 and bool((x == x.round()).all(0).sum() >= 2)


def test_mask_inputs_hold_both_zeros_and_tiny_positives():
    y = rc.mask_input(255, 100, 1)
    bits = y.view(torch.int32)
    assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any()) and bool(((y > 0) & (y < 1e-37)).any())
    assert bool(((y > 0) & (y < 1.1e-38)).any())                                              # a denormal


# ------------------------------------------------------------------------------------------------- emulation
def emu_stats(x, t, acc=F64, drop_last=False, biased=False):
    """The kernels' arithmetic: one-pass sums in `acc`, finalisation in acc, results and the rest in f32."""
    n = x.shape[0]
    xa = (x[:-1] if drop_last else x).to(acc)
    m = xa.sum(0) / n
    var = ((xa * xa).sum(0) / n - m * m).clamp_min(0.0)
    mean = m.float()
    invstd = (1.0 / torch.sqrt(var + rc.EPS)).float()
    scale = t["gamma"] * invstd
    unbiased = (var * (1.0 if biased or n == 1 else n / (n - 1.0))).float()
    return dict(mean=mean, invstd=invstd, scale=scale, shift=t["beta"] - mean * scale,
                rm=(1 - rc.MOMENTUM) * t["rm"] + rc.MOMENTUM * mean, rv=(1 - rc.MOMENTUM) * t["rv"] + rc.MOMENTUM * unbiased)


def emu_apply(x, st, res, relu, res_times=1):
    out = x * st["scale"] + st["shift"]
    for _ in range(res_times if res is not None else 0):
        out = out + res
    return out.clamp_min(0.0) if relu else out


def emu_backward(c, t, ge=False, keep_means=False):
    x, dy, n = t["x"], t["dy"], t["x"].shape[0]
    mu, is_ = t["mean32"], t["invstd32"]
    g = dy if t["y_out"] is None else torch.where((t["y_out"] >= 0) if ge else (t["y_out"] > 0), dy, torch.zeros_like(dy))
    xhat = (x - mu) * is_
    sg, sgx = g.double().sum(0), (g.double() * xhat.double()).sum(0)
    train = c.training or keep_means
    mg = (sg / n).float() if train else torch.zeros_like(mu)
    mx = (sgx / n).float() if train else torch.zeros_like(mu)
    dbeta, dgamma = sg.float(), sgx.float()
    if c.acc:
        dbeta, dgamma = t["dbeta0"] + dbeta, t["dgamma0"] + dgamma
    return dict(dbeta=dbeta, dgamma=dgamma, mean_g=mg, mean_gx=mx, dres=g, dx=t["gamma"] * is_ * (g - mg - xhat * mx))


def _refs(c, t):
    st = rc.ref_stats(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"])
    out = rc.ref_apply(t["x"], st, t["beta"], t["res"], c.relu)
    rb = None
    if c.family in ("bwd", "tile"):
        rb = rc.ref_backward(t["x"], t["dy"], t["y_out"], t["mean32"], t["invstd32"], t["gamma"], c.training,
                             t["dgamma0"] if c.acc else None, t["dbeta0"] if c.acc else None)
    return st, out, rb


def _cases(max_rows=None):
    return [c for c in rc.all_bn_cases() if c.plan != "refused" and (max_rows is None or c.n <= max_rows)]


def _merge(worst, fr):
    for k, v in fr.items():
        worst[k] = max(worst.get(k, 0.0), v)


def test_comparators_accept_the_kernels_arithmetic_on_every_case():
    worst = {}
    for c in _cases():
        t = rc.bn_inputs(c)
        st, (out, mag), rb = _refs(c, t)
        if c.family in ("fwd", "tile"):
            e = emu_stats(t["x"], t)
            fr = rc.stats_fractions(e, st)
            fr["out"] = rc.elem_ratio(emu_apply(t["x"], e, t["res"], c.relu), out, mag)
            assert max(fr.values()) <= 1.0, (c.family, c.name, fr)
            _merge(worst, fr)
        if rb is not None:
            e = emu_backward(c, t)
            fr = rc.backward_fractions(e, rb)
            assert max(fr.values()) <= 1.0 and rc.same_bits(e["dres"], rb["g32"]), (c.family, c.name, fr)
            if not c.training:
                assert not bool(rb["mean_g"].any()) and not bool(rb["mean_gx"].any())
            _merge(worst, fr)
    print("f32 arithmetic / f64 sums on the CPU, largest fraction of each bound over every case:")
    print("  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------- planted errors
def _wide(c):
    """Eight columns or more: every recipe is in the case."""
    return c.c >= rc.N_RECIPES


def test_every_row_count_up_to_4097_has_a_case_with_every_recipe():
    rows = {c.n for c in _cases(4097)}
    assert rows == {c.n for c in _cases(4097) if _wide(c)}
    assert {1, 2, 33, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097} <= rows


def test_comparators_reject_planted_errors_in_the_statistics():
    cases = [c for c in _cases(4097) if c.family in ("fwd", "tile") and _wide(c)]
    cases.append(next(c for c in rc.BN_CASES["fwd"] if c.n == 70001))
    for c in cases:
        t = rc.bn_inputs(c)
        st, (out, mag), _ = _refs(c, t)

        def rejected(e):
            fr = rc.stats_fractions(e, st)
            fr["out"] = rc.elem_ratio(emu_apply(t["x"], e, t["res"], c.relu), out, mag)
            return max(fr.values()) > 1.0

        if c.n > 1:                                               # (one row: nothing is left / the factor is 1 by rule)
            assert rejected(emu_stats(t["x"], t, drop_last=True)), (c.name, "the last row left out of the statistics")
        if c.n == 70001:
            continue
        if c.n > 1:                      # (one row: s2 / n - m * m is fl(x * x) - fl(x * x) = 0 in either precision)
            assert rejected(emu_stats(t["x"], t, acc=F32)), (c.name, "statistics accumulated in f32")
        if c.n > 1:
            assert rc.stats_fractions(emu_stats(t["x"], t, biased=True), st)["running_var"] > 1.0, (c.name, "biased running var")
        e = emu_stats(t["x"], t)
        live = 0
        for j in range(8):                                        # whichever recipe the column has
            if not bool((out[:, j] > 0).any()):
                continue                                          # ReLU left nothing of this column
            live += 1
            sw = dict(e, scale=torch.where(torch.arange(c.c) == j, e["scale"].roll(-1), e["scale"]))
            assert rc.elem_ratio(emu_apply(t["x"], sw, t["res"], c.relu), out, mag) > 1.0, (c.name, j, "neighbour's scale")
        assert live >= 2, c.name
        if c.res:
            assert rc.elem_ratio(emu_apply(t["x"], e, t["res"], c.relu, res_times=2), out, mag) > 1.0, (c.name, "residual twice")


def test_comparators_reject_planted_errors_in_the_backward():
    seen = set()
    for c in [c for c in _cases(4097) if c.family in ("bwd", "tile") and _wide(c)]:
        t = rc.bn_inputs(c)
        _, _, rb = _refs(c, t)
        if c.relu:
            e = emu_backward(c, t, ge=True)
            assert not rc.same_bits(e["dres"], rb["g32"]), (c.name, "mask by >= : dres")
            assert max(rc.backward_fractions(e, rb).values()) > 1.0, (c.name, "mask by >=")
            seen.add("ge")
        if not c.training:
            e = emu_backward(c, t, keep_means=True)
            assert rc.backward_fractions(e, rb)["dx"] > 1.0, (c.name, "mean_g not zeroed in eval mode")
            seen.add("eval")
        if c.n > 1:
            short = dict(t, x=t["x"][:-1], dy=t["dy"][:-1], y_out=None if t["y_out"] is None else t["y_out"][:-1])
            e = emu_backward(c, short)
            fr = dict(dbeta=rc.stat_ratio(e["dbeta"], rb["dbeta"], rb["dbeta_terms"], rb["dbeta_before"]),
                      dgamma=rc.elem_ratio(e["dgamma"], rb["dgamma"], rb["dgamma_mag"]))
            assert fr["dbeta"] > 1.0 and fr["dgamma"] > 1.0, (c.name, "the last row left out of dbeta / dgamma", fr)
    assert seen == {"ge", "eval"}


# ------------------------------------------------------------------------------------------------- row movers
@pytest.mark.parametrize("mode", ("exact", "bounded"))
def test_pooling_reference_accepts_f32_and_rejects_a_child_counted_twice(mode):
    worst = 0.0
    for c in rc.POOL_CASES:
        t = rc.pool_inputs(c, mode)
        ref, mag = rc.ref_pool(t["src"], t["nbr2"], t["row_of"], c.c)
        cnt = (t["nbr2"] >= 0).sum(0)
        assert int(cnt[0]) == 0 and int(cnt[1]) == 8 and float(ref[0].abs().max()) == 0.0
        if mode == "exact":
            assert set(cnt.tolist()) <= {0, 1, 2, 4, 8}
        acc = torch.zeros((c.n_coarse, c.c))
        for k in range(8):                                       # f32, child order: the kernel's sum
            ch = t["nbr2"][k].long()
            rows = t["row_of"][ch.clamp_min(0)] if c.row_of else ch.clamp_min(0)
            acc = acc + torch.where((ch >= 0)[:, None], t["src"][rows][:, :c.c], torch.zeros(()))
        y = acc * (1.0 / cnt.clamp_min(1).float())[:, None]
        assert rc.accepts(mode, y, ref, mag), c.name
        if mode == "bounded":
            worst = max(worst, rc.bounded_ratios(y, ref, mag)[0])
        p = int(torch.nonzero(cnt == (8 if mode == "exact" else cnt.max())).flatten()[0])
        k = int(torch.nonzero(t["nbr2"][:, p] >= 0).flatten()[0])
        ch = int(t["nbr2"][k, p])
        extra = t["src"][int(t["row_of"][ch]) if c.row_of else ch][:c.c]
        if float(extra.abs().max()) > 0:
            twice = y.clone()
            twice[p] += extra / cnt[p]
            assert not rc.accepts(mode, twice, ref, mag), (c.name, "one pooled child counted twice")
    print(f"pooling, f32 on the CPU, {mode}: worst fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("mode", ("exact", "bounded"))
def test_segment_reference_accepts_f32_and_rejects_count_plus_one(mode):
    for c in rc.SEG_CASES:
        seg = rc.segment_ids(c)
        assert seg.shape[0] == c.n and (c.n == 0 or (0 <= int(seg.min()) and int(seg.max()) < c.S))
        src = rc.segment_values(c, mode)
        counts = torch.bincount(seg, minlength=c.S)
        if c.n >= 1023 and c.S > 1:
            assert bool((counts == 0).any()) and int(rc.is_pow2(counts).sum()) >= 10, c.name      # empty segments, exact ones
        if c.layout == "chunks":
            assert len(set(seg[:64].tolist())) == 1 and len(set(seg[64:128].tolist())) == 64
        for m in ("mean", "mean_nonzero", "max_nonzero"):
            ref, mag, cnt = rc.ref_segment(src, seg, c.S, m)
            y = ref.float()
            assert rc.accepts("bounded", y, ref, mag)
            if m == "mean":
                assert torch.equal(cnt, counts)
                if c.n:
                    s = int(seg[0])
                    wrong = y.clone()
                    wrong[s] = (ref[s] * cnt[s] / (cnt[s] + 1)).float()
                    if float(ref[s].abs().max()) > 0:
                        assert not rc.accepts("bounded", wrong, ref, mag), (c.name, "mean divided by count + 1")
            else:
                if c.n >= 1023 and c.S > 1:
                    assert bool(((cnt == 0) & (counts > 0)).any()), (c.name, "no segment with only all-zero rows")
            if mode == "exact":
                ok = rc.is_pow2(cnt) if m != "max_nonzero" else torch.ones_like(cnt, dtype=torch.bool)
                assert torch.equal(y[ok].double(), ref[ok])                    # exactly representable: f32 must hit it


def test_move_cases_index_sets():
    for c in rc.MOVE_CASES:
        idx = rc.move_indices(c)
        assert idx.shape[0] == c.n and int(idx.max()) < c.n_src
        uniq = idx.unique().shape[0]
        assert (uniq < c.n) == (c.kind == "dup") and (uniq == c.n_src) == (c.kind == "perm")
