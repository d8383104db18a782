"""The case tables of tests/attention_cases.py are what they claim to be (no GPU): unique names, every query and key count
the kernels of csrc/attention.hip and the split planner branch on, every plan string equal to what the library plans
(decoded from usc_attn_ws_bytes), score and mask recipes that do what their names say; the comparators accept an
evaluation in the kernels' arithmetic and reject planted errors.

The kernels' arithmetic on the CPU, in f32 with torch.exp / torch.log:
  cross forward   per key split an online softmax over chunks of 32 keys (m_new = max(m_run, chunk max), m_safe = 0 where
                  that is -inf, alpha = exp(m_run - m_safe), l = l alpha + sum p, o = o alpha + p v); the combine over the
                  splits' (o, m, l) in four interleaved groups (group g takes splits g, g + 4, ...), the groups added as
                  (g0 + g1) + (g2 + g3); o = acc / l, lse = M + log l, and 0 / +inf where l is not positive
  cross backward  from the f32 o and lse: D a 16-term f32 sum, p = exp(s - lse), one dq partial per (split, wave) with wave
                  w owning the chunks w, w + 4, ... of its split, the partials summed in the same four groups; dk / dv
                  per key from one product over the queries
  self attention  one launch: the chunks in sequence, o (1 / l) and m + log l; dq summed over the key chunks in order,
                  dk / dv over the query tiles in order
Planted errors (each must be rejected by at least one comparator on every case it applies to): _planted_forward and
_planted_backward."""
import math

import pytest
import torch

import attention_cases as ac

F32 = torch.float32
NEG = float("-inf")
HALF = 0.5
WS_WORD = torch.tensor([0xA5A5A5A5 - (1 << 32)], dtype=torch.int32).view(F32).item()     # a workspace byte pattern as f32


def _ids(cases):
    return [c.name for c in cases]


def _lib():
    from unscene3d_amd._lib import lib
    return lib


# ------------------------------------------------------------------------------------------------- the tables
def test_case_names_are_unique():
    for cases in (ac.CROSS_CASES, ac.SELF_CASES):
        names = [c.name for c in cases]
        assert len(names) == len(set(names)), names


def test_the_table_covers_the_sizes_the_kernels_branch_on():
    cross, slf = ac.CROSS_CASES, ac.SELF_CASES
    assert {c.L for c in cross} >= set(ac.CROSS_L) == {1, 31, 32, 33, 100, 128, 129, 150, 160, 161, 255, 256}
    assert {c.S for c in cross} >= set(ac.CROSS_S) == {1, 3, 31, 32, 33, 77, 200, 999, 1024, 1100, 2100}
    have = {(c.L, c.S, c.B, c.H): c.plan for c in cross}
    assert set(ac.PLANNER_ROWS) <= set(have)
    assert have[(100, 1100, 1, 8)] == "32x64 empty 14" and have[(100, 1024, 1, 8)] == "32x32 empty 0"
    assert have[(150, 999, 2, 8)] == "16x64 empty 0" and have[(5, 200, 33, 8)] == "1x224 empty 0"
    assert have[(33, 2100, 1, 1)] == have[(129, 2100, 1, 1)] == "64x64 empty 31"
    assert [k for k in have if k[1] > 2100] == [(256, 3200, 1, 8)] and max(c.L for c in cross) == 256
    assert {c.H for c in cross} == {1, 3, 8} and {c.B * c.H for c in cross} >= {255, 256, 264}
    assert {c.repeat for c in cross} == {False, True} and 35 <= len(cross) <= 45
    for L in (128, 129):                                             # both sides of the NG switch see empty splits
        assert any("empty 0" not in c.plan for c in cross if (c.L <= 128) == (L <= 128))
    assert {c.L for c in slf} == set(ac.SELF_L) == {1, 2, 31, 32, 33, 64, 100, 128, 129, 160, 161, 255, 256}
    assert {c.B for c in slf} == {1, 2, 3} and {c.H for c in slf} == {1, 3, 8} and 18 <= len(slf) <= 24
    assert {c.L for c in slf if c.count_mode} == {1, 2, 32, 64, 128, 256}
    assert {c.repeat for c in slf} == {False, True}


@pytest.mark.parametrize("c", ac.CROSS_CASES, ids=_ids(ac.CROSS_CASES))
def test_plan_strings_are_what_the_library_plans(c):
    lib = _lib()
    nbytes = lib.usc_attn_ws_bytes(c.L, c.S, c.B, c.H)
    nsplit = ac.nsplit_from_ws_bytes(nbytes, c.L, c.S, c.B, c.H)
    assert nsplit is not None, (c.name, nbytes, "not bits + partials + (m, l) + 256 for any split count")
    kps = -(-(-(-c.S // nsplit)) // 32) * 32
    decoded = ac.plan_string(nsplit, kps, nsplit - -(-c.S // kps))
    assert c.plan == decoded == ac.plan_string(*ac.planned(c.S, c.B, c.H)), (c.name, c.plan, decoded)
    assert sum(ac.ws_layout(c.L, c.S, c.B, c.H, nsplit)) == nbytes
    assert lib.usc_attn_lse_stride(c.L) == ac.lse_stride(c.L) == (128 if c.L <= 128 else 256)


def test_the_planner_rule():
    lib = _lib()
    assert [lib.usc_attn_lse_stride(L) for L in (1, 128, 129, 256)] == [128, 128, 256, 256]
    assert ac.planned(3200, 1, 8) == (32, 128, 7) and ac.planned(12800, 1, 8) == (32, 416, 1)
    assert ac.planned(200, 32, 8)[0] == 1 and ac.planned(200, 85, 3)[0] == 2            # one split from 256 heads on
    assert ac.planned(2048, 1, 3)[0] == 64 and ac.planned(2049, 1, 3)[0] == 64 and ac.planned(2016, 1, 3)[0] == 63
    assert ac.planned(4000, 1, 4)[0] == 64 and ac.planned(4000, 1, 5)[0] == 52


def test_the_recipe_pairs_the_issue_names_occur():
    pairs = set()
    for c in ac.CROSS_CASES:
        got = ac.realised_pairs(c)
        pairs |= got
        if c.L >= 7:
            assert "all" in {m for _, m in got}, (c.name, "no fully masked row")
    for s in ("sharp", "selector", "offset+", "offset-", "ramp"):
        for m in ("first chunk", "split", "one key"):
            assert (s, m) in pairs, (s, m)
    assert {s for s, _ in pairs} == set(ac.SCORE) and {m for _, m in pairs} == set(ac.MASK)


# ------------------------------------------------------------------------------------------------- the recipes
def _all_cases():
    return ac.CROSS_CASES + ac.SELF_CASES


def _all_ids():
    return ["cross-" + c.name for c in ac.CROSS_CASES] + ["self-" + c.name for c in ac.SELF_CASES]


@pytest.mark.parametrize("c", _all_cases(), ids=_all_ids())
def test_recipes_are_what_they_claim(c):
    t = ac.attn_inputs(c)
    L, S, B, H = c.L, c.S, c.B, c.H
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], H)
    srec, pi = t["srec"], t["pi"]
    opened = ~ac._masked(t["mask"], B, L, S, "cpu").expand(B, H, L, S)
    # the selector key holds most of the weight wherever the mask leaves it open
    sel = (srec == 3) & torch.gather(opened, 3, pi[..., None])[..., 0]
    p_sel = torch.gather(fw["p"], 3, pi[..., None])[..., 0]
    assert bool((p_sel[sel] > 0.5).all()), (c.name, float(p_sel[sel].min()))
    assert L < 7 or bool((srec == 3).any())
    # ramp rows: the per-chunk maximum of the scores rises (falls) in every chunk
    s = (ac.heads(t["q"], H).double() / 4) @ ac.heads(t["k"], H).double().transpose(-1, -2)
    pad = torch.full((B, H, L, -S % 32), NEG, dtype=torch.float64)
    cmax = torch.cat([s, pad], -1).view(B, H, L, -1, 32).amax(-1)
    step = cmax[..., 1:] - cmax[..., :-1]
    up = (ac.heads(t["q"], H)[..., 1] > 0)[..., None]
    ramp = (srec == 6)[..., None].expand_as(step)
    assert bool((torch.where(up, step, -step)[ramp] > 0).all()), (c.name, "a ramp row's chunk maximum is not monotone")
    # offset rows
    off = (srec == 4) | (srec == 5)
    assert bool((fw["lse"][off].abs() >= 40).all()), (c.name, float(fw["lse"][off].abs().min()))
    assert float(fw["amp"].max()) < 400, (c.name, float(fw["amp"].max()))
    if not c.masked:
        return
    mask, mrec = t["mask"], t["mrec"]
    nsplit, kps, empty = ac.case_plan(c)
    assert S <= 5 or bool(mask[:, 5, :].all())
    for b in range(B):
        for i in range(L):
            col, r = mask[b, :, i], int(mrec[b, i])
            if r == 0:
                assert int(col.sum()) == (1 if S > 5 else 0)
            if r == 2:
                assert int((~col).sum()) == 1
            if r == 3:
                assert bool(col[:32].all()) and not bool(col[32:].all()), (c.name, b, i)
            if r == 4:
                dead = [sp for sp in range(nsplit - empty) if bool(col[sp * kps:(sp + 1) * kps].all())]
                assert dead and not bool(col.all()), (c.name, b, i)
            if r == 5:
                assert bool(col.all())
    if L >= 7 and S > 32:
        assert 3 in mrec
    if L >= 7 and nsplit - empty > 1:
        assert 4 in mrec


@pytest.mark.parametrize("c", _all_cases(), ids=_all_ids())
def test_count_mode_inputs_are_exact(c):
    if not c.masked and not c.count_mode:
        return
    t = ac.count_inputs(c)
    sums, n = ac.ref_count(t["v"], t["mask"], c.H, c.L)
    assert bool((torch.log2(n) == torch.log2(n).round()).all()) and float(n.min()) >= 1
    if c.masked and c.L > int(math.log2(c.S)):
        assert float(n.max()) == 2 ** int(math.log2(c.S)) and float(n.min()) == 1
    assert ac.largest_count_sum(t["v"], t["mask"], c.H, c.L) < ac.EXACT_LIMIT
    assert bool((sums == sums.round()).all()) and not bool(t["q"].any())


# ------------------------------------------------------------------------------------------------- f32 evaluation
def _combine4(parts):
    """Partials added as the combine and dq-reduce kernels do: four interleaved groups, then (g0 + g1) + (g2 + g3)."""
    groups = []
    for g in range(4):
        acc = torch.zeros_like(parts[0])
        for x in parts[g::4]:
            acc = acc + x
        groups.append(acc)
    return (groups[0] + groups[1]) + (groups[2] + groups[3])


def f32_forward(t, c, masked=None, alpha_one=None, pattern_split=None):
    """(o [L, B, E], lse [B * H, L]) in the kernels' partition.  masked: bool [B, H | 1, L, S] in place of the case's mask;
    alpha_one = (split, chunk): that chunk rescales by 1; pattern_split: that split's partial holds the workspace pattern."""
    L, S, B, H = c.L, c.S, c.B, c.H
    nsplit, kps, _ = ac.case_plan(c)
    qh = ac.heads(t["q"], H) * 0.25
    kh, vh = ac.heads(t["k"], H), ac.heads(t["v"], H)
    if masked is None:
        masked = ac._masked(t["mask"], B, L, S, "cpu")
    parts = []
    for sp in range(nsplit):
        kb, ke = sp * kps, min(sp * kps + kps, S)
        m = torch.full((B, H, L), NEG, dtype=F32)
        l, o = torch.zeros((B, H, L), dtype=F32), torch.zeros((B, H, L, ac.HD), dtype=F32)
        for ci, key0 in enumerate(range(kb, ke, 32)):
            k1 = min(key0 + 32, ke)
            s = (qh @ kh[:, :, key0:k1].transpose(-1, -2)).masked_fill(masked[..., key0:k1], NEG)
            m_new = torch.maximum(m, s.amax(-1))
            m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.ones_like(m) if alpha_one == (sp, ci) else torch.exp(m - m_safe)
            pe = torch.exp(s - m_safe[..., None])
            l = l * alpha + pe.sum(-1)
            o = o * alpha[..., None] + pe @ vh[:, :, key0:k1]
            m = m_new
        if pattern_split == sp:
            m, l, o = torch.full_like(m, WS_WORD), torch.full_like(l, WS_WORD), torch.full_like(o, WS_WORD)
        parts.append((o, m, l))
    if not c.masked:
        o, m, l = parts[0]
        return ac.unheads(o * (1.0 / l)[..., None]), (m + torch.log(l)).reshape(B * H, L)
    M = torch.stack([m for _, m, _ in parts]).amax(0)
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    w = [torch.exp(m - Ms) for _, m, _ in parts]
    Lsum = _combine4([l * wi for (_, _, l), wi in zip(parts, w)])
    acc = _combine4([o * wi[..., None] for (o, _, _), wi in zip(parts, w)])
    live = Lsum > 0
    o = torch.where(live[..., None], acc / Lsum[..., None], torch.zeros_like(acc))
    lse = torch.where(live, Ms + torch.log(Lsum), torch.full_like(Ms, float("inf")))
    return ac.unheads(o), lse.reshape(B * H, L)


def f32_backward(t, c, o32, lse32, masked=None, no_D=False):
    """(dq [L, B, E], dk, dv [S, B, E]) in the kernels' partition from the f32 o and lse."""
    L, S, B, H = c.L, c.S, c.B, c.H
    nsplit, kps, _ = ac.case_plan(c)
    qs, kh, vh = ac.heads(t["q"], H) * 0.25, ac.heads(t["k"], H), ac.heads(t["v"], H)
    dOh, oh = ac.heads(t["dO"], H), ac.heads(o32, H)
    if masked is None:
        masked = ac._masked(t["mask"], B, L, S, "cpu")
    D = torch.zeros((B, H, L), dtype=F32)
    for d in range(ac.HD):
        D = D + dOh[..., d] * oh[..., d]
    if no_D:
        D = torch.zeros_like(D)
    lse = lse32[:, :L].reshape(B, H, L)
    dk, dv = torch.zeros((B, H, S, ac.HD), dtype=F32), torch.zeros((B, H, S, ac.HD), dtype=F32)
    parts = []
    for sp in range(nsplit):
        kb, ke = sp * kps, min(sp * kps + kps, S)
        waves = [torch.zeros((B, H, L, ac.HD), dtype=F32) for _ in range(4)]
        for ci, key0 in enumerate(range(kb, ke, 32)):
            k1 = min(key0 + 32, ke)
            kc, vc = kh[:, :, key0:k1], vh[:, :, key0:k1]
            s = qs @ kc.transpose(-1, -2)
            p = torch.exp(s - lse[..., None]).masked_fill(masked[..., key0:k1].expand_as(s), 0.0)
            ds = p * (dOh @ vc.transpose(-1, -2) - D[..., None])
            w = ci % 4 if c.masked else 0
            waves[w] = waves[w] + (ds * 0.25) @ kc
            if c.masked:
                dv[:, :, key0:k1] = p.transpose(-1, -2) @ dOh
                dk[:, :, key0:k1] = ds.transpose(-1, -2) @ qs
            else:
                for q0 in range(0, L, 32):
                    dv[:, :, key0:k1] += p[:, :, q0:q0 + 32].transpose(-1, -2) @ dOh[:, :, q0:q0 + 32]
                    dk[:, :, key0:k1] += ds[:, :, q0:q0 + 32].transpose(-1, -2) @ qs[:, :, q0:q0 + 32]
        parts += waves
    dq = _combine4(parts) if c.masked else parts[0]
    return ac.unheads(dq), ac.unheads(dk), ac.unheads(dv)


def _refs(c, t):
    """The float64 forward reference and the backward reference on its own rounded o and lse."""
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
    o32, lse32 = ac.saved_forward(fw, ac.lse_stride(c.L))
    return fw, o32, lse32, ac.ref_backward(t["q"], t["k"], t["v"], t["mask"], t["dO"], o32, lse32, c.H)


WORST = {}


@pytest.mark.parametrize("c", _all_cases(), ids=_all_ids())
def test_an_f32_evaluation_uses_at_most_half_of_every_bound(c):
    t = ac.attn_inputs(c)
    fw, o32, lse32, refs = _refs(c, t)
    o, lse = f32_forward(t, c)
    fr = ac.forward_fractions(o, lse, fw)
    assert ac.dead_rows_exact(o, lse, fw)
    fr.update(ac.backward_fractions(*f32_backward(t, c, o32, lse32), refs))
    own = ac.ref_backward(t["q"], t["k"], t["v"], t["mask"], t["dO"], o, lse, c.H)          # chained: its own o and lse
    fr.update({k + " chained": v for k, v in ac.backward_fractions(*f32_backward(t, c, o, lse), own).items()})
    w = WORST.setdefault("cross" if c.masked else "self", {})
    for k, v in fr.items():
        w[k] = max(w.get(k, 0.0), v)
    assert max(fr.values()) <= HALF, (c.name, fr)


@pytest.mark.parametrize("c", _all_cases(), ids=_all_ids())
def test_an_f32_evaluation_gives_count_mode_within_its_bound(c):
    if not c.masked and not c.count_mode:
        return
    t = ac.count_inputs(c)
    o, lse = f32_forward(t, c)
    fr = ac.count_fractions(o, lse, *ac.ref_count(t["v"], t["mask"], c.H, c.L))
    assert max(fr.values()) <= 1.0, (c.name, fr)
    # one key dropped from one row of one head is seen
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
    j = int(fw["p"][0, 0, c.L - 1].argmax())
    if float(ac.heads(t["v"], c.H)[0, 0, j].abs().max()) > 0 and float(fw["p"][0, 0, c.L - 1, j]) < 1:
        masked = ac._masked(t["mask"], c.B, c.L, c.S, "cpu").expand(c.B, c.H, c.L, c.S).clone()
        masked[0, 0, c.L - 1, j] = True
        bad = ac.count_fractions(*f32_forward(t, c, masked=masked), *ac.ref_count(t["v"], t["mask"], c.H, c.L))
        assert max(bad.values()) > 1.0, (c.name, bad)


def test_print_the_host_fractions():
    """A record, not a check (after the half-bound test of every case): the largest fraction of each bound."""
    for fam, w in WORST.items():
        print(f"\n{fam:<8} " + "  ".join(f"{k} {v:.3f}" for k, v in w.items()))


# ------------------------------------------------------------------------------------------------- planted errors
def _rejected_forward(o, lse, fw):
    fr = ac.forward_fractions(o, lse, fw)
    return max(fr.values()) > 1.0 or not ac.dead_rows_exact(o, lse, fw)


def _rejected_backward(got, refs):
    return max(ac.backward_fractions(*got, refs).values()) > 1.0


def _full_mask(c, t):
    return ac._masked(t["mask"], c.B, c.L, c.S, "cpu").expand(c.B, c.H, c.L, c.S).clone()


def _drop_median_key(c, t, fw):
    """A mask in which one head of batch 0 loses the open key of median p of one normal or flat row with at least two
    open keys (the median weight of a sharp, selector or ramp row is below every bound by construction); None where the
    case has no such row."""
    masked = _full_mask(c, t)
    n_open = (~masked[0]).sum(-1)
    rows = [(h, i) for h in range(c.H) for i in range(c.L) if n_open[h, i] >= 2 and int(t["srec"][0, h, i]) in (0, 2)]
    if not rows:
        return None
    h, i = rows[0]
    keys = (~masked[0, h, i]).nonzero()[:, 0]
    order = fw["p"][0, h, i, keys].argsort()
    masked[0, h, i, keys[order[len(order) // 2]]] = True
    return masked


def _tile1_for_tile0(c, t, fw):
    if c.L < 33 or not c.masked:
        return None
    masked = _full_mask(c, t)
    src = torch.zeros_like(masked[:, :, 0:32])                      # bits of queries >= L are clear
    src[:, :, :min(64, c.L) - 32] = masked[:, :, 32:64]
    masked[:, :, 0:32] = src
    return None if torch.equal(masked, _full_mask(c, t)) else masked


def _group0_for_group1(c, t, fw):
    if c.L < 129 or not c.masked:
        return None
    masked = _full_mask(c, t)
    masked[:, :, 128:] = masked[:, :, :c.L - 128]
    return None if torch.equal(masked, _full_mask(c, t)) else masked


def _planted_forward(c, t, fw):
    """name -> (o, lse) of an f32 evaluation with that error, for every error that applies to the case."""
    nsplit, kps, empty = ac.case_plan(c)
    B, H, L = c.B, c.H, c.L
    out = {}
    for name, make in (("key dropped", _drop_median_key), ("tile 1 mask for tile 0", _tile1_for_tile0),
                       ("group 0 mask for group 1", _group0_for_group1)):
        masked = make(c, t, fw)
        if masked is not None:
            out[name] = f32_forward(t, c, masked=masked)
    if min(kps, c.S) > 32 and L >= 7:
        out["alpha = 1 in one chunk"] = f32_forward(t, c, alpha_one=(0, 1))
    live_minus = bool(((t["srec"] == 5) & ~torch.isinf(fw["lse"])).any())
    if empty and live_minus:
        out["empty split holds the pattern"] = f32_forward(t, c, pattern_split=nsplit - 1)
    o, lse = f32_forward(t, c)
    out["lse off by 2^-16 amp"] = (o, lse + (2.0 ** -16 * fw["amp"]).reshape(B * H, L).float())
    dead = torch.isinf(fw["lse"][:, 0]).nonzero()
    if len(dead) and bool(t["v"][0, int(dead[0, 0])].any()):
        b, i = int(dead[0, 0]), int(dead[0, 1])
        o2 = o.clone()
        o2[i, b, :ac.HD] = t["v"][0, b, :ac.HD]
        out["a dead row given v[0]"] = (o2, lse)
    if H >= 2 and bool((~torch.isinf(fw["lse"][:, :2])).any()):
        oh, lh = ac.heads(o, H).clone(), lse.reshape(B, H, L).clone()
        oh[:, 1], lh[:, 1] = oh[:, 0], lh[:, 0]
        out["head 0 written to head 1"] = (ac.unheads(oh), lh.reshape(B * H, L))
    return out


def _planted_backward(c, t, fw, o32, lse32, got):
    """name -> (dq, dk, dv) of an f32 evaluation with that error, for every error that applies to the case."""
    dq, dk, dv = got
    live = bool((~torch.isinf(fw["lse"][:, :2])).any())
    back = {}
    if live:
        back["D left out of ds"] = f32_backward(t, c, o32, lse32, no_D=True)
    for name, make in (("key dropped", _drop_median_key), ("tile 1 mask for tile 0", _tile1_for_tile0),
                       ("group 0 mask for group 1", _group0_for_group1)):
        masked = make(c, t, fw)
        if masked is not None:
            back[name] = f32_backward(t, c, o32, lse32, masked=masked)
    if c.S >= 2 and c.L >= 7:
        dk2, dv2 = dk.clone(), dv.clone()
        dk2[[c.S - 1, c.S - 2]], dv2[[c.S - 1, c.S - 2]] = dk[[c.S - 2, c.S - 1]], dv[[c.S - 2, c.S - 1]]
        back["last two keys swapped"] = (dq, dk2, dv2)
    if c.H >= 2 and live:
        dvh = ac.heads(dv, c.H).clone()
        dvh[:, 1] = dvh[:, 0]
        back["head 0 written to head 1"] = (dq, dk, ac.unheads(dvh))
    return back


@pytest.mark.parametrize("c", _all_cases(), ids=_all_ids())
def test_planted_errors_are_rejected(c):
    t = ac.attn_inputs(c)
    fw, o32, lse32, refs = _refs(c, t)
    assert not _rejected_forward(*f32_forward(t, c), fw)
    planted = _planted_forward(c, t, fw)
    missed = [name for name, (o, lse) in planted.items() if not _rejected_forward(o, lse, fw)]
    assert not missed, (c.name, missed)
    got = f32_backward(t, c, o32, lse32)
    assert not _rejected_backward(got, refs)
    back = _planted_backward(c, t, fw, o32, lse32, got)
    missed = [name for name, bad in back.items() if not _rejected_backward(bad, refs)]
    assert not missed, (c.name, missed)


def test_every_planted_error_applies_to_some_case():
    names = set()
    for key in ((100, 1100, 1, 8), (150, 999, 2, 8)):
        c = next(c for c in ac.CROSS_CASES if (c.L, c.S, c.B, c.H) == key)
        t = ac.attn_inputs(c)
        fw, o32, lse32, _ = _refs(c, t)
        names |= set(_planted_forward(c, t, fw)) | set(_planted_backward(c, t, fw, o32, lse32, f32_backward(t, c, o32, lse32)))
    assert names == {"key dropped", "tile 1 mask for tile 0", "group 0 mask for group 1", "alpha = 1 in one chunk",
                     "empty split holds the pattern", "lse off by 2^-16 amp", "D left out of ds", "last two keys swapped",
                     "a dead row given v[0]", "head 0 written to head 1"}
