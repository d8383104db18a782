"""The case tables of tests/decoder_cases.py are what they claim to be (no GPU): unique names, every size the kernels of
csrc/decoder.hip branch on, exact cases below EXACT_LIMIT, LayerNorm rows inside LN_CONDITION_CAP; the comparators accept
an evaluation in the kernels' arithmetic and reject planted errors.

The kernels' arithmetic on the CPU, in f32: a linear product is four wave partials (wave w owns the 32-wide chunks
w, w + 4, ... of the reduction dimension) added in wave order, then bias, accumulate, dx_add, dx_add2, ReLU in the order
of tile_reduce_store; db is four wave partials too; dgamma / dbeta are 16 wave partials (wave w owns rows w, w + 16, ...
of its block) added in wave order, then the G block partials in block order; the LayerNorm statistics are per-lane sums
over columns l, l + 64, ... followed by the xor butterfly 32, 16, ..., 1.

Branches of decoder.hip and the cases that reach them:
  layernorm_fwd_kernel<PER>        PER = 1, 2, 3, 4, 6, 8: d = 64 ... 512; res / no res; a last workgroup with 1, 2, 3
                                   and 4 live waves (rows 1, 5 / 129, 3, 4 / 100, ...)
  layernorm_bwd_kernel<PER>        prefetch path (a workgroup owns <= 128 rows at d <= 128: rows 1 ... 128, and the
                                   second workgroup of 1025, 1152; <= 64 rows at d >= 192: rows 1, 5, 64 and the second
                                   workgroup of 1025, 1088) and the row loop (129, 1024, 1153 / 65, 1024, 1089), with and
                                   without dx_add; gridDim.x == 1 with accumulate 0 / 1; gridDim.x == 2, 3 (2500 rows)
  layernorm_bwd_final_kernel       accumulate 0 / 1, G = 2 and 3
  linear_fwd_kernel                1, 3, 4, 5 and 32 chunks (idle waves at K = 32, 96; wave 0 with two chunks at 160);
                                   x2 / no x2, x2_cols 0, 2E, N; split 0, E, N; bias / none; relu; rows beyond M kept,
                                   zeroed up to M_pad and left alone beyond it
  linear_dx_tile<EX>               the same chunk counts over N (the in-flight prefetch of the next chunk: N = 160 is not
                                   in the table, N = 1024 has eight chunks per wave); ymask; dx_add, dx_add2, dx_b
  linear_dw_tile<EX>               M = 1 ... 129: one to five 32-row blocks (wave 0 takes a second block at 129), the
                                   128-row step from both sides through usc_qkv_proj_bwd and usc_linear_bwd at M = 100 /
                                   129; ymask, x2; db / none, accumulate 0 / 1
  qkv_bwd_kernel                   E = 32, 96, 128; pos, dres, dx_b, db each present and absent
  col_sum_partial / final          one to 17 row blocks (more than 16: lane 0 adds two partials), a ragged last block,
                                   c below, at and above the 16- and 64-column workgroup widths, no rows at all
Compiled and out of reach of the table: nothing.  The kernels also take wider matrices (the table stops at 1024, the
decoder's FFN width) and LayerNorm row counts above 2500.  One thing the bounds do not see: with |x| + |mean| in place of
|x - mean|, the rows of recipe 2 (mean 100, std 0.05) carry a dx bound of some hundred units and lift the dgamma bound
of every column; on those rows a wrong value shows in dbeta and in the neighbouring recipes' rows, not in dx."""
import math

import pytest
import torch

import decoder_cases as dc

F32 = torch.float32


def _merge(worst, fr, prefix=""):
    for k, v in fr.items():
        worst[prefix + k] = max(worst.get(prefix + k, 0.0), v)


# ------------------------------------------------------------------------------------------------- the tables
def test_case_names_are_unique():
    for cases in [dc.LN_CASES, dc.COLSUM_CASES] + list(dc.LIN_CASES.values()):
        names = [c.name for c in cases]
        assert len(names) == len(set(names)), names


def test_the_table_covers_the_sizes_the_kernels_branch_on():
    ln = dc.LN_CASES
    assert {c.d for c in ln} == set(dc.LN_DIMS)
    assert {c.rows for c in ln if c.d == 128} == set(dc.LN_ROWS_NARROW) == {1, 3, 4, 5, 100, 128, 129, 1024, 1025, 1152, 1153, 2500}
    assert {c.rows for c in ln if c.d == 192} == set(dc.LN_ROWS_WIDE) == {1, 5, 64, 65, 1024, 1025, 1088, 1089}
    assert {c.rows for c in ln if c.d <= 128} <= set(dc.LN_ROWS_NARROW)
    assert {c.rows for c in ln if c.d >= 192} <= set(dc.LN_ROWS_WIDE)
    assert max(c.rows for c in ln) == 2500
    for d in dc.LN_DIMS:
        assert {c.launches for c in ln if c.d == d} == {1, 2}, d
    for launches in (1, 2):
        for flag in ("res", "dx_add", "accumulate", "repeat", "shift"):
            assert {getattr(c, flag) for c in ln if c.launches == launches} == {False, True}, (launches, flag)
    assert {c.accumulate for c in ln if c.rows == 1025} == {False, True}            # one row in the last workgroup
    for lo, hi in ((128, 129), (64, 65)):                                              # both sides of the prefetch step
        assert any(c.dx_add for c in ln if c.rows in (lo, hi)) and any(not c.dx_add for c in ln if c.rows in (lo, hi))

    shapes = {(M, N, K) for M in (1, 31, 32, 33, 100, 129)
              for (N, K) in ((32, 32), (32, 96), (96, 160), (128, 128), (1024, 128), (128, 1024))}
    for fam in ("fwd", "bwd_plain", "bwd_ex"):
        assert {(c.M, c.N, c.K) for c in dc.LIN_CASES[fam]} == shapes, fam
    fwd = dc.LIN_CASES["fwd"]
    assert {(c.x2, c.b, c.relu) for c in fwd} == {(a, b, r) for a in (False, True) for b in (False, True) for r in (False, True)}
    for K in (32, 96, 160, 1024):
        assert {c.x2 for c in fwd if c.K == K} == {False, True}, K
    assert {(c.M, c.M_pad) for c in dc.LIN_CASES["pad"]} == {(100, 128), (100, 110), (1, 64), (33, 33), (32, 33)}
    assert {c.x2 for c in dc.LIN_CASES["pad"]} == {False, True}
    split = dc.LIN_CASES["split"]
    assert {(c.K, c.x2_cols) for c in split if c.split == c.K and c.b and c.x2} == \
        {(E, cols) for E in (32, 96, 128) for cols in (0, 2 * E, 3 * E)}
    assert all(c.N == 3 * c.K for c in split) and any(c.split == c.N for c in split) and any(not c.b for c in split)
    assert 32 in {c.split for c in split}

    plain, ex = dc.LIN_CASES["bwd_plain"], dc.LIN_CASES["bwd_ex"]
    assert all(not c.operands and not c.x2 for c in plain)
    assert {c.operands for c in ex} == {(o,) for o in dc.EX_OPERANDS} | {dc.EX_OPERANDS}
    for cases in (plain, ex):
        assert {c.outputs for c in cases} == set(dc.OUTPUTS)
        assert {(c.outputs, c.accumulate) for c in cases if c.want_dW} == \
            {(o, a) for o in ("dW+db", "dW", "all") for a in (False, True)}
        assert {c.M for c in cases if c.want_db and c.accumulate} >= {1, 100, 129}
        for M in (1, 31, 32, 33, 100, 129):
            assert any(c.want_dx for c in cases if c.M == M) and any(c.want_dW for c in cases if c.M == M), M
        for nk in ((32, 32), (32, 96), (96, 160), (128, 128), (1024, 128), (128, 1024)):
            assert any(c.want_dx for c in cases if (c.N, c.K) == nk) and any(c.want_db for c in cases if (c.N, c.K) == nk), nk
    for ops in {c.operands for c in ex}:
        assert any(c.want_dx for c in ex if c.operands == ops), ops
    assert all(c.want_dx for c in ex if set(c.operands) & {"dx_add", "dx_add2", "dx_b"})
    assert any(c.want_dW and c.M >= 100 for c in ex if c.operands == ("y_relu",))
    assert any(c.want_dW for c in ex if c.operands == ("x2",))

    qkv = dc.LIN_CASES["qkv"]
    assert {(c.K, c.M) for c in qkv} == {(E, M) for E in (32, 96, 128) for M in (1, 100, 129)}
    for E in (32, 96, 128):
        assert {c.accumulate for c in qkv if c.K == E} == {False, True}
    for op in ("pos", "dres", "dx_b", "db"):
        assert {c.has(op) for c in qkv} == {False, True}, op
        assert {c.has(op) for c in qkv if c.M >= 100} == {False, True}, op
    assert any(c.has("db") and c.accumulate for c in qkv) and any(c.has("db") and not c.accumulate for c in qkv)

    cs = dc.COLSUM_CASES
    assert {(c.n, c.c) for c in cs if c.n} == {(n, c) for n in (63, 64, 65, 1025) for c in (1, 17, 65)}
    assert {c.accumulate for c in cs if c.n == 0} == {False, True} and {c.accumulate for c in cs if c.n == 1025} == {False, True}
    # nothing larger than the largest sizes named
    assert max(max(c.M, c.M_pad) for c in dc.all_lin_cases()) == 129 and max(max(c.N, c.K) for c in dc.all_lin_cases()) == 1024


def test_exact_cases_keep_every_partial_sum_below_the_limit():
    worst = 0.0
    for c in dc.all_lin_cases():
        t = dc.lin_inputs(c, "exact")
        worst = max(worst, dc.largest_partial_sum(_lin_refs(c, t)))
    for c in dc.COLSUM_CASES:
        t = dc.colsum_inputs(c, "exact")
        worst = max(worst, float(dc.ref_col_sum(t["x"], t["before"])[1].max()))
    assert worst < dc.EXACT_LIMIT
    print(f"largest sum of absolute terms over the exact cases: {worst:.0f} (limit 2**24)")


def test_layernorm_rows_respect_the_condition_cap():
    assert dc.LN_CONDITION_CAP <= dc.CONDITION_CAP
    worst = 0.0
    for c in dc.LN_CASES:
        k = dc.ln_condition(dc.ln_inputs(c)["v"])
        worst = max(worst, k)
        assert k <= dc.LN_CONDITION_CAP, (c.name, k)
    print(f"largest mean|v|^2 / (var + eps) of the table: 2**{math.log2(worst):.1f}")
    # the recipes the issue names, per row: a large mean with a small spread, a constant row, spread << sqrt(eps), integers
    v = dc.ln_rows(64, 128, 5).double()
    sd = v.var(1, unbiased=False).sqrt()
    assert bool(((v.mean(1).abs() > 90) & (sd < 0.1)).any()) and bool(((sd == 0) & (v[:, 0] != 0)).any())
    assert bool(((sd > 0) & (sd < 0.1 * math.sqrt(dc.EPS))).any()) and bool(((v == v.round()).all(1) & (sd > 0)).any())
    # with a residual the constant and the integer rows stay exact
    c = next(c for c in dc.LN_CASES if c.res and c.rows >= 100)
    t = dc.ln_inputs(c)
    vv = t["v"].double()
    assert bool((vv.var(1, unbiased=False) == 0).any()) and bool(((vv == vv.round()).all(1)).any()) and bool(t["res"].any())


# ------------------------------------------------------------------------------------------------- emulation: linears
def _waves(parts):
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def emu_product(a, bt):
    """a [P, R] @ bt [R, Q] in f32 in the kernels' partition of R: wave w sums the 32-wide chunks w, w + 4, ... in order,
    the four partial tiles are added in wave order."""
    R = a.shape[1]
    parts = []
    for w in range(4):
        acc = torch.zeros((a.shape[0], bt.shape[1]), dtype=F32)
        for c in range(w, -(-R // 32), 4):
            acc = acc + a[:, 32 * c:32 * c + 32] @ bt[32 * c:32 * c + 32]
        parts.append(acc)
    return _waves(parts)


def emu_colsum_waves(g, skip_half=False):
    """db of linear_dw_tile: wave w sums the rows of its 32-row blocks, the four sums are added in wave order.
    skip_half: the lanes 32 ... 63 (rows m = 4 ... 7 mod 8) are left out."""
    M = g.shape[0]
    if skip_half:
        g = torch.where(((torch.arange(M) % 8) < 4)[:, None], g, torch.zeros_like(g))
    parts = []
    for w in range(4):
        acc = torch.zeros(g.shape[1], dtype=F32)
        for c in range(w, -(-M // 32), 4):
            acc = acc + g[32 * c:32 * c + 32].sum(0)
        parts.append(acc)
    return _waves(parts)


def emu_fwd(c, t, x2_cols=None, pad_garbage=False):
    x, W = t["x"], t["W"]
    y = emu_product(x, W.T.contiguous())
    if t["x2"] is not None:
        cols = x2_cols if x2_cols is not None else (c.x2_cols if c.family == "split" else c.N)
        y2 = emu_product(x + t["x2"], W.T.contiguous())
        y = torch.where((torch.arange(c.N) < cols)[None], y2, y)
    if t["b"] is not None:
        y = y + t["b"]
    if c.relu:
        y = y.clamp_min(0.0)
    if c.family == "pad":
        tail = torch.zeros((c.M_pad - c.M, c.N))
        if pad_garbage and c.M_pad > c.M:
            tail[0] = y[0]
        y = torch.cat([y, tail])
    return y


def emu_bwd(c, t, ge=False, skip_half=False, ignore_acc=False):
    g = t["dy"]
    if t["y_relu"] is not None:
        g = torch.where((t["y_relu"] >= 0) if ge else (t["y_relu"] > 0), g, torch.zeros_like(g))
    out = {}
    acc = c.accumulate and not ignore_acc
    if c.want_dx:
        o = emu_product(g, t["W"])
        if t["dx_add"] is not None:
            o = o + t["dx_add"]
        if c.has("dx_b"):
            out["dx_b"] = o
        out["dx"] = o + t["dx_add2"] if t["dx_add2"] is not None else o
    if c.want_dW:
        xs = t["x"] + t["x2"] if t["x2"] is not None else t["x"]
        dW = emu_product(g.T.contiguous(), xs)
        out["dW"] = dW + t["dW0"] if acc else dW
    if c.want_db:
        db = emu_colsum_waves(g, skip_half)
        out["db"] = t["db0"] + db if acc else db
    return out


def emu_qkv(c, t):
    d3, W = t["dy3"], t["W"].view(3, c.K, c.K)
    qk = emu_product(torch.cat([d3[0], d3[1]], 1), torch.cat([W[0], W[1]]))       # (an order of its own: chunks of q then k)
    vv = emu_product(d3[2], W[2])
    out = dict(dx=qk + vv)
    if t["dres"] is not None:
        out["dx"] = out["dx"] + t["dres"]
    if c.has("dx_b"):
        out["dx_b"] = qk
    xs = [t["x"] + t["pos"] if t["pos"] is not None and j < 2 else t["x"] for j in range(3)]
    dW = torch.cat([emu_product(d3[j].T.contiguous(), xs[j]) for j in range(3)])
    out["dW"] = dW + t["dW0"] if c.accumulate else dW
    if c.has("db"):
        db = torch.cat([emu_colsum_waves(d3[j]) for j in range(3)])
        out["db"] = t["db0"] + db if c.accumulate else db
    return out


def _lin_refs(c, t):
    if c.family in ("fwd", "pad", "split"):
        ref, mag = dc.ref_linear_fwd(t["x"], t["x2"], t["W"], t["b"], c.relu, c.x2_cols if c.family == "split" else None)
        if c.family == "pad":
            z = torch.zeros((c.M_pad - c.M, c.N), dtype=torch.float64)
            ref, mag = torch.cat([ref, z]), torch.cat([mag, z])
        return dict(y=(ref, mag))
    if c.family == "qkv":
        return dc.ref_qkv_bwd(t["dy3"], t["x"], t["pos"], t["W"], t["dres"], t["dW0"] if c.accumulate else None,
                              t["db0"] if c.accumulate else None)
    return dc.ref_linear_bwd(t["dy"], t["y_relu"], t["x"], t["x2"], t["W"], t["dx_add"], t["dx_add2"],
                             t["dW0"] if c.accumulate else None, t["db0"] if c.accumulate else None)


def _lin_emu(c, t, **kw):
    if c.family in ("fwd", "pad", "split"):
        return dict(y=emu_fwd(c, t, **kw))
    return emu_qkv(c, t) if c.family == "qkv" else emu_bwd(c, t, **kw)


@pytest.mark.parametrize("mode", dc.MODES)
def test_comparators_accept_the_linear_kernels_arithmetic(mode):
    worst = {}
    for c in dc.all_lin_cases():
        t = dc.lin_inputs(c, mode)
        fr = dc.fractions(mode, _lin_emu(c, t), _lin_refs(c, t))
        assert max(fr.values()) <= 1.0, (c.family, c.name, mode, fr)
        _merge(worst, fr, c.family + " ")
    if mode == "bounded":
        print("linear kernels, f32 in the kernels' partition on the CPU, largest fraction of each bound over every case:")
        print("  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_split_layout_is_piece_major():
    y = torch.arange(2 * 6, dtype=F32).view(2, 6)
    assert dc.split_layout(y, 3).tolist() == [[0, 1, 2], [6, 7, 8], [3, 4, 5], [9, 10, 11]]
    assert torch.equal(dc.split_layout(y, 6), y)


# ------------------------------------------------------------------------------------------------- planted errors: linears
def _rejects(mode, y, ref, mag):
    return dc.fraction(mode, y, ref, mag) > 1.0


@pytest.mark.parametrize("mode", dc.MODES)
def test_comparators_reject_planted_errors_in_the_linears(mode):
    seen = set()
    for c in dc.all_lin_cases():
        t = dc.lin_inputs(c, mode)
        refs, emu = _lin_refs(c, t), _lin_emu(c, t)
        if c.family in ("fwd", "pad", "split"):
            ref, mag = refs["y"]
            y = emu["y"]
            # one term dropped from one output element (the last row, the last column: the far corner of the last tile)
            m, n = c.M - 1, c.N - 1
            k = int(torch.nonzero(t["x"][m] * t["W"][n]).flatten()[-1]) if bool((t["x"][m] * t["W"][n]).any()) else None
            live = not c.relu or float(ref[m, n]) > 0
            if k is not None and live and float(ref[m, n] - t["x"][m, k].double() * t["W"][n, k].double()) > 0:
                bad = y.clone()
                bad[m, n] -= t["x"][m, k] * t["W"][n, k]
                assert _rejects(mode, bad, ref, mag), (c.name, "one term dropped")
                seen.add("term")
            # one row / one column of a tile shifted by one
            if c.M >= 32:
                bad = y.clone()
                bad[31] = y[30]
                assert _rejects(mode, bad, ref, mag), (c.name, "row 31 holds row 30")
                seen.add("row")
            bad = y.clone()
            bad[:, 31] = y[:, 30]
            if c.M > 1 or not torch.equal(y[:, 31], y[:, 30]):
                assert _rejects(mode, bad, ref, mag), (c.name, "column 31 holds column 30")
                seen.add("col")
            if c.family == "pad" and c.M_pad > c.M and bool(y[0].any()):
                assert _rejects(mode, emu_fwd(c, t, pad_garbage=True), ref, mag), (c.name, "a padding row left non-zero")
                seen.add("pad")
            if c.family == "split" and c.x2 and c.x2_cols < c.N:
                leak = emu_fwd(c, t, x2_cols=c.x2_cols + 32)
                assert _rejects(mode, leak, ref, mag), (c.name, "x2 leaks into column block x2_cols / 32")
                assert not _rejects(mode, leak[:, :c.x2_cols], ref[:, :c.x2_cols], mag[:, :c.x2_cols])
                seen.add("leak")
            continue
        if c.family == "qkv":
            continue
        if c.want_db and c.M >= 5:
            bad = emu_bwd(c, t, skip_half=True)["db"]
            assert _rejects(mode, bad, *refs["db"]), (c.name, "db misses the rows m = 4 ... 7 mod 8")
            seen.add("half")
        if c.accumulate and c.want_dW:
            bad = emu_bwd(c, t, ignore_acc=True)
            assert _rejects(mode, bad["dW"], *refs["dW"]), (c.name, "accumulate ignored: dW")
            if c.want_db:
                assert _rejects(mode, bad["db"], *refs["db"]), (c.name, "accumulate ignored: db")
            seen.add("acc")
        if c.has("y_relu"):
            bad = emu_bwd(c, t, ge=True)
            assert any(_rejects(mode, bad[k], *refs[k]) for k in bad), (c.name, "mask by >=")
            if c.M >= 31:                                         # (one row: a column may hold no +0.0 / -0.0 at all)
                assert all(_rejects(mode, bad[k], *refs[k]) for k in bad), (c.name, "mask by >=")
            seen.add("ge")
        if c.want_dx and c.M >= 32:
            bad = emu["dx"].clone()
            bad[31] = emu["dx"][30]
            assert _rejects(mode, bad, *refs["dx"]), (c.name, "dx row 31 holds row 30")
    assert seen == {"term", "row", "col", "pad", "leak", "half", "acc", "ge"}, seen


# ------------------------------------------------------------------------------------------------- emulation: LayerNorm
LANES = torch.arange(64)


def wave_sum(t):
    """[rows, d] -> [rows]: lane l adds columns l, l + 64, ... in order, then wave_reduce_addf's butterfly (common.h)."""
    s = torch.zeros((t.shape[0], 64), dtype=F32)
    for j in range(t.shape[1] // 64):
        s = s + t[:, 64 * j:64 * j + 64]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    assert bool((s == s[:, :1]).all() | torch.isnan(s).all())
    return s[:, 0]


def emu_ln_fwd(t, d):
    v = t["v"]
    mu = wave_sum(v) / torch.tensor(float(d), dtype=F32)
    dev = v - mu[:, None]
    rs = torch.rsqrt(wave_sum(dev * dev) / torch.tensor(float(d), dtype=F32) + torch.tensor(dc.EPS, dtype=F32))
    return dict(mean=mu, rstd=rs, y=dev * rs[:, None] * t["gamma"] + t["beta"])


def emu_block_reduce(terms, before=None, drop_last=False):
    """Column sums of terms [rows, d] in the partition of layernorm_bwd_kernel / layernorm_bwd_final_kernel."""
    rows, d = terms.shape
    if drop_last:
        terms = torch.cat([terms[:-1], torch.zeros((1, d))])
    parts = []
    for r0 in range(0, rows, dc.LN_ROWS_PER_BLOCK):
        blk = terms[r0:r0 + dc.LN_ROWS_PER_BLOCK]
        Q = -(-blk.shape[0] // 16)
        pad = torch.zeros((Q * 16, d), dtype=F32)
        pad[:blk.shape[0]] = blk
        pad = pad.view(Q, 16, d)
        acc = torch.zeros((16, d), dtype=F32)
        for q in range(Q):
            acc = acc + pad[q]
        s = torch.zeros(d, dtype=F32)
        for w in range(16):
            s = s + acc[w]
        parts.append(s)
    total = parts[0]
    if len(parts) > 1:
        total = torch.zeros(d, dtype=F32)
        for p in parts:
            total = total + p
    return total if before is None else before + total


def emu_ln_bwd(c, t, ignore_acc=False, drop_last=False, last_from_first=False):
    x, dy, d = t["v"], t["dy"], c.d
    mu, rs = t["mean32"][:, None], t["rstd32"][:, None]
    if last_from_first:                 # the last row of the last workgroup computed from that workgroup's first row
        r0 = (c.rows - 1) // dc.LN_ROWS_PER_BLOCK * dc.LN_ROWS_PER_BLOCK
        x, dy, mu, rs = x.clone(), dy.clone(), mu.clone(), rs.clone()
        x[-1], dy[-1], mu[-1], rs[-1] = x[r0], dy[r0], mu[r0], rs[r0]
    xh = (x - mu) * rs
    gy = dy * t["gamma"]
    df = torch.tensor(float(d), dtype=F32)
    s1, s2 = wave_sum(gy) / df, wave_sum(gy * xh) / df
    dx = rs * (gy - s1[:, None] - xh * s2[:, None])
    if t["dx_add"] is not None:
        dx = dx + t["dx_add"]
    acc = c.accumulate and not ignore_acc
    return dict(dx=dx, dgamma=emu_block_reduce(dy * xh, t["dgamma0"] if acc else None, drop_last),
                dbeta=emu_block_reduce(dy, t["dbeta0"] if acc else None, drop_last))


def _ln_bwd_refs(c, t):
    return dc.ref_ln_bwd(t["v"], t["dy"], t["mean32"], t["rstd32"], t["gamma"], t["dx_add"],
                         t["dgamma0"] if c.accumulate else None, t["dbeta0"] if c.accumulate else None)


def test_comparators_accept_the_layernorm_arithmetic_within_half_of_the_statistics_bounds():
    worst = {}
    for c in dc.LN_CASES:
        t = dc.ln_inputs(c)
        if c.res:
            assert dc.same_bits(t["v"], (t["x"].double() + t["res"].double()).float())         # sum_out
        st = dc.ref_ln_fwd(t["v"], t["gamma"], t["beta"])
        e = emu_ln_fwd(t, c.d)
        fr = dc.ln_stat_fractions(e["mean"], e["rstd"], st)
        assert max(fr.values()) <= 0.5, (c.name, fr)          # the recipes leave half of each bound to the card
        fr["y"] = dc.fraction("bounded", e["y"], st["y"], st["y_mag"])
        fb = dc.fractions("bounded", emu_ln_bwd(c, t), _ln_bwd_refs(c, t))
        assert max(fr.values()) <= 1.0 and max(fb.values()) <= 1.0, (c.name, fr, fb)
        _merge(worst, fr)
        _merge(worst, fb)
    print("LayerNorm, f32 in the kernels' partition on the CPU, largest fraction of each bound over every case:")
    print("  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_comparators_reject_planted_errors_in_the_layernorm():
    seen = set()
    for c in dc.LN_CASES:
        t = dc.ln_inputs(c)
        refs = _ln_bwd_refs(c, t)
        st = dc.ref_ln_fwd(t["v"], t["gamma"], t["beta"])
        e = emu_ln_fwd(t, c.d)
        # a mean over d - 1 columns (the last lane's last column left out) on the rows where that column is not 0
        short = t["v"].clone()
        short[:, -1] = 0.0
        bad = wave_sum(short) / torch.tensor(float(c.d), dtype=F32)
        rows = t["v"][:, -1].abs() > 1e-3
        if bool(rows.any()):
            fr = dc.ln_stat_fractions(bad[rows], e["rstd"][rows], {k: v[rows] for k, v in st.items() if v.dim() == 1})
            assert fr["mean"] > 1.0, (c.name, "a column left out of the mean")
        # y with the neighbouring row's statistics
        if c.rows > 1:
            yb = (t["v"] - e["mean"].roll(1)[:, None]) * e["rstd"].roll(1)[:, None] * t["gamma"] + t["beta"]
            assert dc.fraction("bounded", yb, st["y"], st["y_mag"]) > 1.0, (c.name, "the neighbouring row's statistics")
        if c.accumulate:
            bad = emu_ln_bwd(c, t, ignore_acc=True)
            assert _rejects("bounded", bad["dgamma"], *refs["dgamma"]) and _rejects("bounded", bad["dbeta"], *refs["dbeta"]), \
                (c.name, "accumulate ignored")
            seen.add(("acc", c.launches))
        if c.rows > 1:
            bad = emu_ln_bwd(c, t, drop_last=True)
            assert _rejects("bounded", bad["dbeta"], *refs["dbeta"]), (c.name, "the last row left out of dbeta")
            bad = emu_ln_bwd(c, t, last_from_first=True)
            if (c.rows - 1) % dc.LN_ROWS_PER_BLOCK:
                # (recipe 2, mean 100 with std 0.05: |x| + |mean| is 4000 spreads, the bound of that row's dx is wide)
                assert _rejects("bounded", bad["dx"], *refs["dx"]) or (c.rows - 1 + c.seed) % dc.N_RECIPES == 2, \
                    (c.name, "the last row computed from the first")
                assert _rejects("bounded", bad["dbeta"], *refs["dbeta"]), (c.name, "the last row computed from the first")
                seen.add(("last", c.rows))
    assert {("acc", 1), ("acc", 2)} <= seen and {("last", 128), ("last", 64), ("last", 1152), ("last", 1088)} <= seen


# ------------------------------------------------------------------------------------------------- column sum
def emu_col_sum(x, before=None):
    n, c = x.shape
    parts = [x[r:r + 64].sum(0) for r in range(0, n, 64)]
    lanes = []
    for ln in range(16):
        s = torch.zeros(c, dtype=F32)
        for p in parts[ln::16]:
            s = s + p
        lanes.append(s)
    t = torch.zeros(c, dtype=F32)
    for s in lanes:
        t = t + s
    return t if before is None else before + t


@pytest.mark.parametrize("mode", dc.MODES)
def test_column_sum_reference_accepts_f32_and_rejects_a_dropped_row_and_an_ignored_accumulate(mode):
    worst = 0.0
    for c in dc.COLSUM_CASES:
        t = dc.colsum_inputs(c, mode)
        before = t["before"] if c.accumulate else None
        ref, mag = dc.ref_col_sum(t["x"], before)
        y = emu_col_sum(t["x"], before)
        worst = max(worst, dc.fraction(mode, y, ref, mag))
        assert worst <= 1.0, c.name
        if c.n == 0:
            assert dc.same_bits(y, t["before"] if c.accumulate else torch.zeros(c.c))
            continue
        if bool(t["x"][-1].any()):
            assert _rejects(mode, emu_col_sum(t["x"][:-1], before), ref, mag), (c.name, "the last row left out")
        if c.accumulate and bool(t["before"].any()):
            assert _rejects(mode, emu_col_sum(t["x"]), ref, mag), (c.name, "accumulate ignored")
    print(f"column sum, f32 on the CPU, {mode}: worst fraction of the bound {worst:.3f}")
