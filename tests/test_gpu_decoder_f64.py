"""The decoder's small-row kernels (csrc/decoder.hip: LayerNorm forward / backward, the 32x32-tile linear forward in its
plain, padded and split forms, the fused dx | dW | db backward, the one-launch q/k/v backward, the fixed-order column sum)
on the MI355X, element-wise against float64 references computed on the card with plain torch operators
(tests/decoder_cases.py).

Each case runs through the C entry points (unscene3d_amd._lib, so the case decides the shape and the operands, not the
Python dispatcher).  Outputs are interior slices of larger buffers whose guards must keep their pattern; workspaces have
exactly the size usc_layernorm_bwd_ws_bytes / usc_col_sum_ws_bytes return.  Integer inputs must come out bit for bit,
random ones within 2**-20 of the sum of the absolute values of their terms.  The last test prints the largest fraction of
each bound a family used (profiles/decoder_f64_ratios.txt is that table of one run: a record)."""

import pytest
import torch

import decoder_cases as dc
from unscene3d_amd._lib import lib

pytestmark = pytest.mark.gpu

RATIOS = {}                                   # family -> {quantity: largest fraction of its bound}, "cases": n


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t):
    return None if t is None else (t.ptr() if hasattr(t, "ptr") else t.data_ptr())


def _ids(cases):
    return [c.name for c in cases]


def _within(family, c, fr):
    r = RATIOS.setdefault(family, {"cases": 0})
    r["cases"] += 1
    for k, v in fr.items():
        r[k] = max(r.get(k, 0.0), v)
    assert max(fr.values()) <= 1.0, (family, c.name, fr)


def _intact(*bufs):
    return all(b.guards_intact() for b in bufs if b is not None)


def _untouched(*bufs):
    return all(bool(b.pattern_rows().all()) and b.guards_intact() for b in bufs if b is not None)


def _same(a, b):
    """Two sets of guarded outputs hold the same bits."""
    return all(dc.same_bits(a[k].t, b[k].t) for k in a if a[k] is not None)


# ------------------------------------------------------------------------------------------------- LayerNorm
def _ln_param(t, name, c, device, keep=True):
    b = dc.GuardedF32(1, c.d, device, init=t[name][None] if keep else None, shift=int(c.shift))
    assert b.ptr() % 16 == (4 if c.shift else 0)
    return b


def _ln_forward(c, t, device):
    o = dict(gamma=_ln_param(t, "gamma", c, device), beta=_ln_param(t, "beta", c, device),
             y=dc.GuardedF32(c.rows, c.d, device), stats=dc.GuardedF32(2, max(c.rows, 1), device),
             sum_out=dc.GuardedF32(c.rows, c.d, device) if c.res else None)
    mean, rstd = _p(o["stats"].t[0]), _p(o["stats"].t[1])
    if c.res:
        code = lib.usc_add_layernorm_fwd(_p(t["x"]), _p(t["res"]), _p(o["gamma"]), _p(o["beta"]), c.rows, c.d, dc.EPS,
                                         _p(o["y"]), _p(o["sum_out"]), mean, rstd, _stream())
    else:
        code = lib.usc_layernorm_fwd(_p(t["x"]), _p(o["gamma"]), _p(o["beta"]), c.rows, c.d, dc.EPS, _p(o["y"]), mean, rstd,
                                     _stream())
    torch.cuda.synchronize()
    assert _intact(*o.values()), (c.name, "the LayerNorm forward wrote outside its outputs")
    return code, o


@pytest.mark.parametrize("c", dc.LN_CASES, ids=_ids(dc.LN_CASES))
def test_layernorm_forward(device, c):
    t = dc.to_device(dc.ln_inputs(c), device)
    code, o = _ln_forward(c, t, device)
    assert code == 0
    if c.res:
        assert dc.same_bits(o["sum_out"].t, t["v"]), (c.name, "sum_out is not f32(x + res) bit for bit")
    st = dc.ref_ln_fwd(t["v"], t["gamma"], t["beta"])
    fr = dc.ln_stat_fractions(o["stats"].t[0], o["stats"].t[1], st)
    fr["y"] = dc.fraction("bounded", o["y"].t, st["y"], st["y_mag"])
    _within("layernorm forward", c, fr)
    if c.repeat:
        _, o2 = _ln_forward(c, t, device)
        assert dc.same_bits(o["y"].t, o2["y"].t) and dc.same_bits(o["stats"].t, o2["stats"].t), (c.name, "a second launch gave other bits")


def _ln_backward(c, t, device, ws_short=0):
    o = dict(gamma=_ln_param(t, "gamma", c, device), dx=dc.GuardedF32(c.rows, c.d, device),
             dgamma=_ln_param(t, "dgamma0", c, device, keep=c.accumulate),
             dbeta=_ln_param(t, "dbeta0", c, device, keep=c.accumulate))
    ws = dc.GuardedWs(lib.usc_layernorm_bwd_ws_bytes(c.rows, c.d) - ws_short, device)
    assert ws.nbytes + ws_short == (0 if c.rows <= dc.LN_ROWS_PER_BLOCK else -(-c.rows // dc.LN_ROWS_PER_BLOCK) * 2 * c.d * 4)
    args = (c.rows, c.d) + ((_p(t["dx_add"]),) if c.dx_add else ()) + \
        (_p(o["dx"]), _p(o["dgamma"]), _p(o["dbeta"]), int(c.accumulate), ws.ptr(), ws.nbytes, _stream())
    fn = lib.usc_layernorm_bwd_ex if c.dx_add else lib.usc_layernorm_bwd
    code = fn(_p(t["dy"]), _p(t["v"]), _p(t["mean32"]), _p(t["rstd32"]), _p(o["gamma"]), *args)
    torch.cuda.synchronize()
    assert _intact(ws, *o.values()), (c.name, "the LayerNorm backward wrote outside its outputs or workspace")
    return code, o


@pytest.mark.parametrize("c", dc.LN_CASES, ids=_ids(dc.LN_CASES))
def test_layernorm_backward(device, c):
    t = dc.to_device(dc.ln_inputs(c), device)
    code, o = _ln_backward(c, t, device)
    assert code == 0
    refs = dc.ref_ln_bwd(t["v"], t["dy"], t["mean32"], t["rstd32"], t["gamma"], t["dx_add"],
                         t["dgamma0"] if c.accumulate else None, t["dbeta0"] if c.accumulate else None)
    got = dict(dx=o["dx"].t, dgamma=o["dgamma"].t[0], dbeta=o["dbeta"].t[0])
    _within("layernorm backward, " + ("one launch" if c.launches == 1 else "two launches"), c, dc.fractions("bounded", got, refs))
    if c.repeat:
        _, o2 = _ln_backward(c, t, device)
        assert _same(o, o2), (c.name, "a second launch gave other bits")


def test_layernorm_refusals_touch_nothing(device):
    for d in dc.LN_REFUSED_DIMS:
        c = dc.LnCase(f"refused-d{d}", 5, d)
        g = torch.Generator().manual_seed(d)
        t = dc.to_device(dict(x=torch.randn((5, d), generator=g), v=torch.randn((5, d), generator=g), res=None, dx_add=None,
                              dy=torch.randn((5, d), generator=g), gamma=torch.ones(d), beta=torch.zeros(d),
                              mean32=torch.zeros(5), rstd32=torch.ones(5)), device)
        code, o = _ln_forward(c, t, device)
        assert code != 0 and _untouched(o["y"], o["stats"]), (d, "forward")
        code, o = _ln_backward(c, t, device)
        assert code != 0 and _untouched(o["dx"], o["dgamma"], o["dbeta"]), (d, "backward")
    # no rows: the forward succeeds and writes nothing, the backward is refused
    c1 = dc.LnCase("one-row", 1, 128, res=True)
    t = dc.to_device(dc.ln_inputs(c1), device)
    for res in (False, True):
        c0 = dc.LnCase("no-rows", 0, 128, res=res)
        o = dict(y=dc.GuardedF32(1, 128, device), sum_out=dc.GuardedF32(1, 128, device), stats=dc.GuardedF32(2, 1, device))
        code = lib.usc_add_layernorm_fwd(_p(t["x"]), _p(t["res"]) if res else None, _p(t["gamma"]), _p(t["beta"]), 0, 128,
                                         dc.EPS, _p(o["y"]), _p(o["sum_out"]), _p(o["stats"].t[0]), _p(o["stats"].t[1]), _stream())
        torch.cuda.synchronize()
        assert code == 0 and _untouched(*o.values()), c0.name
    o = dict(dx=dc.GuardedF32(1, 128, device), dgamma=dc.GuardedF32(1, 128, device), dbeta=dc.GuardedF32(1, 128, device))
    code = lib.usc_layernorm_bwd(_p(t["dy"]), _p(t["v"]), _p(t["mean32"]), _p(t["rstd32"]), _p(t["gamma"]), 0, 128, _p(o["dx"]),
                                 _p(o["dgamma"]), _p(o["dbeta"]), 0, None, 0, _stream())
    torch.cuda.synchronize()
    assert code != 0 and _untouched(*o.values()), "backward without rows"
    # a workspace one byte short of the two-launch reduction
    c = next(c for c in dc.LN_CASES if c.rows == 1025 and c.d == 128)
    code, o = _ln_backward(c, dc.to_device(dc.ln_inputs(c), device), device, ws_short=1)
    assert code != 0 and _untouched(o["dx"]) and (c.accumulate or _untouched(o["dgamma"], o["dbeta"])), "short workspace"


# ------------------------------------------------------------------------------------------------- linear forward
def _fwd(c, t, device):
    args = (_p(t["x"]), _p(t["x2"]), _p(t["W"]), _p(t["b"]), c.M, c.N, c.K)
    if c.family == "split":
        y = dc.GuardedF32(c.N // c.split * c.M, c.split, device)
        code = lib.usc_linear_fwd_split(*args, c.x2_cols, c.split, _p(y), _stream())
    elif c.family == "pad":
        y = dc.GuardedF32(c.M_pad, c.N, device)
        code = lib.usc_linear_fwd_pad(*args, int(c.relu), _p(y), c.M_pad, _stream())
    elif c.x2 or c.relu:
        y = dc.GuardedF32(c.M, c.N, device)
        code = lib.usc_linear_fwd_ex(*args, int(c.relu), _p(y), _stream())
    else:
        y = dc.GuardedF32(c.M, c.N, device)
        code = lib.usc_linear_fwd(_p(t["x"]), _p(t["W"]), _p(t["b"]), c.M, c.N, c.K, _p(y), _stream())
    torch.cuda.synchronize()
    assert y.guards_intact(), (c.name, "the linear forward wrote outside its output")
    return code, y


def _forward_case(device, c, family):
    for mode in dc.MODES:
        t = dc.to_device(dc.lin_inputs(c, mode), device)
        code, y = _fwd(c, t, device)
        assert code == 0
        ref, mag = dc.ref_linear_fwd(t["x"], t["x2"], t["W"], t["b"], c.relu, c.x2_cols if c.family == "split" else None)
        if c.family == "split":
            ref, mag = dc.split_layout(ref, c.split), dc.split_layout(mag, c.split)
        if c.family == "pad":
            assert dc.same_bits(y.t[c.M:], torch.zeros_like(y.t[c.M:])), (c.name, mode, "the padding rows are not +0.0")
        fr = dict(y=dc.fraction(mode, y.t[:ref.shape[0]], ref, mag))
        if c.relu:
            assert bool((y.t.view(torch.int32) >= 0).all()), (c.name, mode, "ReLU left a negative sign bit")
        if mode == "exact":
            assert fr["y"] == 0.0, (c.name, "integer inputs: not the float64 result bit for bit")
        else:
            _within(family, c, fr)
        if c.repeat:
            assert dc.same_bits(y.t, _fwd(c, t, device)[1].t), (c.name, mode, "a second launch gave other bits")


@pytest.mark.parametrize("c", dc.LIN_CASES["fwd"], ids=_ids(dc.LIN_CASES["fwd"]))
def test_linear_forward(device, c):
    _forward_case(device, c, "linear forward")


@pytest.mark.parametrize("c", dc.LIN_CASES["pad"], ids=_ids(dc.LIN_CASES["pad"]))
def test_linear_forward_pad(device, c):
    _forward_case(device, c, "forward pad")


@pytest.mark.parametrize("c", dc.LIN_CASES["split"], ids=_ids(dc.LIN_CASES["split"]))
def test_linear_forward_split(device, c):
    _forward_case(device, c, "forward split")


def test_linear_forward_refusals_touch_nothing(device):
    base = dc.LinCase("fwd", "refused", 33, 96, 96, x2=True)
    t = dc.to_device(dc.lin_inputs(base, "bounded"), device)
    args = (_p(t["x"]), _p(t["x2"]), _p(t["W"]), _p(t["b"]))
    y = dc.GuardedF32(64, 96, device)
    codes = dict(
        pad_below_m=lib.usc_linear_fwd_pad(*args, 33, 96, 96, 0, _p(y), 32, _stream()),
        split_not_a_divisor=lib.usc_linear_fwd_split(*args, 33, 96, 96, 32, 64, _p(y), _stream()),
        split_not_32=lib.usc_linear_fwd_split(*args, 33, 96, 96, 32, 48, _p(y), _stream()),
        n_not_32=lib.usc_linear_fwd_ex(*args, 33, 48, 96, 0, _p(y), _stream()),
        k_not_32=lib.usc_linear_fwd_ex(*args, 33, 96, 48, 0, _p(y), _stream()),
        split_n_not_32=lib.usc_linear_fwd_split(*args, 33, 48, 96, 0, 48, _p(y), _stream()),
        no_rows=lib.usc_linear_fwd(_p(t["x"]), _p(t["W"]), _p(t["b"]), 0, 96, 96, _p(y), _stream()))
    torch.cuda.synchronize()
    assert all(v != 0 for v in codes.values()), codes
    assert _untouched(y)


# ------------------------------------------------------------------------------------------------- linear backward
def _bwd(c, t, device):
    acc = c.accumulate
    o = dict(dx=dc.GuardedF32(c.M, c.K, device) if c.want_dx else None,
             dx_b=dc.GuardedF32(c.M, c.K, device) if c.has("dx_b") else None,
             dW=dc.GuardedF32(c.N, c.K, device, init=t["dW0"] if acc else None) if c.want_dW else None,
             db=dc.GuardedF32(1, c.N, device, init=t["db0"][None] if acc else None) if c.want_db else None)
    if c.family == "bwd_plain":
        code = lib.usc_linear_bwd(_p(t["dy"]), _p(t["x"]), _p(t["W"]), c.M, c.N, c.K, _p(o["dx"]), _p(o["dW"]), _p(o["db"]),
                                  int(acc), _stream())
    elif c.has("dx_add2") or c.has("dx_b"):
        code = lib.usc_linear_bwd_ex2(_p(t["dy"]), _p(t["y_relu"]), _p(t["x"]), _p(t["x2"]), _p(t["W"]), c.M, c.N, c.K,
                                      _p(o["dx"]), _p(t["dx_add"]), _p(t["dx_add2"]), _p(o["dx_b"]), _p(o["dW"]), _p(o["db"]),
                                      int(acc), _stream())
    else:
        code = lib.usc_linear_bwd_ex(_p(t["dy"]), _p(t["y_relu"]), _p(t["x"]), _p(t["x2"]), _p(t["W"]), c.M, c.N, c.K,
                                     _p(o["dx"]), _p(t["dx_add"]), _p(o["dW"]), _p(o["db"]), int(acc), _stream())
    torch.cuda.synchronize()
    assert _intact(*o.values()), (c.name, "the linear backward wrote outside its outputs")
    return code, o


def _got(o):
    return {k: (b.t[0] if k == "db" else b.t) for k, b in o.items() if b is not None}


def _backward_case(device, c, family, run, refs_of):
    for mode in dc.MODES:
        t = dc.to_device(dc.lin_inputs(c, mode), device)
        code, o = run(c, t, device)
        assert code == 0
        fr = dc.fractions(mode, _got(o), refs_of(c, t))
        if mode == "exact":
            assert max(fr.values()) == 0.0, (c.name, fr, "integer inputs: not the float64 result bit for bit")
        else:
            _within(family, c, fr)
        if c.repeat:
            assert _same(o, run(c, t, device)[1]), (c.name, mode, "a second launch gave other bits")


def _bwd_refs(c, t):
    return dc.ref_linear_bwd(t["dy"], t["y_relu"], t["x"], t["x2"], t["W"], t["dx_add"], t["dx_add2"],
                             t["dW0"] if c.accumulate else None, t["db0"] if c.accumulate else None)


@pytest.mark.parametrize("c", dc.LIN_CASES["bwd_plain"], ids=_ids(dc.LIN_CASES["bwd_plain"]))
def test_linear_backward_plain(device, c):
    _backward_case(device, c, "backward plain", _bwd, _bwd_refs)


@pytest.mark.parametrize("c", dc.LIN_CASES["bwd_ex"], ids=_ids(dc.LIN_CASES["bwd_ex"]))
def test_linear_backward_ex(device, c):
    _backward_case(device, c, "backward ex", _bwd, _bwd_refs)


def test_linear_backward_refusals_touch_nothing(device):
    c = dc.LinCase("bwd_ex", "refused", 33, 96, 32, operands=("dx_add",))
    t = dc.to_device(dc.lin_inputs(c, "bounded"), device)
    dx, dW, db = dc.GuardedF32(33, 32, device), dc.GuardedF32(96, 32, device), dc.GuardedF32(1, 96, device)
    head = (_p(t["dy"]), None, _p(t["x"]), None, _p(t["W"]), 33, 96, 32)
    codes = dict(
        dx_add_without_dx=lib.usc_linear_bwd_ex(*head, None, _p(t["dx_add"]), _p(dW), _p(db), 0, _stream()),
        dx_add2_without_dx=lib.usc_linear_bwd_ex2(*head, None, None, _p(t["dx_add"]), None, _p(dW), _p(db), 0, _stream()),
        dx_b_without_dx=lib.usc_linear_bwd_ex2(*head, None, None, None, _p(dx), _p(dW), _p(db), 0, _stream()),
        db_without_dW=lib.usc_linear_bwd(_p(t["dy"]), _p(t["x"]), _p(t["W"]), 33, 96, 32, _p(dx), None, _p(db), 0, _stream()),
        db_without_dW_ex=lib.usc_linear_bwd_ex2(*head, _p(dx), _p(t["dx_add"]), None, None, None, _p(db), 1, _stream()),
        k_not_32=lib.usc_linear_bwd(_p(t["dy"]), _p(t["x"]), _p(t["W"]), 33, 96, 16, _p(dx), _p(dW), _p(db), 0, _stream()),
        no_rows=lib.usc_linear_bwd(_p(t["dy"]), _p(t["x"]), _p(t["W"]), 0, 96, 32, _p(dx), _p(dW), _p(db), 0, _stream()))
    torch.cuda.synchronize()
    assert all(v != 0 for v in codes.values()), codes
    assert _untouched(dx, dW, db)


# ------------------------------------------------------------------------------------------------- q/k/v backward
def _qkv(c, t, device):
    E, acc = c.K, c.accumulate
    o = dict(dx=dc.GuardedF32(c.M, E, device), dx_b=dc.GuardedF32(c.M, E, device) if c.has("dx_b") else None,
             dW=dc.GuardedF32(3 * E, E, device, init=t["dW0"] if acc else None),
             db=dc.GuardedF32(1, 3 * E, device, init=t["db0"][None] if acc else None) if c.has("db") else None)
    code = lib.usc_qkv_proj_bwd(_p(t["dy3"]), _p(t["x"]), _p(t["pos"]), _p(t["W"]), c.M, E, _p(o["dx"]), _p(o["dx_b"]),
                                _p(t["dres"]), _p(o["dW"]), _p(o["db"]), int(acc), _stream())
    torch.cuda.synchronize()
    assert _intact(*o.values()), (c.name, "usc_qkv_proj_bwd wrote outside its outputs")
    return code, o


def _qkv_refs(c, t):
    return dc.ref_qkv_bwd(t["dy3"], t["x"], t["pos"], t["W"], t["dres"], t["dW0"] if c.accumulate else None,
                          t["db0"] if c.accumulate else None)


@pytest.mark.parametrize("c", dc.LIN_CASES["qkv"], ids=_ids(dc.LIN_CASES["qkv"]))
def test_qkv_projection_backward(device, c):
    _backward_case(device, c, "qkv backward", _qkv, _qkv_refs)


# ------------------------------------------------------------------------------------------------- column sum
def _col_sum(c, t, device, ws_short=0):
    out = dc.GuardedF32(1, c.c, device, init=t["before"][None] if c.accumulate else None)
    ws = dc.GuardedWs(lib.usc_col_sum_ws_bytes(c.n, c.c) - ws_short, device)
    assert ws.nbytes + ws_short == -(-c.n // 64) * c.c * 4
    code = lib.usc_col_sum(_p(t["x"]) if c.n else None, c.n, c.c, _p(out), int(c.accumulate), ws.ptr(), ws.nbytes, _stream())
    torch.cuda.synchronize()
    assert out.guards_intact() and ws.guards_intact(), (c.name, "usc_col_sum wrote outside its output or workspace")
    return code, out


@pytest.mark.parametrize("c", dc.COLSUM_CASES, ids=_ids(dc.COLSUM_CASES))
def test_column_sum(device, c):
    for mode in dc.MODES:
        t = dc.to_device(dc.colsum_inputs(c, mode), device)
        code, out = _col_sum(c, t, device)
        assert code == 0
        ref, mag = dc.ref_col_sum(t["x"], t["before"] if c.accumulate else None)
        fr = dict(out=dc.fraction(mode, out.t[0], ref, mag))
        if c.n == 0:
            assert dc.same_bits(out.t[0], t["before"] if c.accumulate else torch.zeros_like(t["before"])), (c.name, mode)
        if mode == "exact":
            assert fr["out"] == 0.0, (c.name, "integer inputs: not the float64 sum bit for bit")
        else:
            _within("column sum", c, fr)
        assert dc.same_bits(out.t, _col_sum(c, t, device)[1].t), (c.name, mode, "a second launch gave other bits")


def test_column_sum_refuses_a_short_workspace(device):
    c = dc.ColSumCase("short", 65, 17)
    code, out = _col_sum(c, dc.to_device(dc.colsum_inputs(c, "bounded"), device), device, ws_short=1)
    assert code != 0 and _untouched(out)


# ------------------------------------------------------------------------------------------------- the dispatcher
@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("rows", (1024, 1025))
def test_ops_linear_with_relu_and_passthrough_on_both_sides_of_the_row_limit(device, rows, mode):
    """ops.linear(relu=True, passthrough=True): 1024 rows take the few-row kernels, 1025 the many-row fallback; y, dx (with
    the residual gradient summed in), dW and db element-wise against float64, the mask taken on the bits of y."""
    from unscene3d_amd import ops

    K = N = 128
    assert ops._small_linear_ok(rows, K, N) == (rows == 1024) and ops._rows_gemm_ok(rows, K, N) == (rows == 1025)
    c = dc.LinCase("bwd_ex", f"ops-linear-{rows}", rows, N, K, operands=("dx_add",))
    t = dc.to_device(dc.lin_inputs(c, mode), device)
    x = t["x"].clone().requires_grad_()
    W, b = torch.nn.Parameter(t["W"].clone()), torch.nn.Parameter(t["b"].clone())
    y, xp = ops.linear(x, W, b, relu=True, passthrough=True)
    torch.autograd.backward([y, xp], [t["dy"], t["dx_add"]])
    torch.cuda.synchronize()
    ref, mag = dc.ref_linear_fwd(t["x"], None, t["W"], t["b"], relu=True)
    refs = dc.ref_linear_bwd(t["dy"], y.detach(), t["x"], None, t["W"], dx_add=t["dx_add"])
    fr = dc.fractions(mode, dict(dx=x.grad, dW=W.grad, db=b.grad), refs)
    fr["y"] = dc.fraction(mode, y.detach(), ref, mag)
    if mode == "exact":
        assert max(fr.values()) == 0.0, (rows, fr)
    else:
        _within("ops.linear " + ("few-row" if rows == 1024 else "many-row"), c, fr)


@pytest.mark.parametrize("add", (False, True))
def test_ops_layer_norm_accumulates_in_place_through_two_launches(device, add):
    """ops.layer_norm(passthrough=True) and ops.add_layer_norm at 1025 rows with pre-allocated .grad buffers: dgamma / dbeta
    are added into them by the two-launch reduction."""
    from unscene3d_amd import ops

    c = dc.LnCase("ops-add-layer-norm" if add else "ops-layer-norm", 1025, 128, res=add, dx_add=not add, accumulate=True)
    t = dc.to_device(dc.ln_inputs(c), device)
    w, b = torch.nn.Parameter(t["gamma"].clone()), torch.nn.Parameter(t["beta"].clone())
    w.grad, b.grad = t["dgamma0"].clone(), t["dbeta0"].clone()
    held = (w.grad, b.grad)
    x = t["x"].clone().requires_grad_()
    if add:
        res = t["res"].clone().requires_grad_()
        y = ops.add_layer_norm(x, res, w, b, dc.EPS)
        saved, _, mean, rstd = y.grad_fn.saved_tensors
        assert dc.same_bits(saved, t["v"]), "the saved sum is not f32(x + res)"
        y.backward(t["dy"])
    else:
        y, xp = ops.layer_norm(x, w, b, dc.EPS, passthrough=True)
        _, _, mean, rstd = y.grad_fn.saved_tensors
        torch.autograd.backward([y, xp], [t["dy"], t["dx_add"]])
    torch.cuda.synchronize()
    assert w.grad is held[0] and b.grad is held[1], "the gradients were not added in place"
    st = dc.ref_ln_fwd(t["v"], t["gamma"], t["beta"])
    fr = dc.ln_stat_fractions(mean, rstd, st)
    fr["y"] = dc.fraction("bounded", y.detach(), st["y"], st["y_mag"])
    refs = dc.ref_ln_bwd(t["v"], t["dy"], mean, rstd, t["gamma"], t["dx_add"], t["dgamma0"], t["dbeta0"])
    fr.update(dc.fractions("bounded", dict(dx=x.grad, dgamma=w.grad, dbeta=b.grad), refs))
    if add:
        assert dc.same_bits(res.grad, x.grad), "both addends receive the same gradient"
    _within("ops." + ("add_layer_norm" if add else "layer_norm"), c, fr)


def test_print_the_bound_fractions_per_family():
    """A record, not a check: the largest fraction of its bound each quantity used, per family."""
    print("\nfamily / cases / largest |err| / bound per quantity")
    for fam, r in RATIOS.items():
        print(f"{fam:<36} {r['cases']:4d}  " + "  ".join(f"{k} {v:.3f}" for k, v in r.items() if k != "cases"))
