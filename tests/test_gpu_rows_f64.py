"""Batch norm in its three forms, ReLU, pooling, gather / scatter and the segment kernels (csrc/rows.hip) and the
batch-norm dispatch of the unit calls (csrc/units.hip) on the MI355X, element-wise against float64 references computed
on the card with plain torch operators (tests/rows_cases.py).

Each case asserts the form usc_bn_plan names, then runs through the C entry points (unscene3d_amd._lib, so the case
decides the form, not the Python dispatcher).  Outputs are interior slices of larger buffers whose guards must keep their
pattern; workspaces have exactly the size usc_colstats_ws_bytes / usc_bn_tile_ws_bytes / usc_segment_csr_ws_bytes return.
The last test prints the largest fraction of each bound a family used (profiles/rows_f64_ratios.txt is that table of one
run: a record)."""

import pytest
import torch

import rows_cases as rc
from unscene3d_amd._lib import check, lib

pytestmark = pytest.mark.gpu

RATIOS = {}                                   # family -> {quantity: largest fraction of its bound}, "cases": n
NBT0 = 41


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t):
    return None if t is None else (t.ptr() if hasattr(t, "ptr") else t.data_ptr())


def _ids(cases):
    return [c.name for c in cases]


def _record(family, fr):
    r = RATIOS.setdefault(family, {"cases": 0})
    r["cases"] += 1
    for k, v in fr.items():
        r[k] = max(r.get(k, 0.0), v)


def _within(family, c, fr):
    _record(family, fr)
    assert max(fr.values()) <= 1.0, (family, c.name, fr)


class Counter:
    """num_batches_tracked: one i64 between two guard words."""

    def __init__(self, device):
        self.buf = torch.tensor([-7, NBT0, -7], dtype=torch.int64, device=device)

    def ptr(self):
        return self.buf.data_ptr() + 8

    def value(self):
        v = self.buf.tolist()
        assert v[0] == -7 and v[2] == -7, "wrote beside num_batches_tracked"
        return v[1]


class GuardedF64:
    def __init__(self, n, device):
        self.g, self.n = 512, n
        self.buf = torch.full((self.g + n + self.g,), float("nan"), dtype=torch.float64, device=device)
        self.t = self.buf[self.g:self.g + n]

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.g]).all()) and bool(torch.isnan(self.buf[self.g + self.n:]).all())


def _param(t, name, c, device, keep=True):
    """A per-channel vector in a guarded buffer, one float into it (4-byte aligned only) when the case says so."""
    b = rc.GuardedF32(1, c.c, device, init=t[name][None] if keep else None, shift=int(c.shift))
    assert b.ptr() % 16 == (4 if c.shift else 0)
    return b


def _intact(*bufs):
    return all(b.guards_intact() for b in bufs if b is not None)


def _untouched(*bufs):
    return all(bool(b.pattern_rows().all()) and b.guards_intact() for b in bufs)


# ------------------------------------------------------------------------------------------------- statistics + apply
def _forward_stats(c, t, device):
    prm = {k: _param(t, k, c, device) for k in ("gamma", "beta", "rm", "rv")}
    stats, nbt = rc.GuardedF32(4, c.c, device), Counter(device)
    ws = rc.GuardedWs(lib.usc_colstats_ws_bytes(c.n, c.c), device)
    code = lib.usc_bn_forward_stats(_p(t["x"]), c.n, c.c, _p(prm["gamma"]), _p(prm["beta"]), rc.EPS, rc.MOMENTUM,
                                    _p(prm["rm"]), _p(prm["rv"]), nbt.ptr(), *(_p(stats.t[i]) for i in range(4)), ws.ptr(),
                                    ws.nbytes, _stream())
    torch.cuda.synchronize()
    assert _intact(stats, ws, *prm.values()), (c.name, "wrote outside its outputs or workspace")
    return code, prm, stats, nbt


def _stat_outputs(prm, stats):
    return dict(mean=stats.t[0], invstd=stats.t[1], scale=stats.t[2], shift=stats.t[3], rm=prm["rm"].t[0], rv=prm["rv"].t[0])


def _apply(c, t, stats, device):
    out = rc.GuardedF32(c.n, c.c, device)
    check(lib.usc_bn_apply(_p(t["x"]), _p(stats.t[2]), _p(stats.t[3]), _p(t["res"]), int(c.relu), out.ptr(), c.n, c.c,
                           _stream()), "usc_bn_apply")
    torch.cuda.synchronize()
    assert out.guards_intact(), (c.name, "usc_bn_apply wrote outside its output")
    return out


@pytest.mark.parametrize("c", rc.BN_CASES["fwd"], ids=_ids(rc.BN_CASES["fwd"]))
def test_forward_statistics_and_apply(device, c):
    assert rc.decoded_plan(lib, c) == c.plan
    t = rc.to_device(rc.bn_inputs(c), device)
    code, prm, stats, nbt = _forward_stats(c, t, device)
    if c.plan == "refused":
        assert code != 0 and _untouched(stats) and nbt.value() == NBT0
        assert rc.same_bits(prm["rm"].t[0], t["rm"]) and rc.same_bits(prm["rv"].t[0], t["rv"])
        return
    assert code == 0 and nbt.value() == NBT0 + 1
    st = rc.ref_stats(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"])
    ref, mag = rc.ref_apply(t["x"], st, t["beta"], t["res"], c.relu)
    fr = rc.stats_fractions(_stat_outputs(prm, stats), st)
    out = _apply(c, t, stats, device)
    fr["out"] = rc.elem_ratio(out.t, ref, mag)
    _within("statistics " + rc.stat_form(c.plan), c, fr)
    if c.repeat:
        _, prm2, stats2, _ = _forward_stats(c, t, device)
        assert rc.same_bits(stats.t, stats2.t) and rc.same_bits(prm["rv"].t, prm2["rv"].t), (c.name, "a second launch gave other bits")
        assert rc.same_bits(out.t, _apply(c, t, stats2, device).t)


# ------------------------------------------------------------------------------------------------- reduce + dx
def _backward(c, t, device):
    gamma = _param(t, "gamma", c, device)
    dgamma, dbeta = _param(t, "dgamma0", c, device, keep=c.acc), _param(t, "dbeta0", c, device, keep=c.acc)
    saved = rc.GuardedF32(2, c.c, device, init=torch.stack([t["mean32"], t["invstd32"]]))
    red = rc.GuardedF32(2, c.c, device)
    ws = rc.GuardedWs(lib.usc_colstats_ws_bytes(c.n, c.c), device)
    code = lib.usc_bn_backward_reduce(_p(t["x"]), _p(t["dy"]), _p(t["y_out"]), _p(saved.t[0]), _p(saved.t[1]), c.n, c.c,
                                      c.training, int(c.acc), dgamma.ptr(), dbeta.ptr(), _p(red.t[0]), _p(red.t[1]),
                                      ws.ptr(), ws.nbytes, _stream())
    torch.cuda.synchronize()
    assert _intact(gamma, dgamma, dbeta, saved, red, ws), (c.name, "usc_bn_backward_reduce wrote outside its outputs")
    if code != 0:
        return code, dgamma, dbeta, red, None, None
    dx = rc.GuardedF32(c.n, c.c, device)
    dres = rc.GuardedF32(c.n, c.c, device) if c.dres else None
    check(lib.usc_bn_backward_dx(_p(t["x"]), _p(t["dy"]), _p(t["y_out"]), _p(saved.t[0]), _p(saved.t[1]), gamma.ptr(),
                                 _p(red.t[0]), _p(red.t[1]), dx.ptr(), _p(dres), c.n, c.c, _stream()), "usc_bn_backward_dx")
    torch.cuda.synchronize()
    assert _intact(dx, dres, gamma, saved, red), (c.name, "usc_bn_backward_dx wrote outside its outputs")
    return code, dgamma, dbeta, red, dx, dres


def _ref_backward(c, t):
    return rc.ref_backward(t["x"], t["dy"], t["y_out"], t["mean32"], t["invstd32"], t["gamma"], c.training,
                           t["dgamma0"] if c.acc else None, t["dbeta0"] if c.acc else None)


@pytest.mark.parametrize("c", rc.BN_CASES["bwd"], ids=_ids(rc.BN_CASES["bwd"]))
def test_backward_reduce_and_dx(device, c):
    assert rc.decoded_plan(lib, c) == c.plan
    t = rc.to_device(rc.bn_inputs(c), device)
    code, dgamma, dbeta, red, dx, dres = _backward(c, t, device)
    if c.plan == "refused":
        assert code != 0 and _untouched(red) and (c.acc or _untouched(dgamma, dbeta))
        return
    assert code == 0
    rb = _ref_backward(c, t)
    got = dict(dbeta=dbeta.t[0], dgamma=dgamma.t[0], mean_g=red.t[0], mean_gx=red.t[1], dx=dx.t)
    _within("backward " + rc.stat_form(c.plan), c, rc.backward_fractions(got, rb))
    if not c.training:
        assert not bool(red.t.any()), (c.name, "eval mode: the two means must be exactly 0")
    if c.dres:
        assert rc.same_bits(dres.t, rb["g32"]), (c.name, "dres is not the masked gradient bit for bit")
    if c.repeat:
        _, dgamma2, dbeta2, red2, dx2, _ = _backward(c, t, device)
        assert rc.same_bits(dx.t, dx2.t) and rc.same_bits(dgamma.t, dgamma2.t) and rc.same_bits(dbeta.t, dbeta2.t) \
            and rc.same_bits(red.t, red2.t), (c.name, "a second launch gave other bits")


def test_apply_and_dx_of_an_empty_map_touch_nothing(device):
    for c in (4, 3):
        out, dres = rc.GuardedF32(1, c, device), rc.GuardedF32(1, c, device)
        v = torch.ones(c, device=device)
        check(lib.usc_bn_apply(_p(v), _p(v), _p(v), None, 1, out.ptr(), 0, c, _stream()), "usc_bn_apply")
        check(lib.usc_bn_backward_dx(_p(v), _p(v), None, _p(v), _p(v), _p(v), _p(v), _p(v), out.ptr(), dres.ptr(), 0, c,
                                     _stream()), "usc_bn_backward_dx")
        torch.cuda.synchronize()
        assert _untouched(out, dres)


# ------------------------------------------------------------------------------------------------- tile form
def _tile_forward(c, t, device):
    prm = {k: _param(t, k, c, device) for k in ("gamma", "beta", "rm", "rv")}
    stats, nbt = rc.GuardedF32(4, c.c, device), Counter(device)
    y = rc.GuardedF32(c.n, c.c, device, init=None if c.G else t["x"])
    out = rc.GuardedF32(c.n, c.c, device)
    ws = rc.GuardedWs(lib.usc_bn_tile_ws_bytes(c.c), device)
    check(lib.usc_bn_tile_forward(_p(t.get("slices")), c.G, y.ptr(), c.n, c.c, _p(prm["gamma"]), _p(prm["beta"]), rc.EPS,
                                  rc.MOMENTUM, _p(prm["rm"]), _p(prm["rv"]), nbt.ptr(), *(_p(stats.t[i]) for i in range(4)),
                                  _p(t["res"]), int(c.relu), out.ptr(), ws.ptr(), ws.nbytes, _stream()), "usc_bn_tile_forward")
    torch.cuda.synchronize()
    assert _intact(y, out, stats, ws, *prm.values()), (c.name, "usc_bn_tile_forward wrote outside its outputs or workspace")
    return prm, stats, nbt, y, out


def _tile_backward(c, t, device):
    gamma = _param(t, "gamma", c, device)
    dgamma, dbeta = _param(t, "dgamma0", c, device, keep=c.acc), _param(t, "dbeta0", c, device, keep=c.acc)
    saved = rc.GuardedF32(2, c.c, device, init=torch.stack([t["mean32"], t["invstd32"]]))
    dout = rc.GuardedF32(c.n, c.c, device, init=t["dout0"] if c.G else t["dy"])
    dy = rc.GuardedF32(c.n, c.c, device)
    dres = rc.GuardedF32(c.n, c.c, device) if c.dres else None
    ws = rc.GuardedWs(lib.usc_bn_tile_ws_bytes(c.c), device)
    check(lib.usc_bn_tile_backward(_p(t.get("dslices")), c.G, int(c.slice_acc), dout.ptr(), _p(t["x"]), _p(t["y_out"]),
                                   _p(saved.t[0]), _p(saved.t[1]), gamma.ptr(), c.n, c.c, c.training, int(c.acc),
                                   dgamma.ptr(), dbeta.ptr(), dy.ptr(), _p(dres), ws.ptr(), ws.nbytes, _stream()),
          "usc_bn_tile_backward")
    torch.cuda.synchronize()
    assert _intact(gamma, dgamma, dbeta, saved, dout, dy, dres, ws), (c.name, "usc_bn_tile_backward wrote outside its outputs")
    return dgamma, dbeta, dout, dy, dres


@pytest.mark.parametrize("c", rc.BN_CASES["tile"], ids=_ids(rc.BN_CASES["tile"]))
def test_tile_form(device, c):
    assert rc.decoded_plan(lib, c) == c.plan
    t = rc.to_device(rc.bn_inputs(c), device)
    # ---- forward: y is the slice sum bit for bit, statistics and apply on that y
    prm, stats, nbt, y, out = _tile_forward(c, t, device)
    assert rc.same_bits(y.t, t["x"]), (c.name, "y is not the f32 sum of the slices in slice order")
    assert nbt.value() == NBT0 + 1
    st = rc.ref_stats(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"])
    ref, mag = rc.ref_apply(t["x"], st, t["beta"], t["res"], c.relu)
    fr = rc.stats_fractions(_stat_outputs(prm, stats), st)
    fr["out"] = rc.elem_ratio(out.t, ref, mag)
    _within("tile forward", c, fr)
    # ---- backward
    dgamma, dbeta, dout, dy, dres = _tile_backward(c, t, device)
    rb = _ref_backward(c, t)
    _within("tile backward", c, rc.backward_fractions(dict(dbeta=dbeta.t[0], dgamma=dgamma.t[0], dx=dy.t), rb))
    before = t["dout0"] if c.G else t["dy"]
    if c.dres:
        assert rc.same_bits(dres.t, rb["g32"]) and rc.same_bits(dout.t, before), (c.name, "masked gradient: dres, dout kept")
    elif c.G:
        assert rc.same_bits(dout.t, rb["g32"]), (c.name, "masked gradient: in place")
    else:
        assert rc.same_bits(dout.t, before), (c.name, "a finished dout without a residual consumer was written")
    if c.repeat:
        prm2, stats2, _, _, out2 = _tile_forward(c, t, device)
        assert rc.same_bits(stats.t, stats2.t) and rc.same_bits(out.t, out2.t) and rc.same_bits(prm["rv"].t, prm2["rv"].t)
        dgamma2, dbeta2, _, dy2, _ = _tile_backward(c, t, device)
        assert rc.same_bits(dy.t, dy2.t) and rc.same_bits(dgamma.t, dgamma2.t) and rc.same_bits(dbeta.t, dbeta2.t)


# ------------------------------------------------------------------------------------------------- eval statistics, colstats
@pytest.mark.parametrize("c", (1, 19, 256, 257, 1024))
def test_eval_statistics(device, c):
    case = rc.BnCase("eval", f"c{c}", "", 1, c, shift=c % 2 == 1)
    t = rc.to_device(rc.params(c, 100 + c), device)
    assert bool((t["rv"] == 0).any())
    prm = {k: _param(t, k, case, device) for k in ("gamma", "beta", "rm", "rv")}
    stats = rc.GuardedF32(4, c, device)
    check(lib.usc_bn_eval_stats(_p(prm["gamma"]), _p(prm["beta"]), _p(prm["rm"]), _p(prm["rv"]), rc.EPS, c,
                                *(_p(stats.t[i]) for i in range(4)), _stream()), "usc_bn_eval_stats")
    torch.cuda.synchronize()
    assert _intact(stats, *prm.values())
    st = rc.ref_eval_stats(t["gamma"], t["beta"], t["rm"], t["rv"])
    assert rc.same_bits(stats.t[0], t["rm"])
    fr = dict(invstd=rc.invstd_ratio(stats.t[1], st["invstd"]), scale=rc.elem_ratio(stats.t[2], st["scale"], st["scale_mag"]),
              shift=rc.elem_ratio(stats.t[3], st["shift"], st["shift_mag"]))
    _within("eval statistics", case, fr)


@pytest.mark.parametrize("n,c,second", [(1, 3, False), (33, 255, True), (5000, 516, True), (4097, 4, False), (70001, 256, False)])
def test_colstats(device, n, c, second):
    x = rc.recipe_table(n, c, n + c).to(device)
    y = torch.randn((n, c), generator=torch.Generator().manual_seed(n)).to(device) if second else None
    s1, s2 = GuardedF64(c, device), GuardedF64(c, device)
    ws = rc.GuardedWs(lib.usc_colstats_ws_bytes(n, c), device)
    check(lib.usc_colstats(_p(x), _p(y), n, c, s1.ptr(), s2.ptr(), ws.ptr(), ws.nbytes, _stream()), "usc_colstats")
    torch.cuda.synchronize()
    assert s1.guards_intact() and s2.guards_intact() and ws.guards_intact()
    xd = x.double()
    other = xd if y is None else y.double()
    fr = dict(sum1=rc._worst((s1.t - xd.sum(0)).abs(), 2.0 ** -45 * xd.abs().sum(0) + 1e-300),
              sum2=rc._worst((s2.t - (xd * other).sum(0)).abs(), 2.0 ** -45 * (xd * other).abs().sum(0) + 1e-300))
    _within("colstats", rc.BnCase("colstats", f"n{n}-c{c}", "", n, c), fr)


# ------------------------------------------------------------------------------------------------- unit calls
@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("n", (4096, 4097))
def test_unit_calls_take_the_form_the_plan_names(device, n, training):
    """units.conv_bn_act over identity rows with an identity weight (y == x): output, statistics and gradients equal the
    direct call of the form usc_bn_plan names for the map, bit for bit."""
    from unscene3d_amd import units

    c = 64
    case = rc.BnCase("bwd", f"unit-n{n}", "", n, c, relu=True, training=int(training))
    plan = rc.decode_plan(lib.usc_bn_plan(n, c, 0))
    assert plan["units"] == int(n == 4096)
    t = rc.to_device(rc.bn_inputs(case), device)
    t["dy"] = t["dy"].contiguous()
    bn = torch.nn.BatchNorm1d(c, eps=rc.EPS, momentum=rc.MOMENTUM).to(device)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"]), bn.bias.copy_(t["beta"]), bn.running_mean.copy_(t["rm"]), bn.running_var.copy_(t["rv"])
        bn.num_batches_tracked.fill_(NBT0)
    bn.train(training)
    W = torch.eye(c, device=device)[None].clone().requires_grad_()
    x = t["x"].clone().requires_grad_()
    out = units.conv_bn_act(x, W, bn, units.kmap_identity(n), units.SAME, residual=None, relu=True)
    _, _, y_saved, stats_saved, _ = out.grad_fn.saved_tensors
    assert torch.equal(y_saved, t["x"])
    out.backward(t["dy"])
    units.flush_deferred_wgrads(device)
    units.join_lane(device)
    torch.cuda.synchronize()
    # ---- the direct calls
    rm, rv = t["rm"].clone(), t["rv"].clone()
    stats, nbt = torch.empty((4, c), device=device), Counter(device)
    direct = torch.empty((n, c), device=device)
    sargs = [_p(stats[i]) for i in range(4)]
    tile = bool(plan["units"])
    ws = rc.GuardedWs(lib.usc_bn_tile_ws_bytes(c) if tile else lib.usc_colstats_ws_bytes(n, c), device)
    yb = t["x"].clone()
    if not training:
        check(lib.usc_bn_eval_stats(_p(t["gamma"]), _p(t["beta"]), _p(rm), _p(rv), rc.EPS, c, *sargs, _stream()), "eval")
        check(lib.usc_bn_apply(_p(yb), sargs[2], sargs[3], None, 1, _p(direct), n, c, _stream()), "apply")
    elif tile:
        check(lib.usc_bn_tile_forward(None, 0, _p(yb), n, c, _p(t["gamma"]), _p(t["beta"]), rc.EPS, rc.MOMENTUM, _p(rm), _p(rv),
                                      nbt.ptr(), *sargs, None, 1, _p(direct), ws.ptr(), ws.nbytes, _stream()), "tile forward")
    else:
        check(lib.usc_bn_forward_stats(_p(yb), n, c, _p(t["gamma"]), _p(t["beta"]), rc.EPS, rc.MOMENTUM, _p(rm), _p(rv),
                                       nbt.ptr(), *sargs, ws.ptr(), ws.nbytes, _stream()), "forward stats")
        check(lib.usc_bn_apply(_p(yb), sargs[2], sargs[3], None, 1, _p(direct), n, c, _stream()), "apply")
    torch.cuda.synchronize()
    assert ws.guards_intact()
    assert rc.same_bits(out.detach(), direct) and rc.same_bits(stats_saved, stats), "unit forward differs from the direct call"
    assert rc.same_bits(bn.running_mean, rm) and rc.same_bits(bn.running_var, rv)
    assert int(bn.num_batches_tracked) == NBT0 + int(training) and nbt.value() == NBT0 + int(training)
    dg, db, dyb = torch.empty(c, device=device), torch.empty(c, device=device), torch.empty((n, c), device=device)
    dout = t["dy"].clone()
    if tile:
        check(lib.usc_bn_tile_backward(None, 0, 0, _p(dout), _p(yb), _p(direct), sargs[0], sargs[1], _p(t["gamma"]), n, c,
                                       int(training), 0, _p(dg), _p(db), _p(dyb), None, ws.ptr(), ws.nbytes, _stream()),
              "tile backward")
    else:
        red = torch.empty((2, c), device=device)
        check(lib.usc_bn_backward_reduce(_p(yb), _p(dout), _p(direct), sargs[0], sargs[1], n, c, int(training), 0, _p(dg),
                                         _p(db), _p(red[0]), _p(red[1]), ws.ptr(), ws.nbytes, _stream()), "reduce")
        check(lib.usc_bn_backward_dx(_p(yb), _p(dout), _p(direct), sargs[0], sargs[1], _p(t["gamma"]), _p(red[0]), _p(red[1]),
                                     _p(dyb), None, n, c, _stream()), "dx")
    torch.cuda.synchronize()
    assert ws.guards_intact()
    assert rc.same_bits(bn.weight.grad, dg) and rc.same_bits(bn.bias.grad, db), "unit dgamma / dbeta differ from the direct call"
    assert torch.equal(x.grad, dyb), "unit dx differs from the direct call"        # (identity weight: dx = dy, up to -0.0)
    # ---- and against float64, with the mask and the saved statistics as inputs
    rb = rc.ref_backward(t["x"], t["dy"], direct, stats[0], stats[1], t["gamma"], int(training))
    fr = rc.backward_fractions(dict(dbeta=bn.bias.grad, dgamma=bn.weight.grad, dx=x.grad), rb)
    _within("unit " + ("tile" if tile else "two-launch") + (" training" if training else " eval"), case, fr)
    if not training:
        g = torch.where(direct > 0, t["dy"], torch.zeros_like(t["dy"])).double()
        plain = t["gamma"].double() * stats[1].double() * g
        assert rc.elem_ratio(x.grad, plain, plain.abs()) <= 1.0, "eval mode: dx is not gamma * invstd * g"
        assert bool(bn.weight.grad.any()) and bool(bn.bias.grad.any())


# ------------------------------------------------------------------------------------------------- ReLU
@pytest.mark.parametrize("numel", rc.RELU_NUMELS)
def test_relu_forward_and_backward(device, numel):
    y_in = rc.mask_input(1, numel, numel).to(device)                         # both zeros, tiny positives
    x = torch.where(torch.rand_like(y_in) < 0.3, -torch.rand_like(y_in), y_in).contiguous()   # negatives, +0.0, -0.0, tiny
    dy = torch.randn((1, numel), generator=torch.Generator().manual_seed(numel)).to(device)
    y, dx = rc.GuardedF32(1, numel, device), rc.GuardedF32(1, numel, device)
    for _ in range(2):
        check(lib.usc_relu_fwd(_p(x), y.ptr(), numel, _stream()), "usc_relu_fwd")
        check(lib.usc_relu_bwd(_p(y_in), _p(dy), dx.ptr(), numel, _stream()), "usc_relu_bwd")
        torch.cuda.synchronize()
        assert y.guards_intact() and dx.guards_intact()
        assert torch.equal(y.t, x.clamp_min(0.0)) and bool((y.t >= 0).all())
        assert rc.same_bits(dx.t, torch.where(y_in > 0, dy, torch.zeros_like(dy)))


# ------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("c", rc.POOL_CASES, ids=_ids(rc.POOL_CASES))
def test_average_pooling(device, c):
    for mode in ("exact", "bounded"):
        t = rc.to_device(rc.pool_inputs(c, mode), device)
        ref, mag = rc.ref_pool(t["src"], t["nbr2"], t["row_of"], c.c)
        out = rc.GuardedF32(c.n_coarse, c.c, device)
        mask = torch.full((4096 + c.n_coarse * c.c + 4096,), 0xA5, dtype=torch.uint8, device=device)
        for m in (None, mask[4096:]):
            check(lib.usc_avgpool_down2_ex(_p(t["src"]), c.c, c.ld, _p(t["row_of"]), _p(t["nbr2"]), c.n_coarse,
                                           out.ptr() if m is None else None, _p(m), _stream()), "usc_avgpool_down2_ex")
        torch.cuda.synchronize()
        assert out.guards_intact() and bool((mask[:4096] == 0xA5).all()) and bool((mask[-4096:] == 0xA5).all()), c.name
        assert not bool(out.t[0].any()), "a coarse row without children must be 0"
        if mode == "exact":
            assert torch.equal(out.t.double(), ref), (c.name, "exact")
            want = (torch.sigmoid(out.t) < 0.5).view(-1).to(torch.uint8)
            assert torch.equal(mask[4096:-4096], want), (c.name, "mask_out")
        else:
            _within("pooling", c, dict(out=rc.elem_ratio(out.t, ref, mag)))
        out2 = rc.GuardedF32(c.n_coarse, c.c, device)
        check(lib.usc_avgpool_down2_ex(_p(t["src"]), c.c, c.ld, _p(t["row_of"]), _p(t["nbr2"]), c.n_coarse, out2.ptr(), None,
                                       _stream()), "usc_avgpool_down2_ex")
        torch.cuda.synchronize()
        assert rc.same_bits(out.t, out2.t)


# ------------------------------------------------------------------------------------------------- gather / scatter
@pytest.mark.parametrize("c", rc.MOVE_CASES, ids=_ids(rc.MOVE_CASES))
def test_gather_and_scatter_rows(device, c):
    idx = rc.move_indices(c).to(device)
    named = torch.zeros(c.n_src, dtype=torch.bool, device=device)
    named[idx] = True
    for mode in ("exact", "bounded"):
        table = rc.move_values((c.n_src, c.c), mode, c.seed).to(device)
        rows = rc.move_values((c.n, c.c), mode, c.seed + 9).to(device)
        prior = rc.move_values((c.n_src, c.c), mode, c.seed + 19).to(device)
        out = rc.GuardedF32(c.n, c.c, device)
        check(lib.usc_gather_rows(_p(table), c.c, _p(idx), c.n, out.ptr(), _stream()), "usc_gather_rows")
        torch.cuda.synchronize()
        assert out.guards_intact() and rc.same_bits(out.t, table[idx]), (c.name, mode, "gather")
        if c.kind != "dup":
            dst = rc.GuardedF32(c.n_src, c.c, device)
            check(lib.usc_scatter_rows_unique(_p(rows), c.c, _p(idx), c.n, dst.ptr(), _stream()), "usc_scatter_rows_unique")
            torch.cuda.synchronize()
            assert dst.guards_intact() and torch.equal(dst.pattern_rows(), ~named), (c.name, mode, "rows no index names")
            assert rc.same_bits(dst.t[idx], rows), (c.name, mode, "scatter")
            dst = rc.GuardedF32(c.n_src, c.c, device, init=prior)
            for _ in range(2):                                              # launch after launch into one buffer
                check(lib.usc_scatter_rows_unique_add(_p(rows), c.c, _p(idx), c.n, dst.ptr(), _stream()),
                      "usc_scatter_rows_unique_add")
            torch.cuda.synchronize()
            want = prior.clone()
            want[idx] = (prior[idx] + rows) + rows
            assert dst.guards_intact() and rc.same_bits(dst.t, want), (c.name, mode, "scatter add, unique")
        dst = rc.GuardedF32(c.n_src, c.c, device, init=prior)
        check(lib.usc_scatter_add_rows(_p(rows), c.c, _p(idx), c.n, dst.ptr(), _stream()), "usc_scatter_add_rows")
        torch.cuda.synchronize()
        ref = prior.double().index_add_(0, idx, rows.double())
        mag = prior.double().abs().index_add_(0, idx, rows.double().abs())
        assert dst.guards_intact() and rc.same_bits(dst.t[~named], prior[~named]), (c.name, mode, "rows no index names")
        if mode == "exact":
            assert torch.equal(dst.t.double(), ref), (c.name, "atomic scatter, exact")
        else:
            _within("atomic scatter", c, dict(out=rc.elem_ratio(dst.t, ref, mag)))
        if mode == "exact" or c.kind != "dup":                              # (bounded duplicates: the order is free)
            dst2 = rc.GuardedF32(c.n_src, c.c, device, init=prior)
            check(lib.usc_scatter_add_rows(_p(rows), c.c, _p(idx), c.n, dst2.ptr(), _stream()), "usc_scatter_add_rows")
            torch.cuda.synchronize()
            assert rc.same_bits(dst.t, dst2.t)


# ------------------------------------------------------------------------------------------------- segments
def _i64_guarded(n, device):
    g = rc.GuardedF32(1, 2 * max(n, 1), device)                             # i64 payload in the same guarded buffers
    return g, g.raw.view(torch.int64)[:n]


@pytest.mark.parametrize("c", rc.SEG_CASES, ids=_ids(rc.SEG_CASES))
def test_segment_csr_and_means(device, c):
    seg = rc.segment_ids(c).to(device)
    order_g, order = _i64_guarded(c.n, device)
    off_g, seg_off = _i64_guarded(c.S + 1, device)
    ws = rc.GuardedWs(lib.usc_segment_csr_ws_bytes(c.n, c.S), device)
    for rep in range(2):
        check(lib.usc_segment_csr(_p(seg) if c.n else None, c.n, c.S, _p(order) if c.n else None, _p(seg_off), ws.ptr(),
                                  ws.nbytes, _stream()), "usc_segment_csr")
        torch.cuda.synchronize()
        assert order_g.guards_intact() and off_g.guards_intact() and ws.guards_intact(), (c.name, "usc_segment_csr")
        counts = torch.bincount(seg, minlength=c.S)
        assert torch.equal(seg_off, torch.cat([torch.zeros(1, dtype=torch.int64, device=device), counts.cumsum(0)]))
        assert torch.equal(order, torch.sort(seg, stable=True).indices), (c.name, "the order is not the stable sort")
    for mode in ("exact", "bounded"):
        src = rc.segment_values(c, mode).to(device)
        if c.n == 0:
            src = torch.zeros((1, c.c), device=device)[:0]
        calls = (("mean", lib.usc_segment_mean_fwd, False), ("mean_nonzero", lib.usc_segment_mean_nonzero, True),
                 ("max_nonzero", lib.usc_segment_max_nonzero, True))
        for m, fn, counted in calls:
            ref, mag, cnt = rc.ref_segment(src, seg, c.S, m)
            out = rc.GuardedF32(c.S, c.c, device)
            nz_g, nz = _i64_guarded(c.S, device)
            src_p = _p(src) if c.n else _p(torch.zeros(4, device=device))
            ord_p = _p(order) if c.n else _p(torch.zeros(1, dtype=torch.int64, device=device))
            args = (src_p, c.c, ord_p, _p(seg_off), c.S, out.ptr()) + ((_p(nz),) if counted else ())
            check(fn(*args, _stream()), m)
            torch.cuda.synchronize()
            assert out.guards_intact() and nz_g.guards_intact(), (c.name, m)
            if counted:
                assert torch.equal(nz, cnt), (c.name, m, "nonzero_cnt")
            assert not bool(out.t[cnt == 0].any()), (c.name, m, "a segment without rows must be 0")
            ok = torch.ones_like(cnt, dtype=torch.bool) if m == "max_nonzero" else rc.is_pow2(cnt)
            if mode == "exact":
                assert torch.equal(out.t[ok].double(), ref[ok]), (c.name, m, "exact")
            _within("segment " + m, c, dict(out=rc.elem_ratio(out.t, ref, mag)))
            out2 = rc.GuardedF32(c.S, c.c, device)
            check(fn(*((src_p, c.c, ord_p, _p(seg_off), c.S, out2.ptr()) + ((None,) if counted else ())), _stream()), m)
            torch.cuda.synchronize()
            assert rc.same_bits(out.t, out2.t), (c.name, m, "a second launch gave other bits")
        # backward of the mean: dsrc[i] = dout[seg[i]] / count[seg[i]], the copy pattern bit for bit
        if c.n:
            dout = rc.move_values((c.S, c.c), mode, c.seed + 3).to(device)
            dsrc = rc.GuardedF32(c.n, c.c, device)
            check(lib.usc_segment_mean_bwd(_p(dout), c.c, _p(seg), _p(seg_off), c.n, dsrc.ptr(), _stream()), "usc_segment_mean_bwd")
            torch.cuda.synchronize()
            inv = (1.0 / counts.float())[seg][:, None]
            assert dsrc.guards_intact() and rc.same_bits(dsrc.t, dout[seg] * inv), (c.name, "segment mean backward")
            if mode == "exact":
                ok = rc.is_pow2(counts)[seg]
                assert torch.equal(dsrc.t[ok].double(), (dout.double()[seg] / counts.double()[seg][:, None])[ok])


def test_print_the_bound_fractions_per_family():
    """A record, not a check: the largest fraction of its bound each quantity used, per family."""
    print("\nfamily / cases / largest |err| / bound per quantity")
    for fam, r in RATIOS.items():
        print(f"{fam:<28} {r['cases']:4d}  " + "  ".join(f"{k} {v:.3f}" for k, v in r.items() if k != "cases"))
