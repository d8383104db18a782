"""The whole Res16UNet trunk as ONE step program each way (csrc/units.hip: usc_program_run).

The reference walks `Res16UNetBase.forward` (models/res16unet.py:224-297) module by module from the interpreter and
autograd walks it back node by node.  units.py already made a residual block one autograd node and a unit one C call;
what was left on the host per training step were ~190 Python-issued native calls, ~450 small tensor allocations and 33
autograd nodes for the trunk: 3 ms forward and 3.5 ms backward of the 13 ms the host needs to issue a 150 k-voxel step
(tools/host_profile.py), and most of the 15.5 ms of a 20 k-voxel step, which is host-bound.

Here the trunk is ONE autograd node:
* the walk is planned once per model (`_plan`: the units, their inputs / residuals / outputs as symbolic buffers, the
  skip concatenations) — the topology of `_trunk`, nothing else;
* per forward pass ONE arena holds every activation (conv outputs, normalised outputs, BN statistics, concatenations);
  the steps are filled in with raw pointers and `usc_program_run` launches the 62 units and 4 concatenations from C;
* the backward pass is the reverse walk over the same plan: ONE gradient arena, the units' backward steps (parameter
  gradients added into p.grad in place, weight gradients of a level's same-shape convolutions queued and issued as
  grouped launches inside the library), column splits for the concatenations and fan-in adds where a tensor has several
  consumers; it is cut into one C call per U-Net stage so that a gradient reducer hears about finished parameters
  while the earlier stages are still being issued (ops.GRAD_WRITTEN_HOOK).

Same kernels and the same arithmetic per unit as units.py (`usc_conv_bn_act_forward/backward`); features are bit-equal
to that path, gradients equal to rounding (different fan-in order).  Falls back to the per-block path whenever a piece
is not the plain form: a bias, a Bottleneck block, a parameter without an in-place gradient target, an open profiler
capture, `USC3D_BACKBONE_PROGRAM=0`.
A forward pass leaves a `_PassState`; a backward walk's gradient table holds `_Grad` entries; a last stage issued ahead
(`early_backward`) is an `_EarlyState` until the node's own backward has continued from it.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import torch

from . import ops, precision, units
from ._lib import STEP_ADD, STEP_CAT, STEP_SPLIT, STEP_UNIT_BWD, STEP_UNIT_FWD, STEP_UNIT_FWD_BF16, Step, check, lib

ENABLED = os.environ.get("USC3D_BACKBONE_PROGRAM", "1") == "1"
SAME, DOWN, UP = units.SAME, units.DOWN, units.UP
_ALIGN = 64          # floats (256 bytes)


class _Plan:
    """Symbolic walk of the trunk: `ops` in forward order, `bufs` id -> (level, channels), `levels` = ids of the five
    block outputs [s16, s8, s4, s2, s1], `act_floats[l]` / `grad_floats[l]` = floats per row of level l the activation /
    gradient arenas need, `n_bufs` for the alignment slack."""

    def __init__(self):
        self.ops, self.bufs, self.levels = [], {}, []
        self.input = None
        self.params = []

    def new(self, level, c):
        i = len(self.bufs)
        self.bufs[i] = (level, c)
        return i


def _plan(model):
    """-> _Plan, or None when the trunk contains something the step program does not cover."""
    from .MinkowskiEngine import MinkowskiBatchNorm, MinkowskiConvolution, MinkowskiConvolutionTranspose
    from .models.modules.resnet_block import BasicBlockBase
    pl = _Plan()

    def unit(stage, conv, norm, kind, level, x, res, relu):
        if not (conv.bias is None and isinstance(norm, MinkowskiBatchNorm) and norm.bn.affine
                and norm.bn.momentum is not None):
            raise NotImplementedError
        if kind == SAME and not (isinstance(conv, MinkowskiConvolution) and conv.stride == 1):
            raise NotImplementedError
        if kind == DOWN and not (isinstance(conv, MinkowskiConvolution) and conv.stride == 2 and conv.ksize == 2):
            raise NotImplementedError
        if kind == UP and not (isinstance(conv, MinkowskiConvolutionTranspose) and conv.stride == 2 and conv.ksize == 2):
            raise NotImplementedError
        lout = level + 1 if kind == DOWN else (level - 1 if kind == UP else level)
        y, out = pl.new(lout, conv.out_channels), pl.new(lout, conv.out_channels)
        pl.ops.append(dict(t="unit", stage=stage, conv=conv, bn=norm.bn, kind=kind, lin=level, lout=lout, x=x, res=res,
                           relu=relu, y=y, out=out, cin=conv.in_channels, cout=conv.out_channels,
                           ksize=conv.ksize, kvol=conv.kernel_volume))
        return out

    def blocks(stage, seq, level, x):
        for blk in seq:
            if not isinstance(blk, BasicBlockBase) or blk.conv1.stride != 1 or blk.conv2.stride != 1 \
                    or blk.conv1.kernel_volume == 1 or blk.conv1.ksize != blk.conv2.ksize:
                raise NotImplementedError
            a1 = unit(stage, blk.conv1, blk.norm1, SAME, level, x, None, True)
            r = x
            if blk.downsample is not None:
                ds = blk.downsample
                if len(ds) != 2 or ds[0].kernel_volume != 1:
                    raise NotImplementedError
                r = unit(stage, ds[0], ds[1], SAME, level, x, None, False)
            x = unit(stage, blk.conv2, blk.norm2, SAME, level, a1, r, True)
        return x

    try:
        pl.input = pl.new(0, model.conv0p1s1.in_channels)
        x = unit("conv0p1s1", model.conv0p1s1, model.bn0, SAME, 0, pl.input, None, True)
        skip = [x]
        for i, (cname, nname, bname) in enumerate(model._DOWN):
            x = unit(cname, getattr(model, cname), getattr(model, nname), DOWN, i, x, None, True)
            x = blocks(bname, getattr(model, bname), i + 1, x)
            skip.append(x)
        pl.levels = [x]
        top = len(model._DOWN)
        for j, (cname, nname, bname) in enumerate(model._UP):
            u = unit(cname, getattr(model, cname), getattr(model, nname), UP, top - j, x, None, True)
            s = skip[top - 1 - j]
            ca, cb = pl.bufs[u][1], pl.bufs[s][1]
            if ca % 4 or cb % 4:
                raise NotImplementedError
            c = pl.new(top - 1 - j, ca + cb)
            pl.ops.append(dict(t="cat", stage=cname, a=u, b=s, out=c, level=top - 1 - j, ca=ca, cb=cb))
            x = blocks(bname, getattr(model, bname), top - 1 - j, c)
            pl.levels.append(x)
    except (NotImplementedError, AttributeError):
        return None
    n_levels = top + 1
    pl.n_levels = n_levels
    act, grad = [0] * n_levels, [0] * n_levels
    n_act = n_grad = 0
    for op in pl.ops:
        if op["t"] == "unit":
            act[op["lout"]] += 2 * op["cout"]
            n_act += 3
            grad[op["lout"]] += 2 * op["cout"]          # dy, dres
            grad[op["lin"]] += 2 * op["cin"]            # dx (+ a temporary when the target cannot be accumulated into)
            n_grad += 4
        else:
            act[op["level"]] += op["ca"] + op["cb"]
            n_act += 1
            grad[op["level"]] += op["ca"] + op["cb"]
            n_grad += 2
    pl.act_floats, pl.grad_floats, pl.n_act, pl.n_grad = act, grad, n_act, n_grad
    pl.stat_floats = sum(4 * op["cout"] for op in pl.ops if op["t"] == "unit")
    seen, params = set(), []
    for op in pl.ops:
        if op["t"] == "unit":
            for p in (op["conv"].kernel, op["bn"].weight, op["bn"].bias):
                if id(p) not in seen:
                    seen.add(id(p))
                    params.append(p)
    pl.params = params
    # the last U-Net stage (transposed conv onto the finest map, concatenation, blocks): ops[early_from:], see early_backward
    pl.early_from = None
    if model._UP:
        last = (model._UP[-1][0], model._UP[-1][2])
        k = len(pl.ops)
        while k > 0 and pl.ops[k - 1]["stage"] in last:
            k -= 1
        first = pl.ops[k] if k < len(pl.ops) else None
        if first is not None and first["t"] == "unit" and first["kind"] == UP and first["x"] == pl.levels[-2]:
            pl.early_from = k
    return pl


def _module_key(model):
    """Identity of every module the plan references: a conversion that swaps modules after the first forward pass (a
    batch-norm conversion, a re-built block) must not be served the old plan, which holds the old modules' parameters.
    (The cached plan keeps references to the modules it uses, so none of THEIR ids can be handed to a new object while
    it is cached; ~30 us per call for the few hundred modules of the trunk — round-5 advice, left as it is.)"""
    return tuple(id(m) for m in model.modules())


def plan_of(model):
    cached = model.__dict__.get("_usc_program_plan")
    key = _module_key(model)
    if cached is None or cached[1] != key:
        cached = model.__dict__["_usc_program_plan"] = (_plan(model) or False, key)
    return cached[0] or None


class _Carver:
    """Hands out 256-byte aligned float ranges of one arena as raw device pointers."""

    def __init__(self, floats, device):
        self.arena = torch.empty(int(floats), dtype=torch.float32, device=device)
        self.base, self.off, self.cap = self.arena.data_ptr(), 0, int(floats)

    def take(self, n):
        off = self.off
        self.off = (off + int(n) + _ALIGN - 1) // _ALIGN * _ALIGN
        if self.off > self.cap:
            raise RuntimeError("step program: arena too small (planning bug)")
        return self.base + 4 * off, off

    def view(self, off, n, c):
        return self.arena[off:off + n * c].view(n, c)


class _Pool:
    """Gradient buffers of one backward pass: chunks allocated on demand, exact-size reuse of released ranges.  The
    steps run in order on ONE stream, so a range released after the step that last reads it may be handed to any later
    step (the weight gradients queued inside a usc_program_run call read their dy until that call returns: those are
    released when the stage's call is closed).  Peak ~1.5 GB for a 150 k-voxel scene instead of the 8 GB the sum of
    all gradient buffers would take."""

    def __init__(self, device, chunk_floats):
        self.device, self.chunk_floats = device, int(chunk_floats)
        self.chunks, self.base, self.off, self.cap = [], 0, 0, 0
        self.free = {}

    def take(self, n):
        n = (int(n) + _ALIGN - 1) // _ALIGN * _ALIGN
        lst = self.free.get(n)
        if lst:
            return lst.pop()
        if self.off + n > self.cap:
            self.cap = max(self.chunk_floats, n)
            t = torch.empty(self.cap, dtype=torch.float32, device=self.device)
            self.chunks.append(t)
            self.base, self.off = t.data_ptr(), 0
        p = self.base + 4 * self.off
        self.off += n
        return p

    def release(self, p, n):
        n = (int(n) + _ALIGN - 1) // _ALIGN * _ALIGN
        self.free.setdefault(n, []).append(p)


def usable(model, x):
    """May this forward pass run as a step program?"""
    if not (ENABLED and units.usable(x.F, None) and x.F.shape[0] > 0):
        return None
    pl = plan_of(model)
    if pl is None:
        return None
    if torch.is_grad_enabled():
        need = [p.requires_grad for p in pl.params]
        if any(need):
            # the backward walk writes EVERY unit's parameter gradients in place and returns no input gradient: a
            # partly frozen trunk, a parameter without a gradient buffer or an input that wants its own gradient go
            # through the per-block path, which hands gradients back through autograd
            if not all(need) or x.F.requires_grad:
                return None
            for p in pl.params:
                if ops._grad_target(p) is None:
                    return None
    return pl


_N_PLAIN_ARGS = 8        # _Trunk.forward's arguments in front of the parameters


# What one forward pass of the trunk leaves for its backward walk(s).  cm: coordinate manager; ts: the input's tensor stride;
# arena: _Carver; ptr: buffer id -> pointer; per op of the plan: stats_ptr (BN statistics), kmaps, bnrefs ((address, usc_bn
# descriptor)); rows: per level; split: op index -> split-bf16 planes, or None
_PassState = namedtuple("_PassState", "model plan cm ts feats arena ptr stats_ptr kmaps bnrefs rows split")
# an entry of a backward walk's gradient table: where the gradient of a buffer stands (read_only: an incoming gradient tensor)
_Grad = namedtuple("_Grad", "ptr read_only floats")


class _EarlyState:
    """The last stage issued ahead (early_backward), until the trunk node's own backward has continued from it: the graph
    task it was issued in, its gradient table, what the lane reads, the device index, the stage's parameters as written."""

    def __init__(self, task, G, keep, key, params):
        self.task, self.G, self.keep, self.key, self.params = task, G, keep, key, params


class _Trunk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, pl, cm, ts, bf16, split, holder, feats, *params):
        dev = feats.device
        settle_abandoned(dev)
        rows = [cm.coord_map(ts << l).n for l in range(pl.n_levels)]
        floats = sum(r * f for r, f in zip(rows, pl.act_floats)) + pl.stat_floats + (pl.n_act + 8) * _ALIGN
        car = _Carver(floats, dev)
        ptr, offs = {pl.input: feats.data_ptr()}, {}
        steps = (Step * len(pl.ops))()
        kcache = {}

        def kmap(op):
            key = (op["kind"], op["lin"], op["kvol"])
            k = kcache.get(key)
            if k is None:
                t = ts << op["lin"]
                if op["kind"] == SAME:
                    k = cm.kmap_identity(t) if op["kvol"] == 1 else cm.kmap_cube(t, op["ksize"])
                elif op["kind"] == DOWN:
                    k = cm.kmap_down(t)
                else:
                    k = cm.kmap_down(t >> 1)
                kcache[key] = k
            return k

        stats_ptr, kmaps, bnrefs = [], [], []
        for i, op in enumerate(pl.ops):
            st = steps[i]
            if op["t"] == "unit":
                n_out, cout = rows[op["lout"]], op["cout"]
                py, offs[op["y"]] = car.take(n_out * cout)
                po, offs[op["out"]] = car.take(n_out * cout)
                ps, _ = car.take(4 * cout)
                ptr[op["y"]], ptr[op["out"]] = py, po
                km = kmap(op)
                bdesc, _ = units._bn_desc(op["bn"], units._training(op["bn"]))
                bref = C.addressof(bdesc)                  # (the descriptor is kept alive by units._BN_DESC and `bnrefs`)
                st.op, st.kind, st.cin, st.cout, st.relu = STEP_UNIT_FWD, op["kind"], op["cin"], cout, int(op["relu"])
                st.map, st.bn = C.addressof(km.struct), bref
                st.x, st.W = ptr[op["x"]], op["conv"].kernel.data_ptr()
                wp = bf16.get(id(op["conv"].kernel)) if bf16 else None
                if wp is not None:                           # inference in bf16: packed weights (kept by `bf16`)
                    st.op, st.W = STEP_UNIT_FWD_BF16, wp.data_ptr()
                if split:                                    # training in split bf16: planes of this unit (0: f32)
                    st.split_planes = split.get(i, 0)
                st.residual = ptr[op["res"]] if op["res"] is not None else None
                st.y, st.stats, st.out = py, ps, po
                stats_ptr.append(ps)
                kmaps.append(km)
                bnrefs.append((bref, bdesc))
            else:
                n = rows[op["level"]]
                pc, offs[op["out"]] = car.take(n * (op["ca"] + op["cb"]))
                ptr[op["out"]] = pc
                st.op, st.a, st.b, st.dst, st.n, st.ca, st.cb = STEP_CAT, ptr[op["a"]], ptr[op["b"]], pc, n, op["ca"], op["cb"]
                stats_ptr.append(None)
                kmaps.append(None)
                bnrefs.append(None)
        wsb = lib.usc_program_ws_bytes(steps, len(pl.ops))
        ws = units.workspace(wsb, dev)
        check(lib.usc_program_run(steps, 0, len(pl.ops), ws.data_ptr(), ws.numel(), ops._stream()), "usc_program_run")
        outs = tuple(car.view(offs[b], rows[pl.bufs[b][0]], pl.bufs[b][1]) for b in pl.levels)
        ctx.state = _PassState(model, pl, cm, ts, feats, car, ptr, stats_ptr, kmaps, bnrefs, rows, split)
        ctx.holder = holder
        if holder is not None:
            holder.state = ctx.state
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        holder, state = ctx.holder, ctx.state
        pl, rows, dev = state.plan, state.rows, state.feats.device
        gar = _Pool(dev, max(rows[0] * 256, 1 << 20))
        lane = units._lane(dev)                  # weight-gradient lane (on by default): its launches read x and dy after
        if lane is not None:                     # this function has moved on -> nothing they read is re-used
            gar.release = lambda p_, n_: None
            state.arena.arena.record_stream(lane[0])
        keep = [g.contiguous() if g is not None else None for g in gouts]
        early = _take_early(holder)
        stream = ops._stream()
        if early is None:
            walk = _BackwardWalk(state, gar, {})
            for b, g in zip(pl.levels, keep):
                if g is not None:
                    walk.G[b] = _Grad(g.data_ptr(), True, g.numel())
            hi = len(pl.ops)
        else:
            # the last stage has been issued on the lane (early_backward): the walk continues from its gradient table behind
            # the event the lane recorded after the stage's chain.  The s1 argument is not used: that stage took its own.
            check(lib.usc_wgrad_lane_wait_chain(stream), "usc_wgrad_lane_wait_chain")
            walk = _BackwardWalk(state, gar, early.G)
            for b, g in zip(pl.levels[:-1], keep[:-1]):
                if g is None:
                    continue
                cur = walk.G.get(b)
                if cur is None:
                    walk.G[b] = _Grad(g.data_ptr(), True, g.numel())
                else:                            # the boundary buffer: the early stage's contribution + the decoder's
                    walk.add_step(cur.ptr, g.data_ptr(), g.numel())
            hi = pl.early_from
            # the stage's parameters are final, and reported only now: the optimizer's early step waits for an event of
            # the lane on ITS stream — the key-preparation stream in the shipped loop, which the decoder's backward needs
            ops._grad_written(*early.params)
            ops._params_final(early.params)
        walk.emit(hi, 0)
        steps, ns, segments = walk.steps, walk.ns, walk.segments
        wsb = lib.usc_program_ws_bytes(steps, ns)
        ws = units.workspace(wsb, dev)
        begin = 0
        # the lane's schedule (usc_wgrad_lane_hold): the fine decoder stages' weight gradients are noted, not launched,
        # until the walk reaches a stage whose maps cannot fill the chip; their parameters are reported then
        holding = lane is not None and units.LANE_HOLD_MIN_ROWS > units.LANE_RELEASE_ROWS > 0 and \
            any(min(rows[o["lin"]], rows[o["lout"]]) <= units.LANE_RELEASE_ROWS for o in pl.ops if o["t"] == "unit")
        unreported = []
        if holding:
            check(lib.usc_wgrad_lane_hold(1, units.LANE_HOLD_MIN_ROWS, units.LANE_RELEASE_ROWS, stream), "usc_wgrad_lane_hold")
        try:
            for end, plist in segments:
                if end > begin:
                    check(lib.usc_program_run(steps, begin, end, ws.data_ptr(), ws.numel(), stream), "usc_program_run")
                if holding and lib.usc_wgrad_lane_holding():
                    unreported.extend(plist)
                elif plist or unreported:
                    ops._grad_written(*unreported, *plist)   # finished stages are reported while the earlier ones are still issued
                    ops._params_final(unreported + plist)    # ... and are final: each unit's parameters are written once
                    unreported = []
                begin = end
            if holding:
                check(lib.usc_wgrad_lane_hold(0, 0, 0, stream), "usc_wgrad_lane_hold")
                if unreported:
                    ops._grad_written(*unreported)
                    ops._params_final(unreported)
        except BaseException:
            if holding:
                lib.usc_wgrad_lane_hold(-1, 0, 0, None)
            raise
        if lane is not None:
            for t in gar.chunks:
                t.record_stream(lane[0])
            units.queue_lane_join(units._dev_key(dev))
        if early is not None:         # the stage's buffers go when the lane has been joined (the join was queued first)
            _EARLY_OPEN.pop(early.key, None)
            ops.at_end_of_backward(early, early.keep.clear, outside="skip")
        if holder is not None:
            holder.state = None
        ctx.state = None
        return (None,) * _N_PLAIN_ARGS + (None,) * len(pl.params)


class _BackwardWalk:
    """The reverse walk over the plan as backward steps: the units' backward steps, column splits for the concatenations and
    fan-in adds where a tensor has several consumers.  `G`: buffer id -> _Grad — the gradient table, which a walk over the first part of the plan hands to the walk over the rest
    (early_backward).  `segments`: one (end step, parameters it finished) per U-Net stage."""

    def __init__(self, state, gar, G):
        self.state, self.gar, self.G = state, gar, G
        self.steps = (Step * (3 * len(state.plan.ops) + 8))()
        self.ns = 0
        self.segments = []

    def add_step(self, dst, src, n):
        st = self.steps[self.ns]
        self.ns += 1
        st.op, st.dst, st.a, st.n = STEP_ADD, dst, src, n

    def emit(self, hi, lo):
        """Steps of pl.ops[lo:hi], last first."""
        state = self.state
        pl, ptr, rows, split = state.plan, state.ptr, state.rows, state.split
        G, gar, steps, add_step = self.G, self.gar, self.steps, self.add_step
        held_dy = []                             # dy buffers the current stage's queued weight gradients still read
        cur_params, stage = [], None

        def contribute(bid, numel, can_accumulate):
            """Where the next contribution to the gradient of buffer `bid` goes -> (pointer, accumulate flag, finish):
            finish() is called after the producing step has been emitted (fan-in add when the target could not be
            accumulated into: an incoming gradient tensor is never written, and the pair-list forms only write)."""
            cur = G.get(bid)
            if cur is None:
                p = gar.take(numel)
                G[bid] = _Grad(p, False, numel)
                return p, 0, None
            if can_accumulate and not cur.read_only:
                return cur.ptr, 1, None
            p = gar.take(numel)
            if cur.read_only:                    # new buffer = this contribution + the incoming gradient; ours from now on
                def fin(p=p, old=cur.ptr):
                    add_step(p, old, numel)
                    G[bid] = _Grad(p, False, numel)
            else:
                def fin(p=p, old=cur.ptr):
                    add_step(old, p, numel)
                    gar.release(p, numel)
            return p, 0, fin

        def consumed(bid):
            """The gradient of buffer `bid` has been read by its producer's backward step: give the range back."""
            cur = G.pop(bid, None)
            if cur is not None and not cur.read_only:
                gar.release(cur.ptr, cur.floats)

        for i in range(hi - 1, lo - 1, -1):
            op = pl.ops[i]
            if op["stage"] != stage:
                if stage is not None:
                    self.segments.append((self.ns, cur_params))
                    cur_params = []
                    for p_, n_ in held_dy:       # the stage's C call flushes its queued weight gradients before it returns
                        gar.release(p_, n_)
                    held_dy = []
                stage = op["stage"]
            if op["t"] == "cat":
                g = G.get(op["out"])
                if g is None:
                    continue
                n = rows[op["level"]]
                pa, _, fa = contribute(op["a"], n * op["ca"], False)
                cur_b = G.get(op["b"])
                if cur_b is not None and not cur_b.read_only:
                    pb, acc_b, fb = cur_b.ptr, 1, None
                else:
                    pb, acc_b, fb = contribute(op["b"], n * op["cb"], False)
                st = steps[self.ns]
                self.ns += 1
                st.op, st.a, st.dst, st.dst2, st.n, st.ca, st.cb, st.accumulate = STEP_SPLIT, g.ptr, pa, pb, n, op["ca"], \
                    op["cb"], acc_b
                for f in (fa, fb):
                    if f is not None:
                        f()
                consumed(op["out"])
                continue
            g = G.get(op["out"])
            if g is None:
                continue                          # nothing downstream asked for this unit's gradient
            n_out, n_in, cin, cout = rows[op["lout"]], rows[op["lin"]], op["cin"], op["cout"]
            pdy = gar.take(n_out * cout)
            pres, fres = None, None
            if op["res"] is not None:
                pres, _, fres = contribute(op["res"], n_out * cout, False)
            need_dx = op["x"] != pl.input
            pdx, acc, fdx = (None, 0, None)
            if need_dx:
                pdx, acc, fdx = contribute(op["x"], n_in * cin, op["kind"] != DOWN)
            conv, bn = op["conv"], op["bn"]
            tW, tg, tb = ops._grad_target(conv.kernel), ops._grad_target(bn.weight), ops._grad_target(bn.bias)
            if tW is None or tg is None or tb is None:
                raise RuntimeError("step program: a parameter lost its in-place gradient target between forward and "
                                   "backward (keep p.grad allocated: optimizer.zero_grad(set_to_none=False))")
            st = steps[self.ns]
            self.ns += 1
            st.op, st.kind, st.cin, st.cout = STEP_UNIT_BWD, op["kind"], cin, cout
            st.map, st.bn = C.addressof(state.kmaps[i].struct), state.bnrefs[i][0]
            st.x, st.W = ptr[op["x"]], conv.kernel.data_ptr()
            st.y, st.stats = ptr[op["y"]], state.stats_ptr[i]
            st.out = ptr[op["out"]] if op["relu"] else None
            st.dout, st.dy, st.dres, st.dx, st.dx_accumulate = g.ptr, pdy, pres, pdx, acc
            st.dW, st.dW_accumulate, st.dgamma, st.dbeta, st.dbn_accumulate = tW.data_ptr(), 1, tg.data_ptr(), \
                tb.data_ptr(), 1
            st.defer_wgrad = int(units.GROUP_WGRAD)
            if split:                            # the planes this unit's forward ran in
                st.split_planes = split.get(i, 0)
            cur_params.extend((conv.kernel, bn.weight, bn.bias))
            for f in (fres, fdx):
                if f is not None:
                    f()
            consumed(op["out"])
            if st.defer_wgrad and op["kind"] == SAME and op["kvol"] > 1:
                held_dy.append((pdy, n_out * cout))
            else:
                gar.release(pdy, n_out * cout)
        self.segments.append((self.ns, cur_params))


# ---- the last U-Net stage ahead of the rest ----------------------------------------------------------------------------
# The backward of the last stage (the transposed convolution onto the stride-1 map, the skip concatenation, the blocks at
# that width) needs the gradient of the s1 output and nothing else.  A caller that has that gradient before autograd
# reaches the trunk's node — models/mask3d.py: it is the sum of the mask heads' input gradients, which the criterion hands
# back all at once — issues that stage on the weight-gradient lane (usc_program_run_lane) while the compute stream goes
# through the decoder's backward; _Trunk.backward then continues from the stage's gradient table.
# USC3D_EARLY_STAGE=0: the walk is issued whole by _Trunk.backward, as before.
EARLY_STAGE = os.environ.get("USC3D_EARLY_STAGE", "1") == "1"
EARLY_RUNS = 0                  # stages issued ahead so far (tests, tools)
_EARLY_WS = {}                  # device index -> scratch of the early range (the shared one serves other streams meanwhile)
_EARLY_OPEN = {}                # device index -> the early state whose continuation has not run yet


class TrunkHandle:
    """What a forward pass of the trunk leaves for early_backward: the node's state, and between early_backward and the
    node's own backward the stage's gradient table."""

    __slots__ = ("state", "early", "__weakref__")

    def __init__(self):
        self.state, self.early = None, None


def handle_of(s1_features):
    """The TrunkHandle of the forward pass that produced this stride-1 output (None: not a step program's)."""
    return getattr(s1_features, "_usc_trunk", None)


def early_possible(handle):
    """May the last stage of this forward pass be issued ahead?  Needs the switch, a lane and no gradient reducer (its
    bucket order follows the order in which gradients are reported written)."""
    if not (EARLY_STAGE and handle is not None and handle.state is not None and handle.early is None):
        return False
    if ops.GRAD_WRITTEN_HOOK is not None:
        return False
    return units._lane(handle.state.feats.device) is not None


def _early_ws(nbytes, device):
    key = units._dev_key(device)
    ws = _EARLY_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _EARLY_WS[key] = torch.empty(int(nbytes * 1.25) + (1 << 20), dtype=torch.uint8, device=device)
    return ws


def early_backward(handle, g_s1, keep=()):
    """Issue the last stage's backward for the s1 gradient `g_s1` on the lane, behind the current stream (which may be the
    lane itself); the trunk node's own backward, later in the same backward pass, continues from there.  `keep`: whatever
    else the lane reads on the caller's behalf, held with the stage's own buffers until the lane has been joined."""
    global EARLY_RUNS
    if not early_possible(handle):
        raise RuntimeError("program.early_backward: not possible for this forward pass (program.early_possible)")
    state = handle.state
    pl, rows, dev = state.plan, state.rows, state.feats.device
    lane_st = units._lane(dev)[0]
    key = units._dev_key(dev)
    settle_abandoned(dev)
    g = g_s1.contiguous()
    if tuple(g.shape) != (rows[0], pl.bufs[pl.levels[-1]][1]) or g.dtype != torch.float32:
        raise RuntimeError("program.early_backward: the gradient does not have the s1 output's shape")
    # buffers of the stage: a pool of their own, nothing handed out twice (the lane and, behind the chain's event, the
    # compute stream read them), alive until the lane has been joined
    gar = _Pool(dev, max(rows[0] * 256, 1 << 20))
    gar.release = lambda p_, n_: None
    walk = _BackwardWalk(state, gar, {pl.levels[-1]: _Grad(g.data_ptr(), True, g.numel())})
    walk.emit(len(pl.ops), pl.early_from)
    state.arena.arena.record_stream(lane_st)
    g.record_stream(lane_st)
    for t in gar.chunks:
        t.record_stream(lane_st)
    ws = _early_ws(lib.usc_program_ws_bytes(walk.steps, walk.ns), dev)
    ws.record_stream(lane_st)
    early = _EarlyState(ops._graph_task(), walk.G, [gar, g, walk.steps, ws, state, list(keep)], key,
                        [p for _, plist in walk.segments for p in plist])
    _EARLY_OPEN[key] = early
    try:
        check(lib.usc_program_run_lane(walk.steps, 0, walk.ns, ws.data_ptr(), ws.numel(), ops._stream()),
              "usc_program_run_lane")
    except BaseException:
        lib.usc_wgrad_lane_hold(-1, 0, 0, None)
        raise
    handle.early = early
    EARLY_RUNS += 1
    units.queue_lane_join(key)


def _take_early(holder):
    early = None if holder is None else holder.early
    if early is None:
        return None
    holder.early = None
    if early.task >= 0 and early.task != ops._graph_task():      # (< 0: issued by a direct call, outside any pass)
        raise RuntimeError("step program: the last stage was issued ahead in another backward pass than this one")
    return early


def settle_abandoned(device=None):
    """After a backward pass that raised between early_backward and the trunk's own backward: the lane still runs (or has
    run) that stage, nobody continued from it and the engine dropped the queued join.  The current stream waits for the
    lane, nothing stays noted, the stage's gradient table is dropped.  Called by the next forward pass and the next
    early_backward; a training loop that reuses the gradient buffers after a failed pass calls it before it zeroes them."""
    key = units._dev_key(device)
    state = _EARLY_OPEN.pop(key, None)
    if state is None:
        return False
    lib.usc_wgrad_lane_hold(-1, 0, 0, None)
    with torch.cuda.device(key):
        units.join_lane()
    state.G = None
    state.keep.clear()
    return True


def trunk(model, x):
    """-> (list of the five block outputs as feature matrices [s16, s8, s4, s2, s1]) or None when the step program
    does not apply to this model / tensor / gradient configuration."""
    pl = usable(model, x)
    if pl is None:
        return None
    cm, ts = x.coordinate_manager, x._ts()
    feats = x.F.contiguous()
    # bf16 inference (precision.py): id(conv weight) -> packed bf16 weights, decided here (outside the Function, whose
    # forward always runs with gradients off); None when every unit runs in f32
    bf16 = None
    if precision.bf16_active():
        bf16 = {}
        for op in pl.ops:
            if op["t"] == "unit":
                wp = precision.unit_weights(op["conv"].kernel, op["kind"] == SAME, cm.coord_map(ts << op["lout"]).n)
                if wp is not None:
                    bf16[id(op["conv"].kernel)] = wp
    # split-bf16 training (precision.py): index of the unit in the plan -> planes, decided here for the same reason; None
    # when every unit runs in f32 (the default: the steps are then exactly the f32 program's)
    split = None
    if precision.current_training() != "f32" and torch.is_grad_enabled():
        split = {}
        for i, op in enumerate(pl.ops):
            if op["t"] == "unit":
                planes = precision.train_planes(op["conv"].kernel, op["kind"] == SAME, cm.coord_map(ts << op["lout"]).n)
                if planes:
                    split[i] = planes
        split = split or None
    holder = TrunkHandle() if (EARLY_STAGE and torch.is_grad_enabled() and pl.early_from is not None) else None
    outs = list(_Trunk.apply(model, pl, cm, ts, bf16, split, holder, feats, *pl.params))
    if holder is not None and holder.state is not None:
        outs[-1]._usc_trunk = holder
    return outs
