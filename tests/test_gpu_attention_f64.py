"""The decoder's attention kernels (csrc/attention.hip: usc_attn_fwd / usc_attn_bwd with their mask pack, combine and dq
reduce passes, usc_self_attn_fwd / usc_self_attn_bwd) on the MI355X, element-wise against float64 references computed on
the card with plain torch operators (tests/attention_cases.py).

Each case runs through the C entry points (unscene3d_amd._lib, so the case decides the shape, not the Python
dispatcher).  o, lse, dq, dk and dv are interior slices of larger buffers whose guards must keep their pattern; the
workspace has exactly usc_attn_ws_bytes bytes, starts filled with its byte pattern (a partial of an empty split that a
kernel does not write shows) and has an intact guard behind it; the columns L .. stride - 1 of lse hold NaN when the
backward runs.  Fully masked rows must give o = +0.0 and lse = +inf bit for bit and exactly zero gradients, count mode
(tests/attention_cases.py) must stay within two roundings, repeated launches must give the same bits.  The last test
prints the largest fraction of each bound a family used (profiles/attention_f64_ratios.txt is that table of one run: a
record; it is where the accuracy of the fast exponential on the card is written down)."""

import pytest
import torch

import attention_cases as ac
from unscene3d_amd._lib import lib

pytestmark = pytest.mark.gpu

RATIOS = {}                                   # family -> {quantity: largest fraction of its bound}, "cases": n
NAN = float("nan")


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
    return all(ac.same_bits(a[k].t, b[k].t) for k in a)


def _mask8(t):
    return None if t["mask"] is None else t["mask"].contiguous().view(torch.uint8)


def _as3(buf, c, n):
    """The [n, B, E] view of a guarded [n * B, E] output."""
    return buf.t.view(n, c.B, c.E)


def _workspace(c, device, short=0):
    if not c.masked:
        return None
    ws = ac.GuardedWs(lib.usc_attn_ws_bytes(c.L, c.S, c.B, c.H) - short, device)
    assert ws.nbytes + short == sum(ac.ws_layout(c.L, c.S, c.B, c.H, ac.planned(c.S, c.B, c.H)[0]))
    return ws


def _forward(c, t, device, ws=None, L=None, E=None, short=0):
    """(code, dict(o, lse), ws): one forward launch into guarded outputs; L / E override what the call is told."""
    stride = ac.lse_stride(c.L)
    o = dict(o=ac.GuardedF32(c.L * c.B, c.E, device), lse=ac.GuardedF32(c.B * c.H, stride, device))
    L, E = c.L if L is None else L, c.E if E is None else E
    if c.masked:
        ws = _workspace(c, device, short) if ws is None else ws
        code = lib.usc_attn_fwd(_p(t["q"]), _p(t["k"]), _p(t["v"]), _p(_mask8(t)), L, c.S, c.B, c.H, E, _p(o["o"]),
                                _p(o["lse"]), ws.ptr(), ws.nbytes, _stream())
    else:
        code = lib.usc_self_attn_fwd(_p(t["q"]), _p(t["k"]), _p(t["v"]), L, c.B, c.H, E, _p(o["o"]), _p(o["lse"]), _stream())
    torch.cuda.synchronize()
    assert _intact(ws, *o.values()), (c.name, "the forward wrote outside its outputs or workspace")
    if code == 0:
        pad = o["lse"].raw.view(c.B * c.H, stride)[:, c.L:]
        assert bool((pad == ac.PATTERN).all()), (c.name, "lse written beyond column L")
    return code, o, ws


def _backward(c, t, o32, lse32, device, ws=None, bits_in_ws=0, L=None, E=None, short=0):
    """(code, dict(dq, dk, dv)): one backward launch into guarded outputs from the given f32 o [L, B, E] and lse
    [B * H, stride]."""
    o = dict(dq=ac.GuardedF32(c.L * c.B, c.E, device), dk=ac.GuardedF32(c.S * c.B, c.E, device),
             dv=ac.GuardedF32(c.S * c.B, c.E, device))
    L, E = c.L if L is None else L, c.E if E is None else E
    if c.masked:
        ws = _workspace(c, device, short) if ws is None else ws
        code = lib.usc_attn_bwd(_p(t["q"]), _p(t["k"]), _p(t["v"]), _p(_mask8(t)), _p(o32), _p(lse32), _p(t["dO"]), L, c.S,
                                c.B, c.H, E, _p(o["dq"]), _p(o["dk"]), _p(o["dv"]), bits_in_ws, ws.ptr(), ws.nbytes,
                                _stream())
    else:
        code = lib.usc_self_attn_bwd(_p(t["q"]), _p(t["k"]), _p(t["v"]), _p(o32), _p(lse32), _p(t["dO"]), L, c.B, c.H, E,
                                     _p(o["dq"]), _p(o["dk"]), _p(o["dv"]), _stream())
    torch.cuda.synchronize()
    assert _intact(ws, *o.values()), (c.name, "the backward wrote outside its outputs or workspace")
    return code, o


def _gradients(c, o):
    return _as3(o["dq"], c, c.L), _as3(o["dk"], c, c.S), _as3(o["dv"], c, c.S)


def _tensors(c, device, count=False):
    t = ac.count_inputs(c) if count else ac.attn_inputs(c)
    return ac.to_device({k: t[k] for k in ("q", "k", "v", "dO", "mask")}, device)


def _nan_padded(lse, L):
    """A copy of lse [B * H, stride] with NaN in the columns L .. stride - 1."""
    out = lse.clone()
    out[:, L:] = NAN
    return out


# ------------------------------------------------------------------------------------------------- forward
def _forward_case(device, c, family):
    t = _tensors(c, device)
    code, o, _ = _forward(c, t, device)
    assert code == 0
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
    got_o = _as3(o["o"], c, c.L)
    assert ac.dead_rows_exact(got_o, o["lse"].t, fw), (c.name, "a fully masked row is not o = +0.0, lse = +inf")
    _within(family, c, ac.forward_fractions(got_o, o["lse"].t, fw))
    if c.repeat:
        assert _same(o, _forward(c, t, device)[1]), (c.name, "a second launch gave other bits")


def _count_case(device, c):
    t = _tensors(c, device, count=True)
    code, o, _ = _forward(c, t, device)
    assert code == 0
    _within("count mode", c, ac.count_fractions(_as3(o["o"], c, c.L), o["lse"].t, *ac.ref_count(t["v"], t["mask"], c.H, c.L)))


@pytest.mark.parametrize("c", ac.CROSS_CASES, ids=_ids(ac.CROSS_CASES))
def test_cross_forward(device, c):
    _forward_case(device, c, "cross forward")


@pytest.mark.parametrize("c", ac.CROSS_CASES, ids=_ids(ac.CROSS_CASES))
def test_cross_forward_count_mode(device, c):
    _count_case(device, c)


# ------------------------------------------------------------------------------------------------- backward
def _standalone_case(device, c, family):
    """The backward on its own: o and lse are the float64 reference rounded to f32 (+inf on fully masked rows), the mask
    is packed by this call into a fresh pattern-filled workspace."""
    t = _tensors(c, device)
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
    o32, lse32 = ac.saved_forward(fw, ac.lse_stride(c.L))
    refs = ac.ref_backward(t["q"], t["k"], t["v"], t["mask"], t["dO"], o32, lse32, c.H)
    del fw
    code, o = _backward(c, t, o32, lse32, device)
    assert code == 0
    _within(family, c, ac.backward_fractions(*_gradients(c, o), refs))
    if c.repeat:
        assert _same(o, _backward(c, t, o32, lse32, device)[1]), (c.name, "a second launch gave other bits")


def _chained_case(device, c, family):
    """Forward, then the backward on the forward's own o and lse (cross attention: on the forward's workspace with
    mask_bits_in_ws = 1, and once more with mask_bits_in_ws = 0 on a fresh one: the same bits)."""
    t = _tensors(c, device)
    code, f, ws = _forward(c, t, device)
    assert code == 0
    o32, lse32 = _as3(f["o"], c, c.L), _nan_padded(f["lse"].t, c.L)
    code, o = _backward(c, t, o32, lse32, device, ws=ws, bits_in_ws=1)
    assert code == 0
    refs = ac.ref_backward(t["q"], t["k"], t["v"], t["mask"], t["dO"], o32, lse32, c.H)
    _within(family, c, ac.backward_fractions(*_gradients(c, o), refs))
    if c.masked:
        code, o2 = _backward(c, t, o32, lse32, device)
        assert code == 0 and _same(o, o2), (c.name, "mask_bits_in_ws = 0 and 1 gave different bits")


@pytest.mark.parametrize("c", ac.CROSS_CASES, ids=_ids(ac.CROSS_CASES))
def test_cross_backward_standalone(device, c):
    _standalone_case(device, c, "cross backward stand-alone")


@pytest.mark.parametrize("c", ac.CROSS_CASES, ids=_ids(ac.CROSS_CASES))
def test_cross_backward_chained(device, c):
    _chained_case(device, c, "cross backward chained")


# ------------------------------------------------------------------------------------------------- self attention
@pytest.mark.parametrize("c", ac.SELF_CASES, ids=_ids(ac.SELF_CASES))
def test_self_forward(device, c):
    _forward_case(device, c, "self forward")
    if c.count_mode:
        _count_case(device, c)


@pytest.mark.parametrize("c", ac.SELF_CASES, ids=_ids(ac.SELF_CASES))
def test_self_backward_standalone(device, c):
    _standalone_case(device, c, "self backward")


@pytest.mark.parametrize("c", ac.SELF_CASES, ids=_ids(ac.SELF_CASES))
def test_self_backward_chained(device, c):
    _chained_case(device, c, "self backward")


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_nothing(device):
    for c in (next(c for c in ac.CROSS_CASES if (c.L, c.S) == (33, 33)), next(c for c in ac.SELF_CASES if c.L == 33)):
        t = _tensors(c, device)
        fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
        o32, lse32 = ac.saved_forward(fw, ac.lse_stride(c.L))
        refused = [dict(L=0), dict(L=257), dict(E=c.E + 16), dict(E=c.E - 16)] + ([dict(short=1)] if c.masked else [])
        for kw in refused:
            code, o, ws = _forward(c, t, device, **kw)
            assert code != 0 and _untouched(*o.values()), (c.name, kw, "forward")
            assert ws is None or bool((ws.interior() == ac.WS_BYTE).all()), (c.name, kw, "forward: workspace written")
            code, o = _backward(c, t, o32, lse32, device, **kw)
            assert code != 0 and _untouched(*o.values()), (c.name, kw, "backward")


# ------------------------------------------------------------------------------------------------- the dispatcher
@pytest.mark.parametrize("kind", ("cross", "self"))
def test_ops_attention_with_autograd_and_a_strided_q(device, kind):
    """ops.masked_cross_attention / ops.self_attention on q handed over as a non-contiguous view ([B, L, E] transposed):
    o, the saved lse and the three gradients with the comparators of the C entry points."""
    from unscene3d_amd import ops

    c = next(c for c in ac.CROSS_CASES if (c.L, c.S, c.B) == (150, 999, 2)) if kind == "cross" else \
        next(c for c in ac.SELF_CASES if (c.L, c.B, c.H) == (129, 2, 3))
    t = _tensors(c, device)
    qb = t["q"].transpose(0, 1).contiguous().requires_grad_()
    q = qb.transpose(0, 1)
    assert not q.is_contiguous()
    k, v = t["k"].clone().requires_grad_(), t["v"].clone().requires_grad_()
    y = ops.masked_cross_attention(q, k, v, t["mask"], c.H) if kind == "cross" else ops.self_attention(q, k, v, c.H)
    lse = y.grad_fn.saved_tensors[5 if kind == "cross" else 4]
    assert lse.shape == (c.B * c.H, ac.lse_stride(c.L))
    y.backward(t["dO"])
    torch.cuda.synchronize()
    fw = ac.ref_forward(t["q"], t["k"], t["v"], t["mask"], c.H)
    assert ac.dead_rows_exact(y.detach(), lse, fw)
    fr = ac.forward_fractions(y.detach(), lse, fw)
    refs = ac.ref_backward(t["q"], t["k"], t["v"], t["mask"], t["dO"], y.detach(), lse, c.H)
    fr.update(ac.backward_fractions(qb.grad.transpose(0, 1).contiguous(), k.grad, v.grad, refs))
    _within("ops." + ("masked_cross_attention" if kind == "cross" else "self_attention"), c, fr)


def test_print_the_bound_fractions_per_family():
    """A record, not a check: the largest fraction of its bound each quantity used, per family."""
    print("\nfamily / cases / largest |err| / bound per quantity")
    for fam, r in RATIOS.items():
        print(f"{fam:<36} {r['cases']:4d}  " + "  ".join(f"{k} {v:.3f}" for k, v in r.items() if k != "cases"))
