"""The device set criterion (csrc/criterion.hip) on plain tensors: the only caller of lib.usc_criterion_*.
models/criterion.py::_FusedCriterion wraps these three functions for autograd, the entry-point tests call them directly.

    scene_forward   per scene: usc_criterion_target_bits, the cost matrices of all levels (_costs, 2 launches), their
                    assignments (usc_lsap_batch: scipy's algorithm and tie-breaking), the label / mask / dice sums
                    (_losses, 1 launch).  With DropLoss one more launch counts the overlap of every matched pair
                    (_drop_counts) and _losses_ex turns the counts into the 0 / 1 pair weights and applies them.
    table           per batch: usc_criterion_table, the [L, 4] loss table.
    scene_backward  per scene: usc_criterion_backward[_ex], 2 launches.

Up to 32 targets a row's target membership is one 32-bit word.  A scene with 32 < T <= max_targets (an opt-in of the
callers, at most 128) goes through the usc_criterion_*_wide twins of the same functions: W = ceil(T / 32) words per row,
word-major, and the cost pair once per word (2 W launches in place of 2).  A scene with T <= 32 calls exactly the
one-word functions, whatever max_targets is.

No device->host copy, no host solve, no synchronisation.  Inputs are contiguous HIP tensors of the stated dtypes; the
callers see to that, nothing is checked or converted here.  Every output and the
workspace come from `alloc(shape, dtype)`, by default torch.empty on the inputs' device; the tests pass an allocator that
poisons the memory, so that an element a kernel does not write shows."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from ._lib import check, lib
from .ops import _stream, lsap_batch

_F32, _I32 = torch.float32, torch.int32


class SceneState(NamedTuple):
    """What scene_forward leaves on the device for one scene (L levels, Q queries, T targets, S rows of ld columns)."""
    S: int
    ld: int
    T: int
    bits: torch.Tensor                  # i32[S]      target membership of a row, one bit per target; with more than 32
                                        #             targets i32[W,S], W = ceil(T / 32): word w = the targets 32w..32w+31
    cnt: torch.Tensor                   # i32[T]      rows per target
    cost: torch.Tensor                  # f32[L,Q,T]  the assignment costs
    cmask: torch.Tensor                 # f32[L,Q,T]  BCE cost = mask loss of the pair   (cmask | cdice | nmat are views
    cdice: torch.Tensor                 # f32[L,Q,T]  dice cost = dice loss of the pair    of one [3,L,Q,T] allocation)
    nmat: torch.Tensor                  # f32[L,Q,T]  dice numerators, for the backward
    ssum: torch.Tensor                  # f32[L,Q]    sigmoid sums, for the backward
    logp: torch.Tensor                  # f32[L,Q,C]  log-softmax of the class logits
    src: torch.Tensor                   # i64[L,T]    matched queries (ascending)
    tid: torch.Tensor                   # i64[L,T]    their targets
    status: torch.Tensor                # i32[L]      != 0: infeasible assignment problem
    tcls: torch.Tensor                  # i32[L,Q]    target class per query
    counts: Optional[torch.Tensor]      # i32[2,L,T]  I | F per matched pair; None without DropLoss
    wts: Optional[torch.Tensor]         # f32[L,T]    0 / 1 pair weights; None without DropLoss


def _empty_on(device):
    return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)


def _table_ptrs(tabs):
    return (ctypes.c_void_p * len(tabs))(*[t.data_ptr() for t in tabs])


def _entry_points(T, max_targets):
    """The C functions of a scene with T targets -> (target_bits, costs, drop_counts, losses_ex, backward_ex, suffix)."""
    if T <= 32:
        return (lib.usc_criterion_target_bits, lib.usc_criterion_costs, lib.usc_criterion_drop_counts,
                lib.usc_criterion_losses_ex, lib.usc_criterion_backward_ex, "")
    if T > max_targets:
        raise ValueError(f"criterion_device: {T} targets, the caller allows {max_targets} (max_targets, at most 128)")
    return (lib.usc_criterion_target_bits_wide, lib.usc_criterion_costs_wide, lib.usc_criterion_drop_counts_wide,
            lib.usc_criterion_losses_wide, lib.usc_criterion_backward_wide, "_wide")


def scene_forward(tabs, tm, labels, logits, b, cost_weights, class_w, noobj, part, drop_thresh=None, alloc=None,
                  max_targets=32):
    """Matching and losses of scene b on all L levels.
    tabs: L mask-logit tables f32[S, ld] (ld >= Q; the columns Q <= col < ld are never read); tm: target masks u8[T, S];
    labels: i64[T]; logits: f32[L, B, Q, C]; cost_weights: (cost_mask, cost_class, cost_dice); class_w: f32[C];
    noobj: the no-object class; part: f32[L, 4], receives the scene's (ce numerator, ce denominator, mask, dice) sums.
    drop_thresh: the DropLoss IoU threshold, None = no DropLoss.  max_targets: the largest T taken (32 .. 128); above 32
    targets the wide entry points run (module docstring)."""
    L, B, Q, NC = logits.shape
    S, ld = tabs[0].shape
    T = int(tm.shape[0])
    alloc = alloc or _empty_on(logits.device)
    st = _stream()
    wide = T > 32
    f_bits, f_costs, f_counts, f_losses, _, sfx = _entry_points(T, max_targets)
    bits = alloc(((T + 31) // 32, S) if wide else (S,), _I32)
    cnt = alloc((T,), _I32)
    check(f_bits(tm.data_ptr(), T, S, bits.data_ptr(), cnt.data_ptr(), st), "usc_criterion_target_bits" + sfx)
    ptrs = _table_ptrs(tabs)
    cost = alloc((L, Q, T), _F32)
    cmask, cdice, nmat = alloc((3, L, Q, T), _F32).unbind(0)
    ssum = alloc((L, Q), _F32)
    logp = alloc((L, Q, NC), _F32)
    wsb = lib.usc_criterion_ws_bytes(L, S, T)
    ws = alloc((wsb,), torch.uint8)
    lg = logits[:, b]                                                           # [L,Q,C] view: strides (B*Q*C, C, 1)
    w_mask, w_class, w_dice = cost_weights
    check(f_costs(ptrs, L, ld, S, Q, T, bits.data_ptr(), cnt.data_ptr(), lg.data_ptr(), B * Q * NC, NC, NC,
                  labels.data_ptr(), float(w_mask), float(w_class), float(w_dice), cost.data_ptr(), cmask.data_ptr(),
                  cdice.data_ptr(), nmat.data_ptr(), ssum.data_ptr(), logp.data_ptr(), ws.data_ptr(), wsb, st),
          "usc_criterion_costs" + sfx)
    src, tid, status = lsap_batch(cost)                                         # [L,T] queries (ascending), targets
    tcls = alloc((L, Q), _I32)
    counts = wts = None
    if drop_thresh is not None:
        counts = alloc((2, L, T), _I32)
        wts = alloc((L, T), _F32)
        check(f_counts(ptrs, L, ld, S, Q, T, bits.data_ptr(), src.data_ptr(), tid.data_ptr(), counts.data_ptr(), st),
              "usc_criterion_drop_counts" + sfx)
        check(f_losses(cmask.data_ptr(), cdice.data_ptr(), logp.data_ptr(), src.data_ptr(), tid.data_ptr(),
                       labels.data_ptr(), class_w.data_ptr(), L, Q, T, NC, noobj, tcls.data_ptr(), part.data_ptr(),
                       counts.data_ptr(), cnt.data_ptr(), float(drop_thresh), wts.data_ptr(), st),
              "usc_criterion_losses" + (sfx or "_ex"))
    elif wide:
        check(f_losses(cmask.data_ptr(), cdice.data_ptr(), logp.data_ptr(), src.data_ptr(), tid.data_ptr(),
                       labels.data_ptr(), class_w.data_ptr(), L, Q, T, NC, noobj, tcls.data_ptr(), part.data_ptr(),
                       None, None, 0.0, None, st), "usc_criterion_losses_wide")
    else:
        check(lib.usc_criterion_losses(cmask.data_ptr(), cdice.data_ptr(), logp.data_ptr(), src.data_ptr(), tid.data_ptr(),
                                       labels.data_ptr(), class_w.data_ptr(), L, Q, T, NC, noobj, tcls.data_ptr(),
                                       part.data_ptr(), st), "usc_criterion_losses")
    return SceneState(S, ld, T, bits, cnt, cost, cmask, cdice, nmat, ssum, logp, src, tid, status, tcls, counts, wts)


def table(parts, alloc=None):
    """parts f32[B, L, 4] of all scenes -> (the loss table f32[L, 4]: loss_ce, loss_mask, loss_dice, 0 per level,
    den_tot f32[L]: the batch's cross-entropy denominators, which the backward divides by)."""
    B, L, _ = parts.shape
    alloc = alloc or _empty_on(parts.device)
    out = alloc((L, 4), _F32)
    den_tot = alloc((L,), _F32)
    check(lib.usc_criterion_table(parts.data_ptr(), B, L, out.data_ptr(), den_tot.data_ptr(), _stream()),
          "usc_criterion_table")
    return out, den_tot


def scene_backward(state, tabs, b, class_w, gtable, den_tot, dlogits, alloc=None, max_targets=32):
    """Gradients of scene b: writes dlogits[:, b] (dlogits f32[L, B, Q, C]) and returns dtab f32[L, S, ld], the
    gradients of the L tables (zero in unmatched, dropped and padding columns).  gtable: f32[L * 4], the gradient of
    the flattened loss table; state: scene_forward's record of this scene, tabs: the tables it was given; max_targets:
    as given to scene_forward."""
    L, B, Q, NC = dlogits.shape
    alloc = alloc or _empty_on(dlogits.device)
    dtab = alloc((L, state.S, state.ld), _F32)
    dptrs = (ctypes.c_void_p * L)(*[dtab[l].data_ptr() for l in range(L)])
    sc = state
    args = (_table_ptrs(tabs), dptrs, L, sc.ld, sc.S, Q, sc.T, sc.bits.data_ptr(), sc.cnt.data_ptr(), sc.src.data_ptr(),
            sc.tid.data_ptr(), sc.nmat.data_ptr(), sc.ssum.data_ptr(), sc.logp.data_ptr(), sc.tcls.data_ptr(),
            class_w.data_ptr(), gtable.data_ptr(), den_tot.data_ptr(), NC, B * Q * NC, NC, dlogits[:, b].data_ptr())
    if sc.T > 32:
        f_bwd = _entry_points(sc.T, max_targets)[4]
        check(f_bwd(*args, sc.wts.data_ptr() if sc.wts is not None else None, _stream()), "usc_criterion_backward_wide")
    elif sc.wts is not None:
        check(lib.usc_criterion_backward_ex(*args, sc.wts.data_ptr(), _stream()), "usc_criterion_backward_ex")
    else:
        check(lib.usc_criterion_backward(*args, _stream()), "usc_criterion_backward")
    return dtab
