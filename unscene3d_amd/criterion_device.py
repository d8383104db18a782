"""The device set criterion (csrc/criterion.hip) on plain tensors: the only caller of lib.usc_criterion_*.
models/criterion.py::_FusedCriterion wraps these three functions for autograd, the entry-point tests call them directly.

    scene_forward   per scene: usc_criterion_target_bits, the cost matrices of all levels (_costs, 2 launches per 32
                    targets), their assignments (usc_lsap_batch: scipy's algorithm and tie-breaking), the label / mask /
                    dice sums (_losses, 1 launch).  With DropLoss one more launch counts the overlap of every matched
                    pair (_drop_counts) and _losses turns the counts into the 0 / 1 pair weights and applies them.
    table           per batch: usc_criterion_table, the [L, 4] loss table.
    scene_backward  per scene: usc_criterion_backward, 2 launches.

A scene has at most max_targets targets (32 unless the caller opts in, at most 128); the library refuses more.  Up to 32
targets a row's target membership is one 32-bit word, above that W = ceil(T / 32) words per row, word-major.
Queries and table columns: up to 256 (Q <= ld <= 256, any ld); above 128 the library's launches take a second group of
128 columns and the workspace is the larger one of usc_criterion_ws_bytes_q.  There is no bound on Q here: the library
refuses what it cannot take (SetCriterion admits more than 128 queries only with device_max_queries).

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


def scene_forward(tabs, tm, labels, logits, b, cost_weights, class_w, noobj, part, drop_thresh=None, alloc=None,
                  max_targets=32):
    """Matching and losses of scene b on all L levels.
    tabs: L mask-logit tables f32[S, ld] (ld >= Q; the columns Q <= col < ld are never read); tm: target masks u8[T, S];
    labels: i64[T]; logits: f32[L, B, Q, C]; cost_weights: (cost_mask, cost_class, cost_dice); class_w: f32[C];
    noobj: the no-object class; part: f32[L, 4], receives the scene's (ce numerator, ce denominator, mask, dice) sums.
    drop_thresh: the DropLoss IoU threshold, None = no DropLoss.  max_targets: the largest T taken (32 .. 128); above 32
    targets the bits are W words per row (module docstring)."""
    L, B, Q, NC = logits.shape
    S, ld = tabs[0].shape
    T = int(tm.shape[0])
    alloc = alloc or _empty_on(logits.device)
    st = _stream()
    if T > max_targets:
        raise ValueError(f"criterion_device: {T} targets, the caller allows {max_targets} (max_targets, at most 128)")
    bits = alloc(((T + 31) // 32, S) if T > 32 else (S,), _I32)
    cnt = alloc((T,), _I32)
    check(lib.usc_criterion_target_bits(tm.data_ptr(), T, max_targets, S, bits.data_ptr(), cnt.data_ptr(), st),
          "usc_criterion_target_bits")
    ptrs = _table_ptrs(tabs)
    cost = alloc((L, Q, T), _F32)
    cmask, cdice, nmat = alloc((3, L, Q, T), _F32).unbind(0)
    ssum = alloc((L, Q), _F32)
    logp = alloc((L, Q, NC), _F32)
    wsb = lib.usc_criterion_ws_bytes_q(L, S, T, Q)
    ws = alloc((wsb,), torch.uint8)
    lg = logits[:, b]                                                           # [L,Q,C] view: strides (B*Q*C, C, 1)
    w_mask, w_class, w_dice = cost_weights
    check(lib.usc_criterion_costs(ptrs, L, ld, S, Q, T, max_targets, bits.data_ptr(), cnt.data_ptr(), lg.data_ptr(),
                                  B * Q * NC, NC, NC, labels.data_ptr(), float(w_mask), float(w_class), float(w_dice),
                                  cost.data_ptr(), cmask.data_ptr(), cdice.data_ptr(), nmat.data_ptr(), ssum.data_ptr(),
                                  logp.data_ptr(), ws.data_ptr(), wsb, st), "usc_criterion_costs")
    src, tid, status = lsap_batch(cost)                                         # [L,T] queries (ascending), targets
    tcls = alloc((L, Q), _I32)
    counts = wts = None
    drop = (None, None, 0.0, None)
    if drop_thresh is not None:
        counts = alloc((2, L, T), _I32)
        wts = alloc((L, T), _F32)
        check(lib.usc_criterion_drop_counts(ptrs, L, ld, S, Q, T, max_targets, bits.data_ptr(), src.data_ptr(),
                                            tid.data_ptr(), counts.data_ptr(), st), "usc_criterion_drop_counts")
        drop = (counts.data_ptr(), cnt.data_ptr(), float(drop_thresh), wts.data_ptr())
    check(lib.usc_criterion_losses(cmask.data_ptr(), cdice.data_ptr(), logp.data_ptr(), src.data_ptr(), tid.data_ptr(),
                                   labels.data_ptr(), class_w.data_ptr(), L, Q, T, max_targets, NC, noobj,
                                   tcls.data_ptr(), part.data_ptr(), *drop, st), "usc_criterion_losses")
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
    as given to scene_forward (a smaller one that state.T exceeds is refused by the library, as any bad argument)."""
    L, B, Q, NC = dlogits.shape
    alloc = alloc or _empty_on(dlogits.device)
    dtab = alloc((L, state.S, state.ld), _F32)
    dptrs = (ctypes.c_void_p * L)(*[dtab[l].data_ptr() for l in range(L)])
    sc = state
    check(lib.usc_criterion_backward(
        _table_ptrs(tabs), dptrs, L, sc.ld, sc.S, Q, sc.T, max_targets, sc.bits.data_ptr(), sc.cnt.data_ptr(),
        sc.src.data_ptr(), sc.tid.data_ptr(), sc.nmat.data_ptr(), sc.ssum.data_ptr(), sc.logp.data_ptr(),
        sc.tcls.data_ptr(), class_w.data_ptr(), gtable.data_ptr(), den_tot.data_ptr(), NC, B * Q * NC, NC,
        dlogits[:, b].data_ptr(), sc.wts.data_ptr() if sc.wts is not None else None, _stream()), "usc_criterion_backward")
    return dtab
