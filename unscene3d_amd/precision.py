"""Precision of the backbone's convolutions: inference in f32 (default) or bf16, training in f32 (default) or split bf16.

Inference
---------

    with unscene3d_amd.inference_precision("bf16"):
        with torch.no_grad():
            out = model(x)

Under "bf16" every trunk convolution that runs WITHOUT autograd (torch.is_grad_enabled() False) and whose shape the
bf16 kernel covers (csrc/spconv_bf16.hip: cin a multiple of 16, cout a multiple of 32) rounds its input and its weights
to bf16 and accumulates in f32 on v_mfma_f32_32x32x16_bf16.  Batch norm, residual, ReLU, the decoder, attention, the
criterion and NCut stay f32.  With gradients enabled the f32 path runs whatever the setting: a training step never
sees bf16.  Other shapes (the 3-channel stem) keep the f32 kernels; a shape other than the stem that falls back is
reported once with a RuntimeWarning and recorded in FALLBACKS.

Weights are packed into the kernel's bf16 operand order once per entry into the outermost context (a nested entry
with the same precision shares the packs).  The cache is NOT keyed on Tensor._version: the fused optimizer
(optim.FlatAdamW) writes parameters in place through raw pointers, so the version counter never moves — enter the
context again after an optimizer step (InstanceSegmentation.eval_step does, once per call).

Training
--------

    with unscene3d_amd.training_precision("bf16x3"):
        loss = model(x).F.square().mean()
        loss.backward()

Under "bf16x2" / "bf16x3" a stride-1 trunk convolution with more than one offset that runs WITH autograd, and that the
policy below covers, computes its forward and its input gradient on the bf16 matrix cores at f32-grade accuracy
(csrc/spconv_bf16.hip): each f32 operand is split into 2 or 3 bf16 planes and the plane products (i, j) with
i + j < planes are summed in f32.  Three planes drop at most 2^-23 |x||w| per product (below f32's own rounding), two
planes 3 * 2^-16 |x||w|.  Weight gradients, batch norm, residual and ReLU stay on the f32 kernels.  Nothing is cached:
activations are split and weights packed inside every call, on its stream, so an optimizer that writes parameters in
place (even inside the backward pass) is always ordered against them.  The setting is read when the forward pass is
issued; the backward pass of a unit uses the planes its forward used.  The default "f32" changes nothing: not a launch,
not a bit.
"""
from __future__ import annotations

import warnings

import torch

PRECISIONS = ("f32", "bf16")
FALLBACKS = set()            # (K, cin, cout) of convolutions that ran in f32 under "bf16" (stem excluded)

# Where the bf16 kernel is used: the measured per-unit forward times on the 150 k-voxel bench scene (tools/infer_bench.py)
# favour it only for the wide stride-1 convolutions of the finest levels (96 -> 96 at 148 k rows: 470 -> 294 us; at
# 40 k rows 181 -> 140 us).  On the coarse levels (a few hundred to 10 k rows: too few workgroups without a K split),
# for narrow channels (32 -> 32 at 40 k rows: 65 -> 87 us) and for the stride-2 maps it is slower, so those keep f32.
MIN_ROWS = 32768
MIN_CIN = 96
STRIDED = False              # the stride-2 and transposed convs (covered by the kernel; measured slower)
# Training (split bf16): which stride-1, K > 1 units take the split kernel once a user has opted in (output rows and input
# channels at least these).  Measured (tools/train_precision_bench.py, profiles/train_precision.json):
# forward + input gradient of every stride-1 K = 27 unit shape of the bench scene is SLOWER than f32 in both split
# precisions (148 k rows, 96 -> 96: 891 us f32, 1 176 us bf16x2, 2 374 us bf16x3; worse on the coarse levels), so by
# default NOTHING is covered.  Tests force coverage (both at 0).
TRAIN_PRECISIONS = ("f32", "bf16x2", "bf16x3")
TRAIN_MIN_ROWS = 1 << 62
TRAIN_MIN_CIN = 96
_train = "f32"
_current = "f32"
_packs = None                # id(weight) -> (weight, data_ptr, packed bf16 tensor) of the open context


class inference_precision:
    """Context manager: the precision of trunk convolutions that run without autograd ("f32" or "bf16")."""

    def __init__(self, precision: str):
        if precision not in PRECISIONS:
            raise ValueError(f"inference_precision: unknown precision {precision!r} (expected one of {PRECISIONS})")
        self.precision = precision
        self._saved = None

    def __enter__(self):
        global _current, _packs
        self._saved = (_current, _packs)
        if not (self.precision == _current and _packs is not None):
            _packs = {}
        _current = self.precision
        return self

    def __exit__(self, *exc):
        global _current, _packs
        _current, _packs = self._saved
        self._saved = None
        return False


def current() -> str:
    return _current


def bf16_active() -> bool:
    """Do convolutions issued now run in bf16?  (bf16 selected and autograd off)"""
    return _current == "bf16" and not torch.is_grad_enabled()


def shape_ok(K: int, cin: int, cout: int) -> bool:
    from ._lib import lib
    return lib.usc_spconv_gather_gemm_bf16_ws_bytes(0, cin, cout, K) >= 0


def pack_weights(W3: torch.Tensor) -> torch.Tensor:
    """f32[K, cin, cout] -> the kernel's packed bf16 operand (usc_spconv_pack_w_bf16), a torch.bfloat16 tensor."""
    from . import ops
    from ._lib import check, lib
    K, cin, cout = W3.shape
    W3 = W3.detach().contiguous()
    out = torch.empty(K * cin * cout, dtype=torch.bfloat16, device=W3.device)
    check(lib.usc_spconv_pack_w_bf16(W3.data_ptr(), K, cin, cout, out.data_ptr(), ops._stream()),
          "usc_spconv_pack_w_bf16")
    return out


def unit_weights(W: torch.Tensor, stride1: bool = True, n_out: int = 1 << 62):
    """Packed bf16 weights of one conv (W: f32[K, cin, cout] or [cin, cout]) for the bf16 forward, or None: f32 path
    (bf16 not active, a unit where bf16 is measured slower — see MIN_ROWS — or a shape the kernel does not cover,
    reported once).  stride1 / n_out: whether it is a stride-1 conv, its output rows."""
    if not bf16_active():
        return None
    W3 = W if W.dim() == 3 else W[None]
    K, cin, cout = W3.shape
    if not (stride1 or STRIDED) or (stride1 and K == 1) or n_out < MIN_ROWS or cin < MIN_CIN:
        return None
    if not shape_ok(K, cin, cout):
        key = (int(K), int(cin), int(cout))
        if cin >= 16 and key not in FALLBACKS:
            FALLBACKS.add(key)
            warnings.warn(f"bf16 inference: a {cin} -> {cout} convolution with {K} offsets is not covered by the bf16 "
                          f"kernel; it runs in f32", RuntimeWarning, stacklevel=3)
        return None
    ent = _packs.get(id(W))
    if ent is None or ent[0] is not W or ent[1] != W.data_ptr():
        ent = _packs[id(W)] = (W, W.data_ptr(), pack_weights(W3))
    return ent[2]


class training_precision:
    """Context manager: the precision of trunk convolutions that run with autograd ("f32", "bf16x2" or "bf16x3")."""

    def __init__(self, precision: str):
        if precision not in TRAIN_PRECISIONS:
            raise ValueError(f"training_precision: unknown precision {precision!r} (expected one of {TRAIN_PRECISIONS})")
        self.precision = precision
        self._saved = None

    def __enter__(self):
        global _train
        self._saved = _train
        _train = self.precision
        return self

    def __exit__(self, *exc):
        global _train
        _train = self._saved
        self._saved = None
        return False


def current_training() -> str:
    return _train


def train_shape_ok(K: int, cin: int, cout: int, planes: int) -> bool:
    from ._lib import lib
    return lib.usc_spconv_gather_gemm_split_ws_bytes(0, cin, cout, K, planes) >= 0


def train_planes(W: torch.Tensor, stride1: bool = True, n_out: int = 1 << 62) -> int:
    """Planes (2 or 3) of the split precision one conv (W: f32[K, cin, cout] or [cin, cout]) runs in, or 0: the f32 path
    (default precision, autograd off, not a stride-1 K > 1 conv, a unit below TRAIN_MIN_ROWS / TRAIN_MIN_CIN, or a shape
    the kernel does not cover in the forward or in the input gradient — reported once unless it is the stem)."""
    if _train == "f32" or not torch.is_grad_enabled():
        return 0
    planes = 3 if _train == "bf16x3" else 2
    if not stride1 or W.dim() != 3 or W.shape[0] == 1:
        return 0
    K, cin, cout = W.shape
    if n_out < TRAIN_MIN_ROWS or cin < TRAIN_MIN_CIN:
        return 0
    # both directions: the input gradient is the same product with the operand widths swapped (cout -> cin)
    if not (train_shape_ok(K, cin, cout, planes) and train_shape_ok(K, cout, cin, planes)):
        key = (int(K), int(cin), int(cout))
        if cin >= 16 and key not in FALLBACKS:
            FALLBACKS.add(key)
            warnings.warn(f"{_train} training: a {cin} -> {cout} convolution with {K} offsets is not covered by the split "
                          f"bf16 kernel; it runs in f32", RuntimeWarning, stacklevel=3)
        return 0
    return planes
