"""Tensor-level wrappers over the C ABI (include/usc3d.h) + autograd Functions.

PyTorch is used only as plumbing here: device memory (torch.empty), the current
HIP stream, and autograd bookkeeping.  All arithmetic happens inside
libusc3d_hip.so.  Inputs must be contiguous tensors on a HIP device; anything
else raises RuntimeError (reference: CHECK_CONTIGUOUS / CHECK_CUDA,
utils/cuda_utils/cuda_utils.cpp:4-6, third_party/pointnet2/_ext_src/src/sampling.cpp:68).
"""
from __future__ import annotations

from dataclasses import dataclass

import ctypes
import os
import weakref

import torch

from . import profiler as _prof
from ._lib import check, lib, require_device


def _stream():
    # raw handle of torch's current stream on the current device (torch.cuda.current_stream() builds a Stream
    # object through several Python layers: ~9 us per call, ~850 calls per training step)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _chk(t: torch.Tensor, dtype, name: str):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP (cuda) tensor — unscene3d_amd has no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ coordinates
def voxel_floor(xyz: torch.Tensor, voxel_size: float) -> torch.Tensor:
    """floor(xyz / voxel_size) in f64 -> i32[n,3] (reference datasets/utils.py:403)."""
    require_device()
    _chk(xyz, torch.float64, "xyz")
    out = torch.empty(xyz.shape, dtype=torch.int32, device=xyz.device)
    check(lib.usc_voxel_floor_f64(_ptr(xyz), xyz.shape[0], float(voxel_size), _ptr(out), _stream()),
          "usc_voxel_floor_f64")
    return out


@dataclass
class CoordMap:
    """One coordinate map: coordinates in row order + its HBM-resident hash table."""
    coords: torch.Tensor        # i32[n,4]  (b,x,y,z)
    table_keys: torch.Tensor    # i64[cap] (u64 bit pattern)
    table_vals: torch.Tensor    # i32[cap]
    tensor_stride: int

    @property
    def n(self) -> int:
        return self.coords.shape[0]

    @property
    def cap(self) -> int:
        return self.table_keys.shape[0]


def coordmap_build(coords: torch.Tensor, quant: int = 1, tensor_stride: int = 1):
    """-> (CoordMap of distinct coords, unique_idx i64[n_out], inverse i64[n]).

    First-occurrence unique == ME.utils.sparse_quantize(return_index, return_inverse)
    (reference datasets/utils.py:403-408)."""
    require_device()
    _chk(coords, torch.int32, "coords")
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise RuntimeError("coords must be int32 [n,4] (b,x,y,z)")
    n = coords.shape[0]
    dev = coords.device
    cap = lib.usc_coordmap_capacity(n)
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    vals = torch.empty(cap, dtype=torch.int32, device=dev)
    unique_idx = torch.empty(n, dtype=torch.int64, device=dev)
    inverse = torch.empty(n, dtype=torch.int64, device=dev)
    out_coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = lib.usc_coordmap_ws_bytes(n)
    ws = _ws(wsb, dev)
    check(lib.usc_coordmap_build(_ptr(coords), n, int(quant), _ptr(keys), _ptr(vals), cap, _ptr(unique_idx),
                                 _ptr(inverse), _ptr(out_coords), _ptr(n_out), _ptr(ws), ws.numel(), _stream()),
          "usc_coordmap_build")
    m = int(n_out.item())
    if m < 0:
        raise RuntimeError("usc_coordmap_build: coordinate outside the packable range (|c| < 2^17, batch < 1024)")
    cmap = CoordMap(out_coords[:m].contiguous() if m != n else out_coords, keys, vals, tensor_stride)
    return cmap, unique_idx[:m], inverse


def spatial_order(coords: torch.Tensor, shift: int = 3) -> torch.Tensor:
    """Row permutation (i64[n]) that makes the rows of every 2^shift-voxel cell contiguous, cells in z-order,
    batches kept in order; stable inside a cell.  An optional collate-side optimisation (see usc3d.h)."""
    require_device()
    _chk(coords, torch.int32, "coords")
    n = coords.shape[0]
    dev = coords.device
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    lo = coords[:, 1:].amin(0).tolist()
    hi = coords[:, 1:].amax(0).tolist()
    nb = int(coords[:, 0].max().item()) + 1
    extent = max(h - l for h, l in zip(hi, lo)) >> shift
    bits = max(1, int(extent).bit_length())
    if bits > 10:
        raise RuntimeError("spatial_order: scene extent too large for 10-bit cells; raise `shift`")
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    check(lib.usc_morton_cell_ids(_ptr(coords), n, shift, lo[0], lo[1], lo[2], bits, _ptr(ids), _stream()),
          "usc_morton_cell_ids")
    return segment_csr(ids, nb << (3 * bits)).order


def kernel_map_cube(cmap: CoordMap, ksize: int = 3) -> torch.Tensor:
    """Dense neighbour table i32[K, n] of a stride-1 HYPER_CUBE kernel on `cmap`."""
    K = ksize ** 3
    nbr = torch.empty((K, cmap.n), dtype=torch.int32, device=cmap.coords.device)
    check(lib.usc_kernel_map_cube(_ptr(cmap.coords), cmap.n, cmap.tensor_stride, ksize, _ptr(cmap.table_keys),
                                  _ptr(cmap.table_vals), cmap.cap, _ptr(nbr), _stream()), "usc_kernel_map_cube")
    return nbr


def kernel_map_down2(fine: CoordMap, parent: torch.Tensor, coarse: CoordMap):
    """Child table i32[8, n_coarse] and kidx u8[n_fine] of a k=2,s=2 kernel."""
    dev = fine.coords.device
    nbr2 = torch.full((8, coarse.n), -1, dtype=torch.int32, device=dev)
    kidx = torch.empty(fine.n, dtype=torch.uint8, device=dev)
    check(lib.usc_kernel_map_down2(_ptr(fine.coords), fine.n, fine.tensor_stride, _ptr(parent), _ptr(coarse.coords),
                                   coarse.n, _ptr(nbr2), _ptr(kidx), _stream()), "usc_kernel_map_down2")
    return nbr2, kidx


class Rulebook:
    """Per-offset (in,out) pair lists.  in_idx/out_idx are allocated at capacity K*n_out; only the first
    koff[K] entries are meaningful.  `P` (the pair count) is read back from the device lazily — the
    kernels take the device-side koff and an upper bound, so the hot path never synchronises on it."""

    def __init__(self, in_idx, out_idx, koff, capacity, P=None):
        self.in_idx, self.out_idx, self.koff, self.capacity = in_idx, out_idx, koff, capacity
        self._P = P

    @property
    def P(self) -> int:
        if self._P is None:
            self._P = int(self.koff[-1].item())
        return self._P


def rulebook_compact(nbr: torch.Tensor) -> Rulebook:
    _chk(nbr, torch.int32, "nbr")
    K, n_out = nbr.shape
    dev = nbr.device
    in_idx = torch.empty(K * n_out, dtype=torch.int32, device=dev)
    out_idx = torch.empty(K * n_out, dtype=torch.int32, device=dev)
    koff = torch.empty(K + 1, dtype=torch.int64, device=dev)
    ws = _ws(lib.usc_rulebook_ws_bytes(K, n_out), dev)
    check(lib.usc_rulebook_compact(_ptr(nbr), K, n_out, _ptr(in_idx), _ptr(out_idx), _ptr(koff), _ptr(ws),
                                   ws.numel(), _stream()), "usc_rulebook_compact")
    return Rulebook(in_idx, out_idx, koff, K * n_out)


# ------------------------------------------------------------------ convolution
def _conv_cost(P, n_in, n_out, K, cin, cout):
    """Algorithmic work of one sparse-conv launch: flops = 2*P*cin*cout,
    bytes = 4*(n_in*cin + n_out*cout + K*cin*cout) + 8*P."""
    return 2.0 * P * cin * cout, 4.0 * (n_in * cin + n_out * cout + K * cin * cout) + 8.0 * P


def _sorted_symbol(cout):
    """The mask-sorted kernel's template instance for this output width (plan_sorted, csrc/spconv_sorted.hip)."""
    cb = cout // 32
    nb = 4 if cb % 4 == 0 else 3 if cb % 3 == 0 else 2 if cb % 2 == 0 else 1
    return f"usc::gather_gemm_sorted_kernel<{nb}, {4 if nb == 4 else 8}>"


def _kernel_symbol(kind, n, cin, cout, K):
    """rocprof-style symbol of the kernel a launch will use (usc_spconv_plan)."""
    code = lib.usc_spconv_plan(kind, int(n), cin, cout, K)
    nb, aligned, compact = code & 0xFF, (code >> 8) & 1, (code >> 12) & 1
    tag = f" [n={int(n)} cin={cin} cout={cout} K={K} G={code >> 16}]" if _prof.SHAPES else ""
    if kind == 0 and (code >> 14) & 1:
        return "usc::stem_conv_kernel" + tag
    if kind == 0 and compact:
        return f"usc::gather_gemm_compact_kernel<{nb}>" + tag
    if kind == 2:
        if (code >> 13) & 1:
            return f"usc::wgrad_full_kernel<{code >> 16}, {nb}>" + tag
        return f"usc::wgrad_kernel<{nb}, {'true' if aligned else 'false'}>" + tag
    base = "usc::gather_gemm_aligned_kernel" if aligned else "usc::gather_gemm_kernel"
    return f"{base}<{nb}, {'true' if kind == 1 else 'false'}>" + tag


def weight_transpose(W: torch.Tensor, mirror: bool) -> torch.Tensor:
    _chk(W, torch.float32, "W")
    K, cin, cout = W.shape
    out = torch.empty((K, cout, cin), dtype=torch.float32, device=W.device)
    check(lib.usc_weight_transpose(_ptr(W), K, cin, cout, int(mirror), _ptr(out), _stream()), "usc_weight_transpose")
    return out


def rowsort(nbr: torch.Tensor):
    """(perm i32[n_out], tile_mask i32[ceil(n_out/32)]) of a neighbour table: output rows grouped by their
    neighbour bitmask (usc_rowsort_build).  Built once per table and kept on the tensor object, so every conv
    on the same kernel map — forward and, for stride-1 maps, dgrad — shares it."""
    cached = getattr(nbr, "_usc_rowsort", None)
    if cached is not None:
        return cached
    _chk(nbr, torch.int32, "nbr")
    K, n_out = nbr.shape
    dev = nbr.device
    perm = torch.empty(n_out, dtype=torch.int32, device=dev)
    tmask = torch.empty((n_out + 31) // 32, dtype=torch.int32, device=dev)
    ws = _ws(lib.usc_rowsort_ws_bytes(K, n_out), dev)
    check(lib.usc_rowsort_build(_ptr(nbr), K, n_out, _ptr(perm), _ptr(tmask), _ptr(ws), ws.numel(), _stream()),
          "usc_rowsort_build")
    nbr._usc_rowsort = (perm, tmask)
    return perm, tmask


# "sorted" (default): mask-sorted kernel for small/medium maps, tile-compacted kernel for large ones;
# "sorted-all" / "legacy": force one family (A/B comparisons, tests)
CONV_PATH = os.environ.get("USC3D_CONV", "sorted")


def _sorted_applies(nbr, K, cin, cout):
    """Mask-sorted kernel for every aligned table-form conv EXCEPT the shapes the tile-compacted kernel takes
    (>= 24 k rows, cin >= 64): measured on the bench scene, 96->96 channels — 148 k rows: compacted 0.51 ms vs
    sorted 0.67 ms; 40 k rows: 0.19 vs 0.28; 9.4 k rows 128->128: row-order 0.146 vs sorted 0.105; 2.2 k rows
    256->256: 0.131 vs 0.086."""
    if CONV_PATH == "legacy" or nbr is None or not (1 < K <= 32) or cin % 32 or cout % 32 or cin > 4096:
        return False
    if CONV_PATH == "sorted-all":
        return True
    compact = (lib.usc_spconv_plan(0, int(nbr.shape[1]), cin, cout, K) >> 12) & 1
    return not compact


def gather_gemm(feats, W, nbr, n_out, bias=None, out=None, accumulate=False, w_transposed=False):
    """out[o] = sum_k feats[nbr[k,o]] @ W[k] (+bias).  W f32[K,cin,cout]; nbr None -> identity.
    w_transposed: W is the FORWARD conv's [K, cout, cin] and W'[k][c][n] = W[K-1-k][n][c] is meant (input gradient
    of a stride-1 conv); the sorted and tile-compacted kernels fold that into their weight staging / packing, the
    row-order kernels get an explicit usc_weight_transpose pass."""
    _chk(feats, torch.float32, "feats")
    _chk(W, torch.float32, "W")
    if w_transposed:
        K, cout, cin = W.shape
        linear_form = nbr is None and K == 1 and cin % 32 == 0 and cout % 32 == 0     # folded into the row-order kernel
        if not (linear_form or _sorted_applies(nbr, K, cin, cout) or
                (nbr is not None and (lib.usc_spconv_plan(0, int(n_out), cin, cout, K) >> 12) & 1)):
            W = weight_transpose(W, mirror=K > 1)
            w_transposed = False
    K, cin, cout = (W.shape[0], W.shape[2], W.shape[1]) if w_transposed else W.shape
    if feats.shape[1] != cin:
        raise RuntimeError(f"gather_gemm: feats have {feats.shape[1]} channels, kernel expects {cin}")
    if nbr is not None:
        _chk(nbr, torch.int32, "nbr")
        if nbr.shape[0] != K or nbr.shape[1] != n_out:
            raise RuntimeError("gather_gemm: neighbour table shape mismatch")
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.float32, device=feats.device)
    if bias is not None:
        _chk(bias, torch.float32, "bias")
    if _sorted_applies(nbr, K, cin, cout):
        perm, tmask = rowsort(nbr)
        wsb = lib.usc_spconv_sorted_ws_bytes(n_out, cin, cout, K)
        ws = _ws(wsb, feats.device) if wsb > 0 else None
        # (named per template instance like every other kernel of the capture — the way rocprofv3 lists them: the merged
        #  family once overtook the tile-compacted kernel as "dominant" by 0.2 ms between two boxes)
        with _prof.maybe(lambda: _sorted_symbol(cout) + (f" [n={n_out} cin={cin} cout={cout} K={K}]" if _prof.SHAPES else ""),
                         lambda: _conv_cost(_prof.table_pairs(nbr), feats.shape[0], n_out, K, cin, cout)):
            check(lib.usc_spconv_sorted_gemm(_ptr(feats), feats.shape[0], cin, _ptr(W), K, cout, _ptr(nbr), _ptr(perm),
                                             _ptr(tmask), n_out, _ptr(bias), _ptr(out), int(accumulate),
                                             int(w_transposed), _ptr(ws), wsb, _stream()), "usc_spconv_sorted_gemm")
        return out
    wsb = lib.usc_spconv_gather_gemm_ws_bytes(n_out, cin, cout, K)
    ws = _ws(wsb, feats.device) if wsb > 0 else None
    with _prof.maybe(lambda: _kernel_symbol(0, n_out, cin, cout, K),
                     lambda: _conv_cost(_prof.table_pairs(nbr) if nbr is not None else n_out, feats.shape[0], n_out,
                                        K, cin, cout)):
        check(lib.usc_spconv_gather_gemm(_ptr(feats), feats.shape[0], cin, _ptr(W), K, cout, _ptr(nbr), n_out,
                                         _ptr(bias), _ptr(out), int(accumulate), int(w_transposed), _ptr(ws), wsb,
                                         _stream()), "usc_spconv_gather_gemm")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    """f32 -> bf16 copy, round to nearest even (usc_cast_bf16)."""
    _chk(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.usc_cast_bf16(_ptr(x), x.numel(), _ptr(out), _stream()), "usc_cast_bf16")
    return out


def _gather_gemm_planes(xs, planes, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate):
    """What gather_gemm_bf16 (planes None: xs bf16[n_in, cin]) and gather_gemm_split (xs bf16[n_in, planes, cin]) share:
    the table, output and bias checks and the call."""
    if planes is None:
        name, ws_bytes, gemm, split = "usc_spconv_gather_gemm_bf16", lib.usc_spconv_gather_gemm_bf16_ws_bytes, \
            lib.usc_spconv_gather_gemm_bf16, ()
    else:
        name, ws_bytes, gemm, split = "usc_spconv_gather_gemm_split", lib.usc_spconv_gather_gemm_split_ws_bytes, \
            lib.usc_spconv_gather_gemm_split, (planes,)
    if nbr is not None:
        _chk(nbr, torch.int32, "nbr")
        if nbr.shape[0] != K or nbr.shape[1] != n_out:
            raise RuntimeError(f"{name[11:]}: neighbour table shape mismatch")
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.float32, device=xs.device)
    if bias is not None:
        _chk(bias, torch.float32, "bias")
    wsb = ws_bytes(n_out, cin, cout, K, *split)
    ws = _ws(wsb, xs.device) if wsb > 0 else None
    check(gemm(_ptr(xs), xs.shape[0], cin, _ptr(Wp), K, cout, *split, _ptr(nbr), n_out, _ptr(bias), _ptr(out),
               int(accumulate), _ptr(ws), max(wsb, 0), _stream()), name)
    return out


def gather_gemm_bf16(feats, Wp, K, cout, nbr, n_out, bias=None, out=None, accumulate=False):
    """out[o] (+)= sum_k bf16(feats[nbr[k,o]]) @ bf16(W[k]) (+bias), f32 accumulate (csrc/spconv_bf16.hip).
    feats bf16[n_in, cin] (cast_bf16) or f32 (cast here); Wp: precision.pack_weights(W f32[K, cin, cout]);
    nbr i32[K, n_out] (-1 = no neighbour) or None (identity, K = 1).  Raises for shapes the kernel does not cover
    (precision.shape_ok)."""
    if feats.dtype == torch.float32:
        feats = cast_bf16(feats.contiguous())
    _chk(feats, torch.bfloat16, "feats")
    _chk(Wp, torch.bfloat16, "Wp")
    cin = feats.shape[1]
    if Wp.numel() != K * cin * cout:
        raise RuntimeError("gather_gemm_bf16: packed weights do not match K, cin, cout")
    return _gather_gemm_planes(feats, None, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate)


def split_bf16(x: torch.Tensor, planes: int) -> torch.Tensor:
    """f32[rows, c] -> bf16[rows, planes, c]: x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)
    (usc_split_bf16_rows); a 1-d f32[n] gives bf16[planes, n] (usc_split_bf16)."""
    _chk(x, torch.float32, "x")
    if x.dim() == 1:
        out = torch.empty((planes, x.shape[0]), dtype=torch.bfloat16, device=x.device)
        check(lib.usc_split_bf16(_ptr(x), x.numel(), planes, _ptr(out), _stream()), "usc_split_bf16")
        return out
    rows, c = x.shape
    out = torch.empty((rows, planes, c), dtype=torch.bfloat16, device=x.device)
    check(lib.usc_split_bf16_rows(_ptr(x), rows, c, planes, _ptr(out), _stream()), "usc_split_bf16_rows")
    return out


def pack_w_split(W: torch.Tensor, planes: int, transposed: bool = False) -> torch.Tensor:
    """f32[K, cin, cout] -> the split kernel's packed weight planes (usc_spconv_pack_w_split), bf16[planes, K*cin*cout];
    transposed: the mirrored transpose the input gradient needs (operand shape cout -> cin)."""
    _chk(W, torch.float32, "W")
    K, cin, cout = W.shape
    out = torch.empty((planes, K * cin * cout), dtype=torch.bfloat16, device=W.device)
    check(lib.usc_spconv_pack_w_split(_ptr(W), K, cin, cout, planes, int(transposed), _ptr(out), _stream()),
          "usc_spconv_pack_w_split")
    return out


def gather_gemm_split(xs, Wp, K, cout, nbr, n_out, bias=None, out=None, accumulate=False):
    """out[o] (+)= sum_k sum_{i+j<P} x_i[nbr[k,o]] @ W_j[k] (+bias), f32 accumulate (csrc/spconv_bf16.hip).
    xs bf16[n_in, P, cin] (split_bf16); Wp bf16[P, K*cin*cout] (pack_w_split); nbr i32[K, n_out] or None (identity)."""
    _chk(xs, torch.bfloat16, "xs")
    _chk(Wp, torch.bfloat16, "Wp")
    n_in, planes, cin = xs.shape
    if Wp.shape[0] != planes or Wp.shape[1] != K * cin * cout:
        raise RuntimeError("gather_gemm_split: packed weights do not match P, K, cin, cout")
    return _gather_gemm_planes(xs, planes, cin, Wp, K, cout, nbr, n_out, bias, out, accumulate)


def pairs_gemm(feats, W, rows_in, rows_out, koff, P, n_out):
    """out[rows_out[p]] = feats[rows_in[p]] @ W[k(p)] — every out row written exactly once."""
    _chk(feats, torch.float32, "feats")
    _chk(W, torch.float32, "W")
    K, cin, cout = W.shape
    if feats.shape[1] != cin:
        raise RuntimeError("pairs_gemm: channel mismatch")
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feats.device)
    with _prof.maybe(lambda: _kernel_symbol(1, int(P), cin, cout, K),
                     lambda: _conv_cost(int(P), feats.shape[0], n_out, K, cin, cout)):
        check(lib.usc_spconv_pairs_gemm(_ptr(feats), cin, _ptr(W), K, cout, _ptr(rows_in), _ptr(rows_out),
                                        _ptr(koff), int(P), _ptr(out), _stream()), "usc_spconv_pairs_gemm")
    return out


# Parameter gradients straight into `p.grad`: when a leaf parameter already has a gradient buffer (the trainer
# keeps them allocated: zero_grad(set_to_none=False), one flat buffer for the all-reduce), the backward kernels add
# into it and the Function returns None, instead of returning a fresh tensor that autograd's AccumulateGrad then
# adds with one more small kernel per parameter (~250 launches per step for the backbone).  See _grad_target.


# streams other than the compute stream that backward kernels of this package write parameter gradients on (the decoder's
# key-preparation stream, models/mask3d.py): whoever reads p.grad outside autograd's own stream bookkeeping — a gradient
# reducer starting a collective in the middle of backward — lets the current stream wait for them first
SIDE_STREAMS = []


def on_side_stream():
    if not SIDE_STREAMS:
        return False
    raw = _stream()
    return any(st.cuda_stream == raw for st in SIDE_STREAMS)


def join_side_streams():
    cur = torch.cuda.current_stream()
    for st in SIDE_STREAMS:
        if st.device == cur.device:
            cur.wait_stream(st)


GRAD_WRITTEN_HOOK = None   # callable(param), set by ddp.BucketedGradReducer: "the kernels that add into p.grad are queued"


def _grad_target(param):
    """p.grad when the backward kernels may add into it directly, else None (the gradient is then returned to
    autograd).  Never when somebody else listens for the gradient through autograd: tensor hooks, or
    post-accumulate hooks (torch DDP, FSDP, user hooks) unless they belong to this package's own reducer, which is
    told about in-place writes through GRAD_WRITTEN_HOOK."""
    if isinstance(param, torch.nn.Parameter) and param.is_leaf and param.grad is not None \
            and param.grad.is_contiguous() and not param._backward_hooks \
            and (GRAD_WRITTEN_HOOK is not None or not getattr(param, "_post_accumulate_grad_hooks", None)):
        return param.grad
    return None


def _graph_task():
    """Id of the running backward pass (-1 outside one)."""
    return torch._C._current_graph_task_id()


_END_MARKS = weakref.WeakKeyDictionary()    # key object -> graph task in which at_end_of_backward queued the key's callback


def at_end_of_backward(key, fn, outside):
    """Run `fn` when the running backward pass ends: queued with the engine once per (key, pass), `key` being the object
    the work belongs to.  Outside a pass (a direct call of a backward function) "run" calls `fn` now, "skip" does nothing.
    The engine drops its callbacks when a backward node raises, so the marks are keyed on the graph task: a mark of
    another pass is stale and is replaced (a sticky one kept every later pass from queueing,
    test_joins_are_queued_again_after_a_failed_backward); held weakly, it goes with a short-lived key (a GradSink)."""
    if outside not in ("run", "skip"):
        raise ValueError("at_end_of_backward: outside is 'run' or 'skip'")
    task = _graph_task()
    if task < 0:
        if outside == "run":
            fn()
        return
    if _END_MARKS.get(key) == task:
        return
    _END_MARKS[key] = task

    def done():
        if _END_MARKS.get(key) == task:
            del _END_MARKS[key]
        fn()
    torch.autograd.Variable._execution_engine.queue_callback(done)


def queued_at_end_of_backward(key):
    """Is the callback of `key` queued in the RUNNING pass?  If not, state that a caller keeps for the callback
    (units._WgradQueue) was left by a pass that never finished."""
    return 0 <= _graph_task() == _END_MARKS.get(key)


def _join_after_backward():
    """Called by backward kernels that may be running on one of SIDE_STREAMS.  The engine makes the caller's stream wait
    for the streams of the AccumulateGrad nodes it ran, not for a stream on which a backward wrote p.grad in place: one
    end-of-backward callback lets the caller's stream wait for the side streams, so that `loss.backward();
    optimizer.step()` stays correct without the caller knowing about them."""
    if SIDE_STREAMS and on_side_stream():
        at_end_of_backward(join_side_streams, join_side_streams, outside="skip")


PARAMS_FINAL_HOOK = None  # callable(list of params), set by optim.FlatAdamW.enable_early: "every kernel that adds into the
                          # gradients of THESE parameters this step has been queued (compute stream and lane) — nothing
                          # else will" — only callers that know it by construction report (program.backward: a trunk
                          # unit's parameters are written once per backward pass)


def _params_final(params):
    if PARAMS_FINAL_HOOK is not None and params:
        PARAMS_FINAL_HOOK(params)


def _grad_written(*params):
    _join_after_backward()
    if GRAD_WRITTEN_HOOK is not None:
        for p in params:
            if p is not None:
                GRAD_WRITTEN_HOOK(p)


def _param_grads(params, zeros=False):
    """The parameter-gradient rule of one backward node, for its parameters in order (None: the node has no such
    parameter) -> (buffers, accumulate, finish).  In place only if EVERY parameter has a target (_grad_target): the
    buffers are then the p.grad tensors and the kernels add into them (accumulate); otherwise fresh buffers that the
    kernels write and autograd gets whole — zeros=True for a node that writes only some rows of a packed parameter.
    finish(), after the node's last launch: -> what the node returns for the parameters (None where written in place,
    which is also reported: _grad_written)."""
    live = [p for p in params if p is not None]
    bufs = [_grad_target(p) for p in live]
    in_place = all(t is not None for t in bufs)
    if not in_place:
        new = torch.zeros_like if zeros else torch.empty_like
        bufs = [new(p, memory_format=torch.contiguous_format) for p in live]
    it = iter(bufs)
    bufs = [None if p is None else next(it) for p in params]

    def finish():
        if not in_place:
            return tuple(bufs)
        _grad_written(*params)
        return (None,) * len(params)
    return bufs, in_place, finish


def wgrad(a, b, K, a_idx=None, b_idx=None, koff=None, into=None, out=None, nbr=None):
    """dW[k] = sum_{p in list k} a[a_idx[p]]^T b[b_idx[p]] -> f32[K,cin,cout]; ADDED into `into`, or WRITTEN to `out`
    (a contiguous buffer of K*cin*cout floats), when given.
    nbr (optional): the forward conv's neighbour table i32[K, n_out] of a stride-1 conv whose pair lists these are;
    the stem (<= 4 input channels, 32 output channels) then takes the table form (usc_spconv_wgrad_table)."""
    _chk(a, torch.float32, "a")
    _chk(b, torch.float32, "b")
    cin, cout = a.shape[1], b.shape[1]
    dW = into if into is not None else (out if out is not None else
                                        torch.empty((K, cin, cout), dtype=torch.float32, device=a.device))
    if nbr is not None and cin <= 4 and cout == 32 and K <= 32 and nbr.shape == (K, b.shape[0]):
        wsb = lib.usc_spconv_wgrad_table_ws_bytes(K, cin, cout)
        ws = _ws(wsb, a.device)
        with _prof.maybe(lambda: "usc::stem_wgrad_kernel" + (f" [n={b.shape[0]} cin={cin} cout={cout} K={K}]" if _prof.SHAPES else ""),
                         lambda: _conv_cost(_prof.table_pairs(nbr), a.shape[0], b.shape[0], K, cin, cout)):
            check(lib.usc_spconv_wgrad_table(_ptr(a), cin, _ptr(b), cout, _ptr(nbr), K, b.shape[0], _ptr(dW),
                                             int(into is not None), _ptr(ws), ws.numel(), _stream()),
                  "usc_spconv_wgrad_table")
        return dW
    ws = _ws(lib.usc_spconv_wgrad_ws_bytes(K, cin, cout), a.device)
    n_rows = a.shape[0] if a_idx is None else int(a_idx.shape[0])
    # (profiling only) real pair count = koff[K]; n_rows is the capacity of the pair lists
    with _prof.maybe(lambda: _kernel_symbol(2, n_rows, cin, cout, K),
                     lambda: _conv_cost(n_rows if koff is None else int(koff[-1].item()), a.shape[0], b.shape[0], K,
                                        cin, cout)):
        check(lib.usc_spconv_wgrad(_ptr(a), cin, _ptr(b), cout, K, _ptr(a_idx), _ptr(b_idx), _ptr(koff), n_rows,
                                   _ptr(dW), int(into is not None), _ptr(ws), ws.numel(), _stream()), "usc_spconv_wgrad")
    return dW


def wgrad_group(a_list, b_list, into_list, K, a_idx, b_idx, koff):
    """R same-shape weight gradients on one kernel map in ONE launch (usc_spconv_wgrad_group):
    into_list[r][k] += sum_p a_list[r][a_idx[p]]^T b_list[r][b_idx[p]].  The buffers of `into_list` are added into."""
    import ctypes as C
    R = len(a_list)
    if not (R == len(b_list) == len(into_list) and 1 <= R <= lib.usc_spconv_wgrad_group_max()):
        raise RuntimeError("wgrad_group: between 1 and usc_spconv_wgrad_group_max() problems, three lists of equal length")
    cin, cout = a_list[0].shape[1], b_list[0].shape[1]
    for a, b, w in zip(a_list, b_list, into_list):
        _chk(a, torch.float32, "a")
        _chk(b, torch.float32, "b")
        _chk(w, torch.float32, "dW")
        if a.shape[1] != cin or b.shape[1] != cout or w.numel() != K * cin * cout:
            raise RuntimeError("wgrad_group: the problems of a group have one shape")
    n_rows = a_list[0].shape[0] if a_idx is None else int(a_idx.shape[0])
    pa = (C.c_void_p * R)(*[t.data_ptr() for t in a_list])
    pb = (C.c_void_p * R)(*[t.data_ptr() for t in b_list])
    pw = (C.c_void_p * R)(*[t.data_ptr() for t in into_list])
    check(lib.usc_spconv_wgrad_group(R, pa, pb, pw, cin, cout, K, _ptr(a_idx), _ptr(b_idx), _ptr(koff), n_rows, 1,
                                     _stream()), "usc_spconv_wgrad_group")
    return into_list


class _ConvSame(torch.autograd.Function):
    """k^3 stride-1 conv on one map (in map == out map) or 1x1 conv (nbr None)."""

    @staticmethod
    def forward(ctx, feats, W, bias, nbr, get_rulebook):
        feats = feats.contiguous()
        W3 = W if W.dim() == 3 else W[None]
        out = gather_gemm(feats, W3.contiguous(), nbr, feats.shape[0], bias=None if bias is None else bias.reshape(-1))
        ctx.save_for_backward(feats, W3)
        ctx.nbr, ctx.get_rulebook = nbr, get_rulebook
        ctx.has_bias = bias is not None
        ctx.w_param = W
        return out

    @staticmethod
    def backward(ctx, dout):
        feats, W3 = ctx.saved_tensors
        dfeats, dW, dbias = conv_same_backward(feats, W3, ctx.w_param, dout.contiguous(), ctx.nbr, ctx.get_rulebook,
                                               *ctx.needs_input_grad[:2], ctx.has_bias and ctx.needs_input_grad[2])
        return dfeats, dW, None if dbias is None else dbias.reshape(1, -1), None, None


def _wgrad_param(W_param, a, b, K, a_idx=None, b_idx=None, koff=None, nbr=None):
    """wgrad under the parameter-gradient rule (_param_grads) -> what the node returns for the weight."""
    (dW,), in_place, finish = _param_grads((W_param,))
    wgrad(a, b, K, a_idx, b_idx, koff, into=dW if in_place else None, out=None if in_place else dW, nbr=nbr)
    return finish()[0]


def conv_same_backward(feats, W3, W_param, dout, nbr, get_rulebook, need_dfeats=True, need_dW=True, need_dbias=False):
    """The body of _ConvSame.backward (models/mask3d.py's early-stage gate issues the mask head's on the lane): input
    gradient, weight gradient (None when added into W_param.grad), bias column sum f32[cout]; None where not needed."""
    K = W3.shape[0]
    dfeats = dW = None
    if need_dfeats:
        if K > 1:
            dfeats = gather_gemm(dout, W3.contiguous(), nbr, feats.shape[0], w_transposed=True)
        else:
            dfeats = gather_gemm(dout, weight_transpose(W3.contiguous(), mirror=False), nbr, feats.shape[0])
    if need_dW:
        if nbr is None:
            dW = _wgrad_param(W_param, feats, dout, 1)
        else:
            rb = get_rulebook()
            dW = _wgrad_param(W_param, feats, dout, K, rb.in_idx, rb.out_idx, rb.koff, nbr=nbr)
    return dfeats, dW, colsum(dout) if need_dbias else None


class _ConvDown2(torch.autograd.Function):
    """k=2, s=2 conv: fine map -> coarse map via the child table nbr2[8, n_coarse]."""

    @staticmethod
    def forward(ctx, feats, W, nbr2, get_rulebook):
        feats = feats.contiguous()
        out = gather_gemm(feats, W.contiguous(), nbr2, nbr2.shape[1])
        ctx.save_for_backward(feats, W)
        ctx.nbr2, ctx.get_rulebook = nbr2, get_rulebook
        ctx.w_param = W
        return out

    @staticmethod
    def backward(ctx, dout):
        feats, W = ctx.saved_tensors
        dout = dout.contiguous()
        rb = ctx.get_rulebook()  # in_idx = fine row, out_idx = coarse row
        dfeats = dW = None
        if ctx.needs_input_grad[0]:
            Wt = weight_transpose(W.contiguous(), mirror=False)
            dfeats = pairs_gemm(dout, Wt, rb.out_idx, rb.in_idx, rb.koff, feats.shape[0], feats.shape[0])
        if ctx.needs_input_grad[1]:
            dW = _wgrad_param(ctx.w_param, feats, dout, W.shape[0], rb.in_idx, rb.out_idx, rb.koff)
        return dfeats, dW, None, None


class _ConvTrUp2(torch.autograd.Function):
    """k=2, s=2 transposed conv: coarse map -> cached fine map (same child table)."""

    @staticmethod
    def forward(ctx, feats, W, nbr2, get_rulebook, n_fine):
        feats = feats.contiguous()
        rb = get_rulebook()
        out = pairs_gemm(feats, W.contiguous(), rb.out_idx, rb.in_idx, rb.koff, n_fine, n_fine)
        ctx.save_for_backward(feats, W)
        ctx.nbr2, ctx.rb = nbr2, rb
        ctx.w_param = W
        return out

    @staticmethod
    def backward(ctx, dout):
        feats, W = ctx.saved_tensors
        dout = dout.contiguous()
        rb = ctx.rb
        dfeats = dW = None
        if ctx.needs_input_grad[0]:
            Wt = weight_transpose(W.contiguous(), mirror=False)
            dfeats = gather_gemm(dout, Wt, ctx.nbr2, feats.shape[0])
        if ctx.needs_input_grad[1]:
            dW = _wgrad_param(ctx.w_param, feats, dout, W.shape[0], rb.out_idx, rb.in_idx, rb.koff)
        return dfeats, dW, None, None, None


def conv_same(feats, W, bias, nbr, get_rulebook):
    return _ConvSame.apply(feats, W, bias, nbr, get_rulebook)


def conv_down2(feats, W, nbr2, get_rulebook):
    return _ConvDown2.apply(feats, W, nbr2, get_rulebook)


def conv_tr_up2(feats, W, nbr2, get_rulebook, n_fine):
    return _ConvTrUp2.apply(feats, W, nbr2, get_rulebook, n_fine)


# ------------------------------------------------------------------ batch norm / relu
def colstats(x, y=None):
    """-> (sum_i x[i,c], sum_i x[i,c]*y[i,c]) as f64[c] (y None -> x*x)."""
    _chk(x, torch.float32, "x")
    n, c = x.shape
    s1 = torch.empty(c, dtype=torch.float64, device=x.device)
    s2 = torch.empty(c, dtype=torch.float64, device=x.device)
    ws = _ws(lib.usc_colstats_ws_bytes(n, c), x.device)
    check(lib.usc_colstats(_ptr(x), _ptr(y), n, c, _ptr(s1), _ptr(s2), _ptr(ws), ws.numel(), _stream()),
          "usc_colstats")
    return s1, s2


def colsum(x):
    return colstats(x)[0].to(torch.float32)


def bn_apply(x, scale, shift, residual=None, relu=False):
    _chk(x, torch.float32, "x")
    n, c = x.shape
    y = torch.empty_like(x)
    check(lib.usc_bn_apply(_ptr(x), _ptr(scale), _ptr(shift), _ptr(residual), int(relu), _ptr(y), n, c, _stream()),
          "usc_bn_apply")
    return y


class _BatchNormAct(torch.autograd.Function):
    """y = [relu](BN_train(x) [+ residual]) — MinkowskiBatchNorm (+MinkowskiReLU) (+`out += residual`)
    fused into one stats pass and one apply pass (reference models/modules/resnet_block.py:48-64)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, relu, eps, running_mean, running_var, momentum, training,
                num_batches_tracked=None):
        x = x.contiguous()
        n, c = x.shape
        dev = x.device
        if training:
            stats = torch.empty((4, c), dtype=torch.float32, device=dev)   # mean | invstd | scale | shift
            mean, invstd, scale, shift = stats[0], stats[1], stats[2], stats[3]
            ws = _ws(lib.usc_colstats_ws_bytes(n, c), dev)
            check(lib.usc_bn_forward_stats(_ptr(x), n, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                           _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                                           _ptr(mean), _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(ws), ws.numel(),
                                           _stream()),
                  "usc_bn_forward_stats")
        else:
            mean = running_mean
            invstd = torch.rsqrt(running_var + eps)
            scale = (gamma * invstd).contiguous()
            shift = (beta - mean * scale).contiguous()
        res = None if residual is None else residual.contiguous()
        y = bn_apply(x, scale, shift, res, relu)
        ctx.save_for_backward(x, gamma, mean, invstd, y if relu else None)
        ctx.relu, ctx.has_res, ctx.training = relu, residual is not None, training
        ctx.gamma_param, ctx.beta_param = gamma, beta
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd, y = ctx.saved_tensors
        dy = dy.contiguous()
        n, c = x.shape
        dev = x.device
        red = torch.empty((2, c), dtype=torch.float32, device=dev)   # mean_g | mean_gx
        ws = _ws(lib.usc_colstats_ws_bytes(n, c), dev)
        (dg, db), in_place, finish = _param_grads((ctx.gamma_param, ctx.beta_param))
        check(lib.usc_bn_backward_reduce(_ptr(x), _ptr(dy), _ptr(y), _ptr(mean), _ptr(invstd), n, c,
                                         int(ctx.training), int(in_place), _ptr(dg), _ptr(db), _ptr(red[0]), _ptr(red[1]),
                                         _ptr(ws), ws.numel(), _stream()), "usc_bn_backward_reduce")
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        check(lib.usc_bn_backward_dx(_ptr(x), _ptr(dy), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(red[0]),
                                     _ptr(red[1]), _ptr(dx), _ptr(dres), n, c, _stream()), "usc_bn_backward_dx")
        return (dx, *finish(), dres, None, None, None, None, None, None, None)


def batch_norm_act(x, gamma, beta, residual=None, relu=False, eps=1e-5, running_mean=None, running_var=None,
                   momentum=0.1, training=True, num_batches_tracked=None):
    """`num_batches_tracked` (i64[1], optional) is incremented inside the statistics launch of a training pass."""
    return _BatchNormAct.apply(x, gamma, beta, residual, relu, eps, running_mean, running_var, momentum, training,
                               num_batches_tracked)


class _ReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.usc_relu_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), "usc_relu_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib.usc_relu_bwd(_ptr(y), _ptr(dy), _ptr(dx), y.numel(), _stream()), "usc_relu_bwd")
        return dx


def relu(x):
    _chk(x, torch.float32, "x")
    return _ReLU.apply(x)


# ------------------------------------------------------------------ pooling / gather / segments
def avgpool_down2(feats, nbr2, row_of=None, threshold=False):
    """MinkowskiAvgPooling(kernel_size=2, stride=2) forward: mean over present children.
    row_of (i64[n_fine]): the fine rows are feats[row_of[i]] (feats may be a column slice of a wider table); a child
    table that already holds the ROWS OF `feats` to read (row_of folded into nbr2 once per batch) needs no row_of;
    threshold: return sigmoid(mean) < 0.5 as bool instead of the means."""
    if feats.dtype != torch.float32 or not feats.is_cuda or feats.dim() != 2 or feats.stride(1) != 1:
        raise RuntimeError("avgpool_down2: feats must be an f32 HIP matrix with unit column stride")
    # (a column slice of a wider table is fine either way: rows are addressed through the leading dimension)
    if row_of is not None:
        _chk(row_of, torch.int64, "row_of")
    nc, c = nbr2.shape[1], feats.shape[1]
    ld = feats.stride(0) if feats.shape[0] > 1 else c
    out = torch.empty((nc, c), dtype=torch.bool if threshold else torch.float32, device=feats.device)
    check(lib.usc_avgpool_down2_ex(_ptr(feats), c, ld, _ptr(row_of), _ptr(nbr2), nc,
                                   None if threshold else _ptr(out), _ptr(out) if threshold else None, _stream()),
          "usc_avgpool_down2_ex")
    return out


MAXPOOL_I32_ID_LIMIT = 1 << 24   # the reference pools the ids as f32: above 2^24 its result is not an id any more


def maxpool_down2_i32(ids, nbr2):
    """MinkowskiMaxPooling(kernel_size=2, stride=2) forward on one integer column (segment ids, reference
    pseudo_masks/freemask_main.py:189-199): max over the present children of the `avgpool_down2` child table.
    ids: integer [n_fine] or [n_fine, 1] on the device -> i32 of the same rank.  Ids < 0 or >= 2^24 are refused."""
    if not ids.is_cuda or ids.dtype not in (torch.int32, torch.int64) or ids.dim() not in (1, 2) \
            or (ids.dim() == 2 and ids.shape[1] != 1):
        raise RuntimeError("maxpool_down2_i32: ids must be an i32 / i64 HIP column [n] or [n, 1]")
    _chk(nbr2, torch.int32, "nbr2")
    if nbr2.dim() != 2 or nbr2.shape[0] != 8:
        raise RuntimeError("maxpool_down2_i32: nbr2 must be the i32 [8, n_coarse] child table")
    flat = ids.reshape(-1)
    if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= MAXPOOL_I32_ID_LIMIT):
        raise RuntimeError(f"maxpool_down2_i32: ids outside [0, 2^24): {int(flat.min())} .. {int(flat.max())}")
    flat = flat.to(torch.int32).contiguous()
    nc = nbr2.shape[1]
    out = torch.empty(nc, dtype=torch.int32, device=ids.device)
    check(lib.usc_maxpool_down2_i32(_ptr(flat), flat.numel(), _ptr(nbr2), nc, _ptr(out), _stream()),
          "usc_maxpool_down2_i32")
    return out if ids.dim() == 1 else out.view(-1, 1)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, idx, out=None, unique=False):
        src = src.contiguous()
        idx = idx.contiguous()
        if out is None:
            out = torch.empty((idx.shape[0], src.shape[1]), dtype=torch.float32, device=src.device)
        elif tuple(out.shape) != (idx.shape[0], src.shape[1]) or out.dtype != torch.float32 or not out.is_contiguous() \
                or out.requires_grad:
            raise RuntimeError("gather_rows: `out` must be a contiguous f32 [len(idx), C] tensor that does not require grad")
        check(lib.usc_gather_rows(_ptr(src), src.shape[1], _ptr(idx), idx.shape[0], _ptr(out), _stream()),
              "usc_gather_rows")
        ctx.save_for_backward(idx)
        ctx.n_src, ctx.unique = src.shape[0], bool(unique)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dout = dout.contiguous()
        dsrc = torch.zeros((ctx.n_src, dout.shape[1]), dtype=torch.float32, device=dout.device)
        fn = lib.usc_scatter_rows_unique if ctx.unique else lib.usc_scatter_add_rows
        check(fn(_ptr(dout), dout.shape[1], _ptr(idx), idx.shape[0], _ptr(dsrc), _stream()), "usc_scatter_add_rows")
        return dsrc, None, None, None


def gather_rows(src, idx, out=None, unique=False):
    """out[j] = src[idx[j]]; `out` (optional): the caller's buffer (e.g. a HIP-graph input) instead of a new tensor.
    unique: the caller guarantees that idx holds no duplicates (a permutation / torch.randperm(n)[:k]); the backward
    pass then scatters with plain stores instead of float atomics."""
    _chk(src, torch.float32, "src")
    _chk(idx, torch.int64, "idx")
    return _GatherRows.apply(src, idx, out, unique)


class GradSink:
    """One gradient buffer for SEVERAL consumers of the same table (the three decoders' key samples of a backbone
    level): every consumer's backward accumulates its rows into `buf` (zero-filled by the first one to arrive) and hands
    autograd None; the last one hands over the buffer.  Replaces one zero fill + scatter per consumer and autograd's
    adds of the dense results (same per-row summation order: arrival order).  A consumer whose backward never runs would
    leave the others' gradients stranded: checked when the backward pass ends."""

    def __init__(self):
        self.buf, self.pending = None, 0

    def _check(self):
        if self.pending != 0 and self.buf is not None:
            self.buf = None
            raise RuntimeError("GradSink: a consumer's backward did not run; the gradients accumulated for its table were "
                               "not delivered (call the consumers without a shared sink)")


class _SampleKeys(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, mask, pos, idx, n_scenes, K, n_valid, outs, unique, sink=None, valid_unique=False):
        # feats None: the mask rows only; mask None: the feature (+ positional) rows only (usc_sample_keys' partial calls)
        c = 0 if feats is None else feats.shape[1]
        q = 0 if mask is None else mask.shape[1]
        p = 0 if pos is None else pos.shape[1]
        dev = idx.device
        if outs is None:
            of = None if feats is None else torch.empty((n_scenes, K, c), dtype=torch.float32, device=dev)
            om = None if mask is None else torch.empty((n_scenes, K, q), dtype=torch.bool, device=dev)
            op = None if pos is None else torch.empty((n_scenes, K, p), dtype=torch.float32, device=dev)
        else:
            # fresh tensor objects over the caller's storage: the objects returned from here get autograd metadata
            of, om, op = (None if o is None else o.detach() for o in outs)
            for name, t, want, dt in (("features", of, (n_scenes, K, c), torch.float32), ("mask", om, (n_scenes, K, q), torch.bool),
                                      ("positions", op, (n_scenes, K, p), torch.float32)):
                if (t is None) != (want[2] == 0):
                    raise RuntimeError(f"sample_keys: an output buffer for the {name} is {'missing' if t is None else 'not wanted'}")
                if t is not None and (tuple(t.shape) != want or t.dtype != dt or not t.is_contiguous()):
                    raise RuntimeError(f"sample_keys: the {name} buffer {tuple(t.shape)} {t.dtype} (strides {t.stride()}) "
                                       f"does not fit {want} contiguous {dt}")
        nv = (ctypes.c_int32 * n_scenes)(*[int(v) for v in n_valid])
        wsb = lib.usc_sample_keys_ws_bytes(n_scenes, K, q) if q else 0
        ws = _ws(wsb, dev) if q else None
        check(lib.usc_sample_keys(_ptr(feats), c, _ptr(mask), q, _ptr(pos), p, _ptr(idx), n_scenes, K, nv, _ptr(of),
                                  _ptr(om), _ptr(op), _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "usc_sample_keys")
        ctx.save_for_backward(idx)
        # the mask and positional outputs never carry a gradient: without this the engine hands backward() zero-filled
        # [B, K, Q] / [B, K, p] tensors for them (two stock fills per decoder pass, up to 26 us for the bool one)
        ctx.set_materialize_grads(False)
        ctx.n_src, ctx.unique = (0 if feats is None else feats.shape[0]), bool(unique)
        ctx.valid_unique = bool(valid_unique)
        ctx.K, ctx.n_valid = int(K), [min(int(v), int(K)) for v in n_valid]
        ctx.sink = sink if (sink is not None and ctx.needs_input_grad[0]) else None     # (forward runs under no_grad)
        if ctx.sink is not None:
            ctx.sink.pending += 1
        outs_ = tuple(t for t in (of, om, op) if t is not None)
        for t in (om, op):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return outs_ if len(outs_) > 1 else outs_[0]

    @staticmethod
    def backward(ctx, dfeats, *_):
        (idx,) = ctx.saved_tensors
        sink = ctx.sink
        if dfeats is None:                     # nothing downstream used the sampled features
            if sink is not None:
                sink.pending -= 1
                if sink.pending == 0 and sink.buf is not None:
                    dsrc, sink.buf = sink.buf, None
                    return (dsrc,) + (None,) * 10
            return (None,) * 11
        dfeats = dfeats.contiguous().view(idx.shape[0], -1)
        c = dfeats.shape[1]

        def scatter(dst, add):
            # unique: all K keys of every scene are distinct rows.  valid_unique (the decoder's plans, models/mask3d.py
            # _draw_key_samples): the first n_valid[b] keys of a scene are distinct — a random subset, or every row of the
            # scene — and the rest is padding that repeats row 0 and is masked for every query, so its gradient rows are
            # exact zeros: only the distinct prefix is scattered, with plain (or read-modify-write) row stores.
            # (Scattering the padding with float atomics serialised on row 0: 214 us per pass on a 20 k-voxel scene.)
            # Neither: duplicates anywhere — float atomics over all keys.
            if not (ctx.unique or ctx.valid_unique):
                check(lib.usc_scatter_add_rows(_ptr(dfeats), c, _ptr(idx), idx.shape[0], _ptr(dst), _stream()),
                      "usc_scatter_add_rows")
                return
            fn = lib.usc_scatter_rows_unique_add if add else lib.usc_scatter_rows_unique
            if ctx.unique or all(v == ctx.K for v in ctx.n_valid):
                check(fn(_ptr(dfeats), c, _ptr(idx), idx.shape[0], _ptr(dst), _stream()), "usc_scatter_rows")
                return
            for b, nv in enumerate(ctx.n_valid):
                if nv > 0:
                    check(fn(dfeats.data_ptr() + 4 * b * ctx.K * c, c, idx.data_ptr() + 8 * b * ctx.K, nv, _ptr(dst),
                             _stream()), "usc_scatter_rows")

        if sink is not None:
            first = sink.buf is None
            if first:
                sink.buf = torch.zeros((ctx.n_src, c), dtype=torch.float32, device=dfeats.device)
                at_end_of_backward(sink, sink._check, outside="skip")
            scatter(sink.buf, add=not first)
            sink.pending -= 1
            if sink.pending > 0:
                return (None,) * 11
            dsrc, sink.buf = sink.buf, None
            return (dsrc,) + (None,) * 10
        dsrc = torch.zeros((ctx.n_src, c), dtype=torch.float32, device=dfeats.device)
        scatter(dsrc, add=False)
        return (dsrc,) + (None,) * 10


def sample_keys(feats, mask, pos, idx, n_scenes, K, n_valid, outs=None, unique=False, sink=None, valid_unique=False):
    """The cross-attention keys of one decoder pass (reference models/mask3d.py:306-346) in two launches:
    rows `idx` (i64[n_scenes*K], batch-wide row numbers) of the level's features f32[n,c], thresholded attention
    masks bool[n,Q] and positional encodings f32[n,p] (or None) -> ([B,K,c], bool[B,K,Q], [B,K,p]) — feats None: the
    masks only (-> bool[B,K,Q], Q <= 256); mask None: the features (and positions) only, in one launch; a query column
    masked in all K rows of its scene is cleared; rows k >= n_valid[b] (padding) are fully masked.
    outs: the caller's three buffers (e.g. the inputs of a captured pass).  Gradient: features only (scatter;
    `unique` as in gather_rows; valid_unique: only the first n_valid[b] keys of every scene are distinct and the padding
    behind them carries no gradient).  sink: a GradSink shared by every call that samples the SAME `feats` in this forward
    pass — their gradients are then accumulated into one buffer."""
    if feats is None and mask is None:
        raise RuntimeError("sample_keys: nothing to gather")
    rows = None
    for t, dt, name in ((feats, torch.float32, "feats"), (mask, torch.bool, "mask"), (pos, torch.float32, "pos")):
        if t is not None:
            _chk(t, dt, name)
            if rows is not None and t.shape[0] != rows:
                raise RuntimeError("sample_keys: feats, mask and pos must have the same rows")
            rows = t.shape[0]
    _chk(idx, torch.int64, "idx")
    if idx.shape[0] != n_scenes * K or len(n_valid) != n_scenes:
        raise RuntimeError("sample_keys: inconsistent sizes")
    if mask is not None and mask.shape[1] > ATTN_MAX_QUERIES:
        raise RuntimeError(f"sample_keys: the mask rows take <= {ATTN_MAX_QUERIES} queries")
    return _SampleKeys.apply(feats, mask, pos, idx, int(n_scenes), int(K), list(n_valid), outs, unique, sink,
                             valid_unique)


ATTN_MASK_ROWS_MAX_QUERIES = 128
ATTN_MASK_ROWS_MAX_STEPS = 4


def attn_mask_rows_applies(logits, tables, n_scenes) -> bool:
    """Whether attn_mask_rows takes these logits and child tables (else: the avgpool_down2 chain and sample_keys)."""
    q = logits.shape[1]
    ld = logits.stride(0) if logits.shape[0] > 1 else q
    return (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
            and q % 4 == 0 and 4 <= q <= ATTN_MASK_ROWS_MAX_QUERIES and ld % 4 == 0 and logits.data_ptr() % 16 == 0
            and 1 <= len(tables) <= ATTN_MASK_ROWS_MAX_STEPS and 1 <= n_scenes <= 16)


def attn_mask_rows(logits, tables, idx, n_scenes, K, n_valid, outs=None, fix=True):
    """The thresholded attention-mask rows of the sampled keys of one decoder pass, bool[B, K, Q], in one launch (and
    sample_keys' all-masked-column launch): the bytes of avgpool_down2 over `tables` in turn (the last step with
    threshold=True) followed by sample_keys(None, mask, None, idx, ...), computed for the rows `idx` only.
    logits: f32[segments, Q] (may be a column slice), Q a multiple of 4 up to 128; tables: 1 to 4 child tables
    i32[8, n_j], the first one holding rows of `logits`; idx: i64[n_scenes*K] rows of the last table's level.
    outs: the caller's bool[B, K, Q] buffer (an input of a captured pass).  fix=False leaves the all-masked-column rule
    out (tests)."""
    if not attn_mask_rows_applies(logits, tables, n_scenes):
        raise RuntimeError("attn_mask_rows: f32 HIP logits with 4..128 queries (a multiple of 4), a leading dimension "
                           "that is a multiple of 4, 1..4 child tables and <= 16 scenes")
    _chk(idx, torch.int64, "idx")
    q, d, dev = logits.shape[1], len(tables), logits.device
    for t in tables:
        _chk(t, torch.int32, "child table")
        if t.dim() != 2 or t.shape[0] != 8 or t.shape[1] < 1:
            raise RuntimeError("attn_mask_rows: a child table must be i32 [8, n]")
    if idx.shape[0] != n_scenes * K or len(n_valid) != n_scenes:
        raise RuntimeError("attn_mask_rows: inconsistent sizes")
    if outs is None:
        out = torch.empty((n_scenes, K, q), dtype=torch.bool, device=dev)
    else:
        out = outs.detach()
        if tuple(out.shape) != (n_scenes, K, q) or out.dtype != torch.bool or not out.is_contiguous():
            raise RuntimeError(f"attn_mask_rows: the mask buffer {tuple(out.shape)} {out.dtype} does not fit "
                               f"{(n_scenes, K, q)} contiguous bool")
    ld = logits.stride(0) if logits.shape[0] > 1 else q
    tabs = (ctypes.c_void_p * d)(*[t.data_ptr() for t in tables])
    rows = (ctypes.c_int64 * d)(*[t.shape[1] for t in tables])
    nv = (ctypes.c_int32 * n_scenes)(*[int(v) for v in n_valid])
    ws = _ws(lib.usc_attn_mask_rows_ws_bytes(n_scenes, K, q, d), dev)
    check(lib.usc_attn_mask_rows(_ptr(logits), ld, q, d, tabs, rows, _ptr(idx), n_scenes, K, nv, _ptr(out), _ptr(ws),
                                 ws.numel(), 0 if fix else 1, _stream()), "usc_attn_mask_rows")
    return out


def gather_rows_i32(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Row gather of an int32 table (coordinates) through the same kernel (bit pattern copy)."""
    _chk(src, torch.int32, "src")
    return _GatherRows.apply(src.view(torch.float32), idx.contiguous(), None, False).view(torch.int32)


@dataclass
class SegmentCSR:
    seg: torch.Tensor      # i64[n]
    order: torch.Tensor    # i64[n] rows sorted by segment (stable)
    seg_off: torch.Tensor  # i64[S+1]
    S: int


def segment_csr(seg: torch.Tensor, S: int) -> SegmentCSR:
    _chk(seg, torch.int64, "seg")
    n = seg.shape[0]
    dev = seg.device
    order = torch.empty(n, dtype=torch.int64, device=dev)
    seg_off = torch.empty(S + 1, dtype=torch.int64, device=dev)
    ws = _ws(lib.usc_segment_csr_ws_bytes(n, S), dev)
    check(lib.usc_segment_csr(_ptr(seg), n, S, _ptr(order), _ptr(seg_off), _ptr(ws), ws.numel(), _stream()),
          "usc_segment_csr")
    return SegmentCSR(seg, order, seg_off, S)


def segment_sum_from_csr(src, csr: SegmentCSR):
    mean = torch.empty((csr.S, src.shape[1]), dtype=torch.float32, device=src.device)
    check(lib.usc_segment_mean_fwd(_ptr(src), src.shape[1], _ptr(csr.order), _ptr(csr.seg_off), csr.S, _ptr(mean),
                                   _stream()), "usc_segment_mean_fwd")
    cnt = (csr.seg_off[1:] - csr.seg_off[:-1]).to(torch.float32)
    return mean * cnt[:, None]


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, csr):
        src = src.contiguous()
        out = torch.empty((csr.S, src.shape[1]), dtype=torch.float32, device=src.device)
        check(lib.usc_segment_mean_fwd(_ptr(src), src.shape[1], _ptr(csr.order), _ptr(csr.seg_off), csr.S, _ptr(out),
                                       _stream()), "usc_segment_mean_fwd")
        ctx.csr, ctx.n = csr, src.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        csr = ctx.csr
        dsrc = torch.empty((ctx.n, dout.shape[1]), dtype=torch.float32, device=dout.device)
        check(lib.usc_segment_mean_bwd(_ptr(dout), dout.shape[1], _ptr(csr.seg), _ptr(csr.seg_off), ctx.n,
                                       _ptr(dsrc), _stream()), "usc_segment_mean_bwd")
        return dsrc, None


def segment_mean(src, csr: SegmentCSR):
    """torch_scatter.scatter_mean(src, seg, dim=0) with a prebuilt CSR (reference models/mask3d.py:223)."""
    _chk(src, torch.float32, "src")
    return _SegmentMean.apply(src, csr)


# ------------------------------------------------------------------ points
def furthest_point_sample(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    """pointnet2_utils.furthest_point_sample(xyz f32[B,N,3], npoint) -> i32[B,npoint]
    (reference third_party/pointnet2/pointnet2_utils.py:50-79)."""
    require_device()
    _chk(xyz, torch.float32, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise RuntimeError("xyz must be f32 [B,N,3]")
    B, N, _ = xyz.shape
    tmp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
    idx = torch.zeros((B, npoint), dtype=torch.int32, device=xyz.device)
    check(lib.usc_furthest_point_sampling(_ptr(xyz), B, N, npoint, _ptr(tmp), _ptr(idx), _stream()),
          "usc_furthest_point_sampling")
    return idx


def fourier_posenc(xyz, lo, hi, gauss_B, d):
    """PositionEmbeddingCoordsSine('fourier', normalize=True): f32[n,3] -> f32[n,d]."""
    _chk(xyz, torch.float32, "xyz")
    out = torch.empty((xyz.shape[0], d), dtype=torch.float32, device=xyz.device)
    check(lib.usc_fourier_posenc(_ptr(xyz), xyz.shape[0], _ptr(lo.contiguous()), _ptr(hi.contiguous()),
                                 _ptr(gauss_B.contiguous()), d, _ptr(out), _stream()), "usc_fourier_posenc")
    return out


# ------------------------------------------------------------------ neighbours / clustering
def knn1(query: torch.Tensor, ref: torch.Tensor):
    """Exact nearest reference point of every query (scipy KDTree.query(k=1)): -> (dist f32[nq], idx i64[nq])."""
    require_device()
    _chk(query, torch.float32, "query")
    _chk(ref, torch.float32, "ref")
    nq = query.shape[0]
    idx = torch.empty(nq, dtype=torch.int64, device=query.device)
    d2 = torch.empty(nq, dtype=torch.float32, device=query.device)
    check(lib.usc_knn1(_ptr(query), nq, _ptr(ref), ref.shape[0], _ptr(idx), _ptr(d2), _stream()), "usc_knn1")
    return d2.sqrt(), idx


KNN1_GRID_CELL_BUDGET = 1 << 22          # cells of a knn1_grid grid: 16 MiB of cell offsets at the most


def knn1_grid_plan(lo, hi, nr: int, cell=None):
    """Host arithmetic of `knn1_grid`: the grid over the box lo..hi (3 floats each) for nr reference points.
    -> (origin f64[3], cell, dims i32[3]).

    cell=None: sqrt(2 * (ex*ey + ey*ez + ez*ex) / nr) for a box of extents ex, ey, ez.  The clouds of this package are
    surfaces (mesh vertices, surface voxels), and a surface of area A meets about A / cell^2 cells, so nr * cell^2 / A
    points share an occupied cell; half the box's surface stands in for A, which is not known without a pass over the
    points, and the 2 asks for two points per occupied cell.  A box with no area (points on a line, one point) takes its
    longest extent / nr, or 1.  profiles/knn1_grid.txt has the occupancy this gives on the package's own shapes.
    A cell that would need more than KNN1_GRID_CELL_BUDGET cells is doubled until the grid fits."""
    import numpy as np
    lo = np.asarray(lo, np.float64).reshape(3)
    ext = np.maximum(np.asarray(hi, np.float64).reshape(3) - lo, 0.0)
    if not (np.isfinite(lo).all() and np.isfinite(ext).all()):
        raise RuntimeError("knn1_grid: the reference bounds are not finite")
    if cell is None:
        area = ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]
        cell = float(np.sqrt(2.0 * area / nr)) if area > 0 else float(ext.max() / nr)
        if not cell > 0:
            cell = 1.0
    cell = float(cell)
    if not (cell > 0 and np.isfinite(cell)):
        raise RuntimeError(f"knn1_grid: cell must be a positive finite number, got {cell!r}")
    while True:
        dims = np.floor(ext / cell) + 1.0
        if dims.prod() <= KNN1_GRID_CELL_BUDGET:
            return lo, cell, dims.astype(np.int32)
        cell *= 2.0


def knn1_grid(query: torch.Tensor, ref: torch.Tensor, cell=None, bounds=None):
    """`knn1` through a uniform grid (usc_knn1_grid): the same (dist f32[nq], idx i64[nq]), bit for bit, in time
    proportional to nq + nr instead of nq * nr when the points are spread over many cells.

    cell: side of a grid cell; None picks one from the bounds and nr (`knn1_grid_plan`).  Too small a cell is enlarged
    until the grid has at most KNN1_GRID_CELL_BUDGET cells; a cell larger than the cloud gives one cell, which works.
    bounds: (lo, hi) of the reference points, 3 numbers each (anything np.asarray takes).  None reads them back from the
    device — one `aminmax` and one host synchronisation per call; a caller that knows the box passes it.  Bounds that
    miss points cost speed, never correctness: points outside are binned into the boundary cells."""
    require_device()
    _chk(query, torch.float32, "query")
    _chk(ref, torch.float32, "ref")
    nq, nr = query.shape[0], ref.shape[0]
    if nr < 1:
        raise RuntimeError("knn1_grid: needs at least one reference point")
    if bounds is None:
        lo, hi = torch.aminmax(ref, dim=0)
        lo, hi = torch.stack([lo, hi]).cpu().numpy()
    else:
        lo, hi = bounds
    origin, cell, dims = knn1_grid_plan(lo, hi, nr, cell)
    nbytes = lib.usc_knn1_grid_ws_bytes(nr, dims.ctypes.data)
    if nbytes < 0:
        check(-1, "usc_knn1_grid_ws_bytes")
    ws = _ws(nbytes, ref.device)
    idx = torch.empty(nq, dtype=torch.int64, device=query.device)
    d2 = torch.empty(nq, dtype=torch.float32, device=query.device)
    check(lib.usc_knn1_grid(_ptr(query), nq, _ptr(ref), nr, origin.ctypes.data, cell, dims.ctypes.data, _ptr(idx),
                            _ptr(d2), _ptr(ws), ws.numel(), _stream()), "usc_knn1_grid")
    return d2.sqrt(), idx


def knn_hybrid(query: torch.Tensor, ref: torch.Tensor, k: int, radius: float, cell=None, bounds=None):
    """The k nearest reference points strictly inside `radius` of every query (usc_knn_hybrid_grid; open3d's
    KDTreeSearchParamHybrid(radius, max_nn=k)) -> (idx i32[nq,k], count i32[nq]).

    Candidates have d2 < r2 with d2 in f64 on the f32 inputs and r2 = float64(float32(radius)) ** 2; they are ordered
    by (d2, index); row i holds its first count[i] = min(k, candidates) indices, then -1.  1 <= k <= 64.
    cell: None means the radius (a query then reads at most 27 cells), doubled until the grid has at most
    KNN1_GRID_CELL_BUDGET cells.  cell and bounds are as in `knn1_grid`: they change the time, never the answer."""
    require_device()
    _chk(query, torch.float32, "query")
    _chk(ref, torch.float32, "ref")
    nq, nr = query.shape[0], ref.shape[0]
    if nr < 1:
        raise RuntimeError("knn_hybrid: needs at least one reference point")
    k, radius = int(k), float(radius)
    if not 1 <= k <= 64:                                      # the library refuses it too; idx needs a valid shape
        raise RuntimeError(f"knn_hybrid: k must be 1 .. 64, got {k}")
    if bounds is None:
        lo, hi = torch.aminmax(ref, dim=0)
        lo, hi = torch.stack([lo, hi]).cpu().numpy()
    else:
        lo, hi = bounds
    origin, cell, dims = knn1_grid_plan(lo, hi, nr, radius if cell is None else cell)
    nbytes = lib.usc_knn_hybrid_grid_ws_bytes(nr, dims.ctypes.data)
    if nbytes < 0:
        check(-1, "usc_knn_hybrid_grid_ws_bytes")
    ws = _ws(nbytes, ref.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=query.device)
    count = torch.empty(nq, dtype=torch.int32, device=query.device)
    check(lib.usc_knn_hybrid_grid(_ptr(query), nq, _ptr(ref), nr, radius, k, origin.ctypes.data, cell, dims.ctypes.data,
                                  _ptr(idx), _ptr(count), _ptr(ws), ws.numel(), _stream()), "usc_knn_hybrid_grid")
    return idx, count


def normals_pca(query: torch.Tensor, ref: torch.Tensor, idx: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """Normal of every query from its neighbour list (usc_normals_pca): the unit eigenvector of the smallest eigenvalue
    of the neighbours' covariance, f32[nq,3]; (0, 0, 1) with fewer than 3 neighbours or a degenerate covariance; the
    component of largest magnitude is >= 0."""
    require_device()
    _chk(query, torch.float32, "query")
    _chk(ref, torch.float32, "ref")
    _chk(idx, torch.int32, "idx")
    _chk(count, torch.int32, "count")
    nq = query.shape[0]
    if idx.dim() != 2 or idx.shape[0] != nq or count.shape != (nq,):
        raise RuntimeError("normals_pca: idx must be [nq,k] and count [nq]")
    out = torch.empty((nq, 3), dtype=torch.float32, device=query.device)
    check(lib.usc_normals_pca(_ptr(query), nq, _ptr(ref), ref.shape[0], _ptr(idx), _ptr(count), idx.shape[1], _ptr(out),
                              _stream()), "usc_normals_pca")
    return out


def estimate_normals(points: torch.Tensor, radius: float = 0.1, max_nn: int = 30) -> torch.Tensor:
    """open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) of a cloud f32[N,3] -> f32[N,3]:
    `knn_hybrid` of the cloud against itself, then `normals_pca`.  The sign is this package's (see `normals_pca`)."""
    idx, count = knn_hybrid(points, points, max_nn, radius)
    return normals_pca(points, points, idx, count)


def mask_gt_overlap(masks: torch.Tensor, slot: torch.Tensor, nslots: int) -> torch.Tensor:
    """Point overlap of every mask column with every GT slot (the ScanNet instance evaluator's intersections):
    masks bool/u8 [N,K] (rows may be strided: stride(0) >= K, stride(1) == 1), slot i32 [N] in [0, nslots)
    -> i32 [K+1, nslots]: row j < K = #points of column j in each slot, row K = #points in each slot."""
    require_device()
    if not isinstance(masks, torch.Tensor) or masks.dim() != 2 or not masks.is_cuda:
        raise RuntimeError("masks must be a 2-D HIP (cuda) tensor")
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    if masks.dtype != torch.uint8:
        raise RuntimeError(f"masks must be bool or uint8, got {masks.dtype}")
    n, k = masks.shape
    if n > 0 and (masks.stride(1) != 1 or masks.stride(0) < k):
        masks = masks.contiguous()
    ld = masks.stride(0) if n > 0 else k
    _chk(slot, torch.int32, "slot")
    if slot.shape != (n,):
        raise RuntimeError(f"slot must be [{n}], got {list(slot.shape)}")
    counts = torch.empty((k + 1, int(nslots)), dtype=torch.int32, device=masks.device)
    check(lib.usc_mask_gt_overlap(_ptr(masks), n, k, ld, _ptr(slot), int(nslots), _ptr(counts), _stream()),
          "usc_mask_gt_overlap")
    return counts


def instance_targets(labels: torch.Tensor, num_segments=None, filter_out_classes=(), label_offset: int = 0, alloc=None):
    """Instance targets of one label table (csrc/targets.hip; reference datasets/utils.py:529-613): labels i64 [N, ld],
    column 0 the semantic label, column 1 the instance id, and — when `num_segments` is given — column 2 a segment id
    in [0, num_segments).  -> (labels i64 [T], masks bool [T, N], segment_mask bool [T, num_segments] or None): one
    target per instance id other than -1 whose label (column 0 of its first row) is not in `filter_out_classes`, in
    ascending id order; labels = max(label - label_offset, 0).  The distinct ids come from torch.unique; the
    decisions are made on the device and T is the one value read back (for the allocation).
    alloc(shape, dtype, zero) -> device tensor: where the outputs and the work arrays come from (tests pass one that
    surrounds every array with guard bytes)."""
    require_device()
    _chk(labels, torch.int64, "labels")
    if labels.dim() != 2 or labels.shape[1] < (2 if num_segments is None else 3):
        raise RuntimeError("labels must be [N, >= 2] (with segments: [N, >= 3])")
    dev = labels.device
    if alloc is None:
        def alloc(shape, dtype, zero):
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
    n, ld = labels.shape
    ids = torch.unique(labels[:, 1]).contiguous()
    u = int(ids.shape[0])
    rank, count, first = alloc((n,), torch.int32, False), alloc((u,), torch.int32, False), alloc((u,), torch.int32, False)
    slot, lab, kept = alloc((u,), torch.int32, False), alloc((u,), torch.int64, False), alloc((1,), torch.int32, False)
    flt = torch.tensor([int(c) for c in filter_out_classes], dtype=torch.int64, device=dev)
    st = _stream()
    check(lib.usc_instance_index(_ptr(labels), n, ld, _ptr(ids), u, _ptr(rank), _ptr(count), _ptr(first), st),
          "usc_instance_index")
    check(lib.usc_instance_select(_ptr(labels), n, ld, _ptr(ids), u, _ptr(count), _ptr(first), _ptr(flt),
                                  int(flt.shape[0]), int(label_offset), _ptr(slot), _ptr(lab), _ptr(kept), st),
          "usc_instance_select")
    t = int(kept.item())                                     # the one read-back of a table
    masks = alloc((t, n), torch.uint8, False)
    seg_mask = None if num_segments is None else alloc((t, int(num_segments)), torch.uint8, True)
    check(lib.usc_instance_masks(_ptr(rank), n, _ptr(slot), u, t, _ptr(masks), _ptr(labels[:, 2:]) if seg_mask is not None
                                 else None, ld, 0 if seg_mask is None else int(num_segments), _ptr(seg_mask), st),
          "usc_instance_masks")
    return lab[:t], masks.view(torch.bool), None if seg_mask is None else seg_mask.view(torch.bool)


VIT_ATTN_PRECISIONS = {"f32": 0, "bf16": 1}


def vit_attention(qkv: torch.Tensor, B: int, T: int, H: int, scale: float, precision: str = "f32") -> torch.Tensor:
    """softmax(scale * q k^T) v per (batch, head) of the ViT image encoder (csrc/vit_attention.hip): qkv f32
    [B, T, 3, H, 64] as nn.Linear(384, 1152) writes it -> o f32 [B, T, H*64], head-major.  precision "f32" or "bf16"
    (q, k, v and the probabilities rounded to bf16; f32 accumulation).  The scores never reach memory."""
    require_device()
    _chk(qkv, torch.float32, "qkv")
    if precision not in VIT_ATTN_PRECISIONS:
        raise RuntimeError(f"precision must be 'f32' or 'bf16', got {precision!r}")
    d = lib.usc_vit_attn_head_dim()
    if qkv.numel() != B * T * 3 * H * d:
        raise RuntimeError(f"qkv must hold [B={B}, T={T}, 3, H={H}, {d}] values, got {list(qkv.shape)}")
    o = torch.empty((B, T, H * d), dtype=torch.float32, device=qkv.device)
    check(lib.usc_vit_attn_fwd(_ptr(qkv), B, T, H, float(scale), VIT_ATTN_PRECISIONS[precision], _ptr(o), _stream()),
          "usc_vit_attn_fwd")
    return o


def cc_eps(xyz: torch.Tensor, eps: float, max_rounds: int = 256) -> torch.Tensor:
    """Connected components of the eps-ball graph == DBSCAN(eps, min_samples=1).labels_ (first-seen order)."""
    require_device()
    _chk(xyz, torch.float32, "xyz")
    n = xyz.shape[0]
    dev = xyz.device
    la = torch.empty(n, dtype=torch.int32, device=dev)
    lb = torch.empty(n, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.usc_cc_eps_init(_ptr(la), n, _stream()), "usc_cc_eps_init")
    for _ in range(max_rounds):
        check(lib.usc_cc_eps_step(_ptr(xyz), n, float(eps), _ptr(la), _ptr(lb), _ptr(changed), _stream()),
              "usc_cc_eps_step")
        la, lb = lb, la
        if int(changed.item()) == 0:
            break
    else:
        raise RuntimeError("cc_eps: label propagation did not converge")
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    check(lib.usc_cc_eps_finish(_ptr(la), n, _ptr(lb), _ptr(labels), _stream()), "usc_cc_eps_finish")
    return labels


DBSCAN_OFF = -2                           # label of a point outside the query's mask (noise is sklearn's -1)
DBSCAN_MAX_CELLS_PER_AXIS = 1 << 20       # USC_DBSCAN_MAX_CELLS_PER_AXIS


def dbscan_masks(xyz: torch.Tensor, masks: torch.Tensor, eps: float, min_samples: int = 1):
    """sklearn.cluster.DBSCAN(eps, min_samples) of every query mask of one scene in one pass (csrc/dbscan.hip).

    xyz f32[N,3], masks f32[N,Q] (on: > 0) -> (labels i32[N,Q], n_clusters i32[Q]).  An on-point carries the label
    sklearn gives it among the on-points of its query (-1: noise), an off-point DBSCAN_OFF.  Distances as in
    `cc_eps`: f64 on the f32 coordinates against the f32 eps squared in f64.  The host reads the scene's bounding box
    (to size the grid and to refuse non-finite coordinates) and the number of occupied cells, nothing else."""
    require_device()
    _chk(xyz, torch.float32, "xyz")
    _chk(masks, torch.float32, "masks")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or masks.dim() != 2 or masks.shape[0] != xyz.shape[0]:
        raise RuntimeError(f"dbscan_masks: xyz must be [N,3] and masks [N,Q], got {list(xyz.shape)}, {list(masks.shape)}")
    eps32 = ctypes.c_float(float(eps)).value              # the value that crosses the ABI
    if not (eps32 > 0.0) or eps32 == float("inf"):
        raise RuntimeError(f"dbscan_masks: eps must be positive and finite, got {eps}")
    if int(min_samples) != min_samples or int(min_samples) < 1:
        raise RuntimeError(f"dbscan_masks: min_samples must be an integer >= 1, got {min_samples}")
    min_samples = int(min_samples)
    N, Q = masks.shape
    dev = xyz.device
    labels = torch.empty((N, Q), dtype=torch.int32, device=dev)
    n_clusters = torch.zeros(Q, dtype=torch.int32, device=dev)
    if N == 0 or Q == 0:
        return labels, n_clusters
    lo, hi = (t.double().cpu() for t in torch.aminmax(xyz, dim=0))
    if not (bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all())):
        raise RuntimeError("dbscan_masks: non-finite coordinates")
    cells = torch.floor((hi - lo) / (eps32 * 0.5)) + 1
    if float(cells.max()) > DBSCAN_MAX_CELLS_PER_AXIS:
        raise RuntimeError(f"dbscan_masks: eps = {eps32} needs {[int(c) for c in cells]} cells over the scene's extent, "
                           f"more than {DBSCAN_MAX_CELLS_PER_AXIS} along an axis")
    nx, ny, nz = (int(c) for c in cells)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    check(lib.usc_dbscan_cell_keys(_ptr(xyz), N, eps32, float(lo[0]), float(lo[1]), float(lo[2]), nx, ny, nz, _ptr(keys),
                                   _stream()), "usc_dbscan_cell_keys")
    keys, order = torch.sort(keys, stable=True)           # stable: original indices ascend inside a cell
    cell_keys, cell_of, counts = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
    M = cell_keys.shape[0]                                # host read: the number of occupied cells
    cell_of = cell_of.to(torch.int32)
    cell_start = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = counts.cumsum(0)
    nbr = torch.empty((M, 125), dtype=torch.int32, device=dev)
    check(lib.usc_dbscan_neighbor_table(_ptr(cell_keys), M, nx, ny, nz, _ptr(nbr), _stream()), "usc_dbscan_neighbor_table")
    xs = xyz.index_select(0, order)
    ws = _ws(lib.usc_dbscan_ws_bytes(N, Q, M, min_samples), dev)
    check(lib.usc_dbscan_labels(_ptr(xs), _ptr(order), _ptr(cell_of), _ptr(cell_start), _ptr(nbr), _ptr(masks), N, Q, M,
                                eps32, min_samples, _ptr(ws), ws.numel(), _ptr(labels), _ptr(n_clusters), _stream()),
          "usc_dbscan_labels")
    return labels, n_clusters


def dbscan_expand(masks: torch.Tensor, labels: torch.Tensor, col_start: torch.Tensor, n_cols: int) -> torch.Tensor:
    """One column per (query, cluster): out f32[N,n_cols], out[i, col_start[q] + labels[i,q]] = masks[i,q] where the
    label is >= 0, else 0.  col_start i64[Q] (exclusive prefix of the clusters per query)."""
    require_device()
    _chk(masks, torch.float32, "masks")
    _chk(labels, torch.int32, "labels")
    _chk(col_start, torch.int64, "col_start")
    if labels.shape != masks.shape or col_start.shape[0] != masks.shape[1]:
        raise RuntimeError("dbscan_expand: labels must match masks [N,Q] and col_start must be [Q]")
    N, Q = masks.shape
    out = torch.zeros((N, int(n_cols)), dtype=torch.float32, device=masks.device)
    if N and Q and n_cols:
        check(lib.usc_dbscan_expand(_ptr(masks), _ptr(labels), _ptr(col_start), N, Q, int(n_cols), _ptr(out), _stream()),
              "usc_dbscan_expand")
    return out


# ------------------------------------------------------------------ dataset tables (csrc/dataset.hip)
def softmask_stats(soft: torch.Tensor, xyz: torch.Tensor, thr: float):
    """Per column of soft f32[N,K]: -> (count i32[K] of the rows with soft > f32(thr), lo f32[K,2], hi f32[K,2] = min /
    max of x and y (xyz f32[N,3]) over those rows; an empty column gives +max / -max of f32)."""
    require_device()
    _chk(soft, torch.float32, "soft")
    _chk(xyz, torch.float32, "xyz")
    if soft.dim() != 2 or soft.shape[0] < 1 or soft.shape[1] < 1 or xyz.shape != (soft.shape[0], 3):
        raise RuntimeError("softmask_stats: soft must be f32 [N>=1, K>=1] and xyz f32 [N,3]")
    N, K = soft.shape
    dev = soft.device
    count = torch.empty(K, dtype=torch.int32, device=dev)
    lo = torch.empty((K, 2), dtype=torch.float32, device=dev)
    hi = torch.empty((K, 2), dtype=torch.float32, device=dev)
    ws = _ws(lib.usc_softmask_stats_ws_bytes(N, K), dev)
    check(lib.usc_softmask_stats(_ptr(soft), _ptr(xyz), N, K, float(thr), _ptr(count), _ptr(lo), _ptr(hi), _ptr(ws),
                                 ws.numel(), _stream()), "usc_softmask_stats")
    return count, lo, hi


def softmask_table(soft: torch.Tensor, thr: float, keep, segments: torch.Tensor) -> torch.Tensor:
    """-> i32[N, len(keep)+2]: column 0 = any kept column set, columns 1.. = soft[:, keep] > f32(thr) as 0/1, the last
    column = (int32)segments.  `keep`: a host list of column indices."""
    require_device()
    _chk(soft, torch.float32, "soft")
    _chk(segments, torch.float32, "segments")
    N, K = soft.shape
    keep = [int(j) for j in keep]
    if not keep or min(keep) < 0 or max(keep) >= K or segments.shape != (N,):
        raise RuntimeError(f"softmask_table: keep must hold indices in [0, {K}) and segments must be f32 [{N}]")
    keep_d = torch.tensor(keep, dtype=torch.int32, device=soft.device)
    out = torch.empty((N, len(keep) + 2), dtype=torch.int32, device=soft.device)
    check(lib.usc_softmask_table(_ptr(soft), N, K, float(thr), _ptr(keep_d), len(keep), _ptr(segments), _ptr(out),
                                 _stream()), "usc_softmask_table")
    return out


# ------------------------------------------------------------------ self-training bit rows (csrc/selftrain.hip)
def _bit_words(n: int) -> int:
    return (int(n) + 63) // 64


def _chk_bits(bits: torch.Tensor, n: int, name: str):
    """Bit rows travel as int64 tensors (the u64 bit pattern), [rows, ceil(n / 64)]."""
    _chk(bits, torch.int64, name)
    if bits.dim() != 2 or bits.shape[1] != _bit_words(n):
        raise RuntimeError(f"{name} must be int64 [rows, {_bit_words(n)}] (bit rows of {n} points), got "
                           f"{tuple(bits.shape)}")
    return bits


def mask_columns_to_bits(masks: torch.Tensor):
    """masks bool / uint8 [N>=1, K] (non-zero = set) -> (bits i64[K, ceil(N/64)]: column j as a bit row, point r = bit
    r % 64 of word r / 64, zero beyond N; count i32[K] = the column popcounts)."""
    require_device()
    if isinstance(masks, torch.Tensor) and masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _chk(masks, torch.uint8, "masks")
    if masks.dim() != 2 or masks.shape[0] < 1:
        raise RuntimeError("mask_columns_to_bits: masks must be bool or uint8 [N>=1, K]")
    N, K = masks.shape
    bits = torch.empty((K, _bit_words(N)), dtype=torch.int64, device=masks.device)
    count = torch.empty(K, dtype=torch.int32, device=masks.device)
    if K:
        check(lib.usc_mask_columns_to_bits(_ptr(masks), N, K, _ptr(bits), _ptr(count), _stream()),
              "usc_mask_columns_to_bits")
    return bits, count


def mask_bits_count(bits: torch.Tensor, n: int) -> torch.Tensor:
    """Set bits of every row of bits i64[K, ceil(n/64)] -> i32[K]."""
    require_device()
    _chk_bits(bits, n, "bits")
    count = torch.empty(bits.shape[0], dtype=torch.int32, device=bits.device)
    if bits.shape[0]:
        check(lib.usc_mask_bits_count(_ptr(bits), bits.shape[0], int(n), _ptr(count), _stream()), "usc_mask_bits_count")
    return count


def mask_bits_gather(src: torch.Tensor, m: int, ind: torch.Tensor, check_range: bool = True):
    """Bit rows of `masks[ind]`: src i64[K, ceil(m/64)] (bit rows over m points), ind i64[N>=1] with every entry in
    [0, m) (checked here with one host read; `check_range=False`: the caller vouches for it, e.g. `knn1`'s output)
    -> (dst i64[K, ceil(N/64)], count i32[K])."""
    require_device()
    _chk_bits(src, m, "src")
    _chk(ind, torch.int64, "ind")
    if ind.dim() != 1 or ind.shape[0] < 1 or m < 1:
        raise RuntimeError("mask_bits_gather: ind must be int64 [N>=1] and m >= 1")
    if check_range:
        lo, hi = torch.aminmax(ind)                   # the kernel dereferences the indices
        if int(lo) < 0 or int(hi) >= m:
            raise RuntimeError(f"mask_bits_gather: index out of range [0, {m}) (min {int(lo)}, max {int(hi)})")
    N, K = ind.shape[0], src.shape[0]
    dst = torch.empty((K, _bit_words(N)), dtype=torch.int64, device=src.device)
    count = torch.empty(K, dtype=torch.int32, device=src.device)
    if K:
        check(lib.usc_mask_bits_gather(_ptr(src), int(m), _ptr(ind), N, K, _ptr(dst), _ptr(count), _stream()),
              "usc_mask_bits_gather")
    return dst, count


def selftrain_merge(st: torch.Tensor, total: torch.Tensor, n: int, fg: torch.Tensor, max_add: int):
    """The greedy merge of the self-training reader on bit rows: st i64[K', W] the exported instances (most confident
    first), total i32[K'] their sizes, fg i64[W] the covered points (UPDATED IN PLACE), W = ceil(n/64).  Row j is
    taken when total[j] > 0 and 2 * popcount(st[j] & ~fg) > total[j]; only its uncovered part is added.
    -> (fresh i64[max_add, W], picked i32[max_add] (-1 past the end), n_added i32[1]), all on the device."""
    require_device()
    _chk_bits(st, n, "st")
    _chk(total, torch.int32, "total")
    _chk(fg, torch.int64, "fg")
    W, kp, max_add = _bit_words(n), st.shape[0], int(max_add)
    if n < 1 or total.shape != (kp,) or fg.shape != (W,) or max_add < 0:
        raise RuntimeError(f"selftrain_merge: needs n >= 1, total i32[{kp}], fg i64[{W}] and max_add >= 0")
    dev = st.device
    fresh = torch.empty((max_add, W), dtype=torch.int64, device=dev)
    picked = torch.empty(max_add, dtype=torch.int32, device=dev)
    n_added = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.usc_selftrain_merge(_ptr(st) if kp else None, _ptr(total) if kp else None, kp, int(n), _ptr(fg), max_add,
                                  _ptr(fresh) if max_add else None, _ptr(picked) if max_add else None, _ptr(n_added),
                                  _stream()), "usc_selftrain_merge")
    return fresh, picked, n_added


def mask_bits_to_columns(bits: torch.Tensor, n: int, rows=None, out: torch.Tensor = None, col0: int = 0,
                         dtype=torch.float32):
    """Columns from bit rows: out[r, col0 + i] = bit r of bits[rows[i]] as 0 / 1, r < n.  rows: a host list or an
    i32 device tensor of row indices (None: every row in order).  out: f32 or uint8 [n, >= col0 + len(rows)]
    (row-major; allocated as [n, len(rows)] of `dtype` when None; torch.bool is written as uint8).  -> out."""
    require_device()
    _chk_bits(bits, n, "bits")
    if rows is None:
        rows = torch.arange(bits.shape[0], dtype=torch.int32, device=bits.device)
    elif not isinstance(rows, torch.Tensor):
        rows = [int(j) for j in rows]
        if rows and (min(rows) < 0 or max(rows) >= bits.shape[0]):
            raise RuntimeError(f"mask_bits_to_columns: rows must hold indices in [0, {bits.shape[0]})")
        rows = torch.tensor(rows, dtype=torch.int32, device=bits.device)
    _chk(rows, torch.int32, "rows")
    m = rows.shape[0]
    if out is None:
        if dtype not in (torch.float32, torch.uint8, torch.bool):
            raise RuntimeError("mask_bits_to_columns: dtype must be float32, uint8 or bool")
        out = torch.empty((int(n), m), dtype=torch.uint8 if dtype == torch.bool else dtype, device=bits.device)
        ret = out.view(torch.bool) if dtype == torch.bool else out
    else:
        ret = out
    if out.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"mask_bits_to_columns: out must be float32 or uint8, got {out.dtype}")
    _chk(out, out.dtype, "out")
    if out.dim() != 2 or out.shape[0] != n or col0 < 0 or out.shape[1] < col0 + m:
        raise RuntimeError(f"mask_bits_to_columns: out must be [{n}, >= {col0 + m}], got {tuple(out.shape)}")
    fn = lib.usc_mask_bits_to_columns if out.dtype == torch.float32 else lib.usc_mask_bits_to_columns_u8
    if n and m:
        check(fn(_ptr(bits), _ptr(rows), m, int(n), _ptr(out), out.shape[1], int(col0), _stream()),
              "usc_mask_bits_to_columns")
    return ret


# ------------------------------------------------------------------ separate_instances (csrc/separate.hip)
def mask_columns_to_segment_bits(masks: torch.Tensor, csr: SegmentCSR, check_range: bool = True) -> torch.Tensor:
    """masks bool / uint8 [N>=1, K] (non-zero = set), csr = `segment_csr(idx, S)` of the points' segment indices
    -> bits i64[K, ceil(S/64)]: bit s of row j is set when any point of segment s has column j set.
    The CSR's values are checked here before the launch (seg_off rises from 0 to N, order within [0, N): host reads);
    `check_range=False`: the caller vouches for them (a CSR that `segment_csr` just built)."""
    require_device()
    if isinstance(masks, torch.Tensor) and masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _chk(masks, torch.uint8, "masks")
    if masks.dim() != 2 or masks.shape[0] < 1:
        raise RuntimeError("mask_columns_to_segment_bits: masks must be bool or uint8 [N>=1, K]")
    N, K = masks.shape
    S = int(csr.S)
    _chk(csr.order, torch.int64, "csr.order")
    _chk(csr.seg_off, torch.int64, "csr.seg_off")
    if csr.order.shape != (N,) or csr.seg_off.shape != (S + 1,):
        raise RuntimeError(f"mask_columns_to_segment_bits: the CSR must cover the {N} rows of masks (order i64[{N}], "
                           f"seg_off i64[{S + 1}])")
    if check_range:
        off = csr.seg_off.cpu()
        if int(off[0]) != 0 or int(off[-1]) != N or bool((off[1:] < off[:-1]).any()):
            raise RuntimeError(f"mask_columns_to_segment_bits: csr.seg_off must rise from 0 to {N}")
        lo, hi = torch.aminmax(csr.order)
        if int(lo) < 0 or int(hi) >= N:
            raise RuntimeError(f"mask_columns_to_segment_bits: csr.order outside [0, {N})")
    bits = torch.empty((K, _bit_words(S)), dtype=torch.int64, device=masks.device)
    if K:
        check(lib.usc_mask_columns_to_segment_bits(_ptr(masks), N, K, _ptr(csr.order), _ptr(csr.seg_off), S,
                                                   _ptr(bits), _stream()), "usc_mask_columns_to_segment_bits")
    return bits


def segment_parts_to_columns(label: torch.Tensor, src: torch.Tensor, root: torch.Tensor, idx: torch.Tensor,
                             check_range: bool = True) -> torch.Tensor:
    """label i32[n, S] (`mask_components`), parts (src i32[R] in [0, n), root i32[R]), idx i32[N] in [0, S)
    -> bool[N, R]: out[r, p] = (label[src[p], idx[r]] == root[p]).  src and idx are checked here (host reads;
    `check_range=False`: the caller vouches for them)."""
    require_device()
    for t, name in ((label, "label"), (src, "src"), (root, "root"), (idx, "idx")):
        _chk(t, torch.int32, name)
    if label.dim() != 2 or label.shape[1] < 1 or src.dim() != 1 or root.shape != src.shape or idx.dim() != 1:
        raise RuntimeError("segment_parts_to_columns: needs label i32[n, S>=1], src i32[R], root i32[R], idx i32[N]")
    n, S = label.shape
    R, N = src.shape[0], idx.shape[0]
    if check_range:
        if R and (int(src.min()) < 0 or int(src.max()) >= n):
            raise RuntimeError(f"segment_parts_to_columns: src outside [0, {n})")
        if N and (int(idx.min()) < 0 or int(idx.max()) >= S):
            raise RuntimeError(f"segment_parts_to_columns: idx outside [0, {S})")
    out = torch.empty((N, R), dtype=torch.uint8, device=label.device)
    if N and R:
        check(lib.usc_segment_parts_to_columns(_ptr(label), n, S, _ptr(src), _ptr(root), R, _ptr(idx), N, _ptr(out),
                                               _stream()), "usc_segment_parts_to_columns")
    return out.view(torch.bool)


def mesh_vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Area-weighted vertex normals of a triangle mesh (vertices f32[V,3], faces i32[F,3]) -> f32[V,3]: the sum of the
    unnormalised face normals (v1-v0)x(v2-v0) over a vertex's faces in ascending face order, in f64, normalised; a
    vertex with no face or a zero / non-finite sum gets (0,0,1).  open3d's `compute_vertex_normals` as published —
    open3d is not available to pin it against: UNPINNED."""
    require_device()
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    V, F = vertices.shape[0], faces.shape[0]
    if F == 0 or V == 0:
        return torch.tensor([0.0, 0.0, 1.0], device=vertices.device).repeat(V, 1)
    lo, hi = torch.aminmax(faces)                     # the kernel dereferences the indices
    if int(lo) < 0 or int(hi) >= V:
        raise RuntimeError(f"mesh_vertex_normals: face index out of range [0, {V}) (min {int(lo)}, max {int(hi)})")
    csr = segment_csr(faces.reshape(-1).to(torch.int64).contiguous(), V)     # stable: ascending face order
    normals = torch.empty((V, 3), dtype=torch.float32, device=vertices.device)
    check(lib.usc_mesh_vertex_normals(_ptr(vertices), _ptr(faces), _ptr(csr.order), _ptr(csr.seg_off), V, F,
                                      _ptr(normals), _stream()), "usc_mesh_vertex_normals")
    return normals


# ------------------------------------------------------------------ decoder-side small-row ops
_LN_DIMS = {64, 128, 192, 256, 384, 512}


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, passthrough=False):
        d = x.shape[-1]
        x2 = x.contiguous().view(-1, d)
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.usc_layernorm_fwd(_ptr(x2), _ptr(weight), _ptr(bias), rows, d, float(eps), _ptr(y), _ptr(mean),
                                    _ptr(rstd), _stream()), "usc_layernorm_fwd")
        ctx.save_for_backward(x2, weight, mean, rstd)
        ctx.shape = x.shape
        ctx.w_param, ctx.b_param = weight, bias
        ctx.passthrough = bool(passthrough)
        # passthrough: x comes back as a second output; the gradient that arrives there (x's other consumer) is summed
        # inside the backward launch (usc_layernorm_bwd_ex: dx_add) instead of by a separate autograd add
        return (y.view(x.shape), x) if passthrough else y.view(x.shape)

    @staticmethod
    def backward(ctx, dy, dpass=None):
        x2, weight, mean, rstd = ctx.saved_tensors
        rows, d = x2.shape
        if dy is None:                                  # only the passthrough output was used
            return (None if dpass is None else dpass), None, None, None, None
        dy2 = dy.contiguous().view(rows, d)
        dadd = None if dpass is None else dpass.contiguous().view(rows, d)
        # x is the output buffer of a captured decoder pass: its gradient goes straight into the buffer the pass's
        # backward graph reads (graphs.grad_buffer_for), which saves the copy in front of the replay.  Safe whether or
        # not this norm is x's only consumer: if autograd has to add another consumer's gradient, the sum is a new
        # tensor and _GraphedFn.backward copies it over what was written here before it replays.
        from .graphs import grad_buffer_for
        buf = grad_buffer_for(x2)
        dx = buf.view(rows, d) if buf is not None else torch.empty_like(x2)
        (dgamma, dbeta), in_place, finish = _param_grads((ctx.w_param, ctx.b_param))
        wsb = lib.usc_layernorm_bwd_ws_bytes(rows, d)
        ws = _ws(wsb, x2.device) if wsb > 0 else None
        check(lib.usc_layernorm_bwd_ex(_ptr(dy2), _ptr(x2), _ptr(mean), _ptr(rstd), _ptr(weight), rows, d, _ptr(dadd),
                                       _ptr(dx), _ptr(dgamma), _ptr(dbeta), int(in_place), _ptr(ws), wsb, _stream()),
              "usc_layernorm_bwd")
        return (dx.view(ctx.shape),) + finish() + (None, None)


class _AddLayerNorm(torch.autograd.Function):
    """LayerNorm(x + res) in one launch; both addends receive the same input gradient (no extra kernel)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        d = x.shape[-1]
        x2 = x.contiguous().view(-1, d)
        r2 = res.contiguous().view(-1, d)
        rows = x2.shape[0]
        y, ssum = torch.empty_like(x2), torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.usc_add_layernorm_fwd(_ptr(x2), _ptr(r2), _ptr(weight), _ptr(bias), rows, d, float(eps), _ptr(y),
                                        _ptr(ssum), _ptr(mean), _ptr(rstd), _stream()), "usc_add_layernorm_fwd")
        ctx.save_for_backward(ssum, weight, mean, rstd)
        ctx.shape = x.shape
        ctx.w_param, ctx.b_param = weight, bias
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        dx, dgamma, dbeta, _, _ = _LayerNorm.backward(ctx, dy)
        return dx, dx, dgamma, dbeta, None


def add_layer_norm(x, res, weight, bias, eps=1e-5):
    """F.layer_norm(x + res) (the post-norm residual of the decoder layers, reference models/mask3d.py:523-524)."""
    _chk(weight, torch.float32, "weight")
    _chk(bias, torch.float32, "bias")
    if x.dtype != torch.float32 or not x.is_cuda or x.shape[-1] not in _LN_DIMS or x.shape != res.shape:
        raise RuntimeError(f"add_layer_norm: needs two equal-shape f32 HIP tensors with last dim in {sorted(_LN_DIMS)}")
    return _AddLayerNorm.apply(x, res, weight, bias, eps)


def layer_norm(x, weight, bias, eps=1e-5, passthrough=False):
    """F.layer_norm over the last dimension through the HIP kernels (f32, contiguous weight/bias, d in _LN_DIMS).
    passthrough: -> (y, x'), x' = x as an output of the same autograd node: hand it to x's OTHER consumer and that
    consumer's gradient is summed inside this norm's backward launch."""
    _chk(weight, torch.float32, "weight")
    _chk(bias, torch.float32, "bias")
    if x.dtype != torch.float32 or not x.is_cuda or x.shape[-1] not in _LN_DIMS:
        raise RuntimeError(f"layer_norm: needs an f32 HIP tensor with last dim in {sorted(_LN_DIMS)}")
    return _LayerNorm.apply(x, weight, bias, eps, passthrough)


# linear layers with at most this many rows go to the tile-per-workgroup kernels of decoder.hip (the 100 queries; the
# few hundred to a thousand segments of the mask logits: 5 us per launch against 11-21 us on the many-row kernels)
SMALL_ROWS = 1024


def _small_linear_ok(rows, n_in, n_out):
    return rows <= SMALL_ROWS and n_in % 32 == 0 and n_out % 32 == 0 and n_in >= 32 and n_out >= 32


def _rows_gemm_ok(rows, n_in, n_out):
    """Many-row linear layers (the sampled voxels of a decoder pass: 200 ... 12 800 rows; segment logits) run on the
    1x1-convolution kernels — the library's heuristics pick 30-95 us kernels for these 0.1-0.4 GFLOP shapes."""
    return rows > SMALL_ROWS and n_in % 32 == 0 and n_out % 32 == 0


def _lin_fwd(x2, W, b, add=None, relu=False, pad_rows_to=None, out=None):
    """y = (x2 [+ add]) W^T + b [then ReLU] for contiguous f32 x2 [M,K], W [N,K] (a contiguous row block is fine);
    `add` / `relu` are folded into the launch on the few-row kernels and applied separately elsewhere.
    pad_rows_to: y gets that many rows, the extra ones zero (few-row kernels only)."""
    M, K = x2.shape
    N = W.shape[0]
    if _small_linear_ok(M, K, N):
        Mp = M if pad_rows_to is None else int(pad_rows_to)
        y = torch.empty((Mp, N), dtype=torch.float32, device=x2.device) if out is None else out
        if tuple(y.shape) != (Mp, N) or y.dtype != torch.float32 or not y.is_contiguous():
            raise RuntimeError(f"linear: `out` must be a contiguous f32 [{Mp}, {N}] tensor")
        check(lib.usc_linear_fwd_pad(_ptr(x2), _ptr(add), _ptr(W), _ptr(b), M, N, K, int(relu), _ptr(y), Mp, _stream()),
              "usc_linear_fwd")
        return y
    if pad_rows_to is not None:
        raise RuntimeError("linear: pad_rows_to needs the few-row kernels (rows <= 1024, widths multiples of 32)")
    if add is not None:
        x2 = x2 + add
    if relu:
        return torch.relu_(_lin_fwd(x2, W, b, out=out))
    if _rows_gemm_ok(M, K, N) and W.is_contiguous():
        # W [N, K] is the product's [cout][cin]: read in place by the row-order kernel (was: a transpose launch per call,
        # 36 per training step inside the captured decoder passes)
        return gather_gemm(x2, W.view(1, N, K), None, M, bias=b, out=out, w_transposed=True)
    y = torch.addmm(b, x2, W.t()) if b is not None else x2 @ W.t()
    return y if out is None else out.copy_(y)


def col_sum(x2, out, accumulate=False):
    """out[c] (+)= sum_r x2[r, c] in a fixed order (usc_col_sum).  Not torch.sum: replayed from the captured decoder
    graphs, ATen's multi-block reduction left the bias gradients of the 3 200 / 12 800-row projections at the value
    of the previous reduction that had used the same scratch block (found by the padded-level graph test)."""
    _chk(x2, torch.float32, "x2")
    if not out.is_contiguous() or out.dtype != torch.float32 or out.numel() != x2.shape[1]:
        raise RuntimeError("col_sum: `out` must be a contiguous f32 vector with one entry per column")
    wsb = lib.usc_col_sum_ws_bytes(x2.shape[0], x2.shape[1])
    ws = _ws(wsb, x2.device)
    check(lib.usc_col_sum(_ptr(x2), x2.shape[0], x2.shape[1], _ptr(out), int(accumulate), _ptr(ws), wsb, _stream()),
          "usc_col_sum")
    return out


def _lin_bwd(dy2, x2, W, dW_out, db_out, need_dx=True, accumulate=False, add=None, y_relu=None, dx_add=None,
             dx_add2=None, want_dx_b=False):
    """-> dx (or None); writes (accumulate: adds) dW_out [N,K] and db_out [N] (row-block views are fine).
    add: the layer's input was x2 + add; y_relu: its output after the fused ReLU; dx_add: added to dx.
    dx_add2 / want_dx_b: -> (dx, dx_b) with dx = dy W + dx_add + dx_add2 and dx_b = dy W + dx_add (usc_linear_bwd_ex2)."""
    M, N = dy2.shape
    K = x2.shape[1]
    if want_dx_b or dx_add2 is not None:
        if not need_dx:                          # the parameter gradients only
            _lin_bwd(dy2, x2, W, dW_out, db_out, False, accumulate, add, y_relu)
            return (None, None) if want_dx_b else None
        if _small_linear_ok(M, K, N):
            dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
            dx_b = torch.empty_like(dx) if want_dx_b else None
            check(lib.usc_linear_bwd_ex2(_ptr(dy2), _ptr(y_relu), _ptr(x2), _ptr(add), _ptr(W), M, N, K, _ptr(dx),
                                         _ptr(dx_add), _ptr(dx_add2), _ptr(dx_b), _ptr(dW_out), _ptr(db_out),
                                         int(accumulate), _stream()), "usc_linear_bwd")
        else:
            dx_b = _lin_bwd(dy2, x2, W, dW_out, db_out, True, accumulate, add, y_relu, dx_add)
            dx = dx_b if dx_add2 is None else dx_b + dx_add2
        return (dx, dx_b) if want_dx_b else dx
    if _small_linear_ok(M, K, N):
        dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device) if need_dx else None
        check(lib.usc_linear_bwd_ex(_ptr(dy2), _ptr(y_relu), _ptr(x2), _ptr(add), _ptr(W), M, N, K, _ptr(dx),
                                    _ptr(dx_add) if need_dx else None, _ptr(dW_out), _ptr(db_out), int(accumulate),
                                    _stream()), "usc_linear_bwd")
        return dx
    if y_relu is not None:
        dy2 = dy2 * (y_relu > 0)
    if add is not None:
        x2 = x2 + add
    if dx_add is not None:
        dx = _lin_bwd(dy2, x2, W, dW_out, db_out, need_dx, accumulate)
        return None if dx is None else dx.add_(dx_add)
    rows_ok = _rows_gemm_ok(M, K, N) and W.is_contiguous()
    if rows_ok and dW_out.is_contiguous():
        # dW[N,K] = dy^T x over many rows: the weight-gradient kernel with identity pairs (a = dy, b = x)
        if accumulate:
            wgrad(dy2, x2, 1, into=dW_out)
        else:
            wgrad(dy2, x2, 1, out=dW_out)
    elif accumulate:
        dW_out.addmm_(dy2.t(), x2)
    else:
        torch.mm(dy2.t(), x2, out=dW_out)
    if db_out is not None:
        col_sum(dy2, db_out, accumulate)
    if not need_dx:
        return None
    if rows_ok:
        return gather_gemm(dy2, W.view(1, N, K), None, M)                # W [N, K] is this product's [cin, cout]
    return dy2 @ W


def linear_heads_dx(dys, Ws):
    """dx [M,K] = P_0 + (P_1 + ( ... + P_{L-1})), P_l = dys[l] [M,N] @ Ws[l] [N,K]: the input gradient of L linear heads
    over one input (the mask-logit products over the segment table) without the L-long chain of
    `linear(..., passthrough=True)` nodes — and with its bits: one launch on the few-row kernels
    (usc_linear_heads_dx), head by head on the kernels the chain takes above SMALL_ROWS."""
    L = len(dys)
    M, N = dys[0].shape
    K = Ws[0].shape[1]
    for dy, W in zip(dys, Ws):
        _chk(dy, torch.float32, "dy")
        _chk(W, torch.float32, "W")
        if tuple(dy.shape) != (M, N) or tuple(W.shape) != (N, K):
            raise RuntimeError("linear_heads_dx: every head needs dy [M, N] and W [N, K] of the same shape")
    if _small_linear_ok(M, K, N):
        if L > lib.usc_linear_heads_max():
            raise RuntimeError(f"linear_heads_dx: at most {lib.usc_linear_heads_max()} heads in one launch, got {L}")
        pd = (ctypes.c_void_p * L)(*[dy.data_ptr() for dy in dys])
        pw = (ctypes.c_void_p * L)(*[W.data_ptr() for W in Ws])
        dx = torch.empty((M, K), dtype=torch.float32, device=dys[0].device)
        check(lib.usc_linear_heads_dx(pd, pw, L, M, N, K, _ptr(dx), _stream()), "usc_linear_heads_dx")
        return dx
    dx = None
    rows_ok = _rows_gemm_ok(M, K, N)
    for l in range(L - 1, -1, -1):                      # what _lin_bwd does for one head of the chain, minus dW
        W = Ws[l]
        p = gather_gemm(dys[l], W.view(1, N, K), None, M) if rows_ok and W.is_contiguous() else dys[l] @ W
        dx = p if dx is None else p.add_(dx)
    return dx


class _LinearRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, relu=False, passthrough=False, pad_rows_to=None):
        x2 = x.contiguous().view(-1, x.shape[-1])
        ctx.rows = x2.shape[0]
        if pad_rows_to is not None:
            if relu or passthrough or x2.shape[0] != x.shape[-2] or pad_rows_to < x2.shape[0]:
                raise RuntimeError("linear: pad_rows_to is for one [.., M, K] table, M <= pad_rows_to, without relu")
            y = _lin_fwd(x2, W, b, pad_rows_to=pad_rows_to)
            ctx.save_for_backward(x2, W, None)
            ctx.shape = x.shape
            ctx.w_param, ctx.b_param = W, b
            return y.view(*x.shape[:-2], int(pad_rows_to), W.shape[0])
        y = _lin_fwd(x2, W, b, relu=relu)
        ctx.save_for_backward(x2, W, y if relu else None)
        ctx.shape = x.shape
        ctx.w_param, ctx.b_param = W, b
        y = y.view(*x.shape[:-1], W.shape[0])
        # passthrough: x is handed back as a second output; whatever gradient arrives there (the residual path around
        # the layer) is added inside the input-gradient launch instead of by a separate autograd add
        return (y, x) if passthrough else y

    @staticmethod
    def backward(ctx, dy, dres=None):
        x2, W, y_relu = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, W.shape[0])[:ctx.rows]       # [:rows]: drops the zero-extension rows, if any
        (dW, db), in_place, finish = _param_grads((ctx.w_param, ctx.b_param))
        dres2 = None if dres is None else dres.contiguous().view(-1, x2.shape[1])
        dx = _lin_bwd(dy2, x2, W, dW, db, need_dx=ctx.needs_input_grad[0], accumulate=in_place, y_relu=y_relu,
                      dx_add=dres2)
        return (None if dx is None else dx.view(ctx.shape),) + finish() + (None, None, None)


def linear(x, W, b=None, relu=False, passthrough=False, pad_rows_to=None):
    """F.linear(x, W, b) (relu: followed by ReLU, in the same launch on the few-row kernels) for f32 HIP tensors;
    few-row inputs run on the wave-per-tile MFMA kernels of decoder.hip.
    passthrough: -> (y, x'), x' = x as an output of the same autograd node: use it for the residual connection
    around the layer, its gradient is then summed inside the layer's input-gradient launch.
    pad_rows_to: x is ONE table [.., M, K]; y comes back as [.., pad_rows_to, N] with zero rows appended (the
    gradient of those rows is dropped)."""
    _chk(W, torch.float32, "W")
    return _LinearRows.apply(x, W, b, relu, passthrough, pad_rows_to)


# The input projections of nn.MultiheadAttention from its packed in_proj_weight [3E,E] / in_proj_bias [3E] (reference:
# nn.MultiheadAttention inside models/mask3d.py:491-605) in the two forms the decoder uses: _InProjSelf (one input for
# q, k and v) and _InProjQ + _InProjKV (queries apart from the memory).  Every node writes its row blocks of ONE [3E,E]
# weight gradient / [3E] bias gradient; the `with_pos_embed` adds of the reference (:485, :517) are folded into the
# projection launches, and an input used twice gets one summed gradient chained through the input-gradient launches
# (dx_add) instead of separate tensors added by autograd.


def _rows(t, E):
    return None if t is None else t.contiguous().view(-1, E)


def _same_tensor(a, c):
    return a.data_ptr() == c.data_ptr() and a.shape == c.shape and a.stride() == c.stride()


class _InProjSelf(torch.autograd.Function):
    """Self attention: q = (x + pos) Wq^T + bq, k = (x + pos) Wk^T + bk, v = x Wv^T + bv.  residual: x comes back as a
    fourth output (the `tgt + attention(tgt ...)` residual of the decoder blocks); its gradient joins x's inside the
    input-gradient launches."""

    @staticmethod
    def forward(ctx, x, W, b, pos, residual=False):
        E = W.shape[1]
        x2, p2 = _rows(x, E), _rows(pos, E)
        M = x2.shape[0]
        xp = x2
        if p2 is not None and not _small_linear_ok(M, E, E):
            xp, p2 = x2 + p2, None                  # (many rows: no fused add on those kernels)
        if _small_linear_ok(M, E, 3 * E) and W.is_contiguous():
            # one launch for the three projections ([3, M, E], each its own matrix)
            y3 = torch.empty((3, M, E), dtype=torch.float32, device=W.device)
            check(lib.usc_linear_fwd_split(_ptr(x2), _ptr(p2), _ptr(W), _ptr(b), M, 3 * E, E, 2 * E, E, _ptr(y3),
                                           _stream()), "usc_linear_fwd_split")
            outs = (y3[0], y3[1], y3[2])
        else:
            outs = (_lin_fwd(xp, W[:E], b[:E], add=p2), _lin_fwd(xp, W[E:2 * E], b[E:2 * E], add=p2),
                    _lin_fwd(x2, W[2 * E:], b[2 * E:]))
        ctx.save_for_backward(xp, x2, W, p2)
        ctx.shape, ctx.pos_shape = x.shape, None if pos is None else pos.shape
        ctx.w_param, ctx.b_param = W, b
        out = tuple(o.view(*x.shape[:-1], E) for o in outs)
        return out + (x,) if residual else out

    @staticmethod
    def backward(ctx, dq, dk, dv, dres=None):
        xp, x2, W, p2 = ctx.saved_tensors
        E = W.shape[1]
        M = x2.shape[0]
        dres2 = _rows(dres, E)
        (dW, db), in_place, finish = _param_grads((ctx.w_param, ctx.b_param))
        need_x, need_pos = ctx.needs_input_grad[0], ctx.pos_shape is not None and ctx.needs_input_grad[3]
        adjacent = (dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous()
                    and dk.data_ptr() == dq.data_ptr() + 4 * M * E and dv.data_ptr() == dk.data_ptr() + 4 * M * E)
        if (need_x and adjacent and W.is_contiguous() and _small_linear_ok(M, 3 * E, E) and dW.is_contiguous()
                and db.is_contiguous()):
            # the attention core hands dq | dk | dv over as one table: the three projections backwards in one launch
            gx = torch.empty((M, E), dtype=torch.float32, device=W.device)
            gpos = torch.empty_like(gx) if need_pos else None
            check(lib.usc_qkv_proj_bwd(_ptr(dq), _ptr(x2), _ptr(p2), _ptr(W), M, E, _ptr(gx), _ptr(gpos), _ptr(dres2),
                                       _ptr(dW), _ptr(db), int(in_place), _stream()), "usc_qkv_proj_bwd")
        else:
            # v (+ residual) first, then k, then q on top of both; the q launch also writes the sum WITHOUT the
            # v / residual part — the positional term's gradient
            def bwd(j, dyj, xj, pj, **kw):
                return _lin_bwd(_rows(dyj, E), xj, W[j * E:(j + 1) * E], dW[j * E:(j + 1) * E], db[j * E:(j + 1) * E],
                                accumulate=in_place, add=pj, **kw)
            gv = bwd(2, dv, x2, None, need_dx=need_x, dx_add=dres2)
            gk = bwd(1, dk, xp, p2, need_dx=need_x or need_pos)
            gx, gpos = bwd(0, dq, xp, p2, need_dx=need_x or need_pos, dx_add=gk, dx_add2=gv, want_dx_b=True)
        return ((gx.view(ctx.shape) if need_x else None,) + finish()
                + (gpos.view(ctx.pos_shape) if need_pos else None, None))


class _InProjQ(torch.autograd.Function):
    """q = (x + pos) Wq^T + bq, Wq = in_proj_weight[:E] — the QUERY third on its own (reference models/mask3d.py:547-605
    CrossAttentionLayer, :517 with_pos_embed), so that the key / value thirds can be computed elsewhere (_InProjKV: they
    do not depend on the queries).  residual: x comes back as a second output and its gradient (the block's residual
    path) is summed inside the input-gradient launch."""

    @staticmethod
    def forward(ctx, x, W, b, pos, residual=False):
        E = W.shape[1]
        x2, p2 = _rows(x, E), _rows(pos, E)
        if p2 is not None and not _small_linear_ok(x2.shape[0], E, E):
            x2, p2 = x2 + p2, None
        y = _lin_fwd(x2, W[:E], b[:E], add=p2)
        ctx.save_for_backward(x2, W, p2)
        ctx.shape, ctx.pos_shape = x.shape, None if pos is None else pos.shape
        ctx.w_param, ctx.b_param = W, b
        y = y.view(*x.shape[:-1], E)
        return (y, x) if residual else y

    @staticmethod
    def backward(ctx, dq, dres=None):
        x2, W, p2 = ctx.saved_tensors
        E = W.shape[1]
        (dW, db), in_place, finish = _param_grads((ctx.w_param, ctx.b_param), zeros=True)
        dres2 = _rows(dres, E)
        need_pos = ctx.pos_shape is not None and ctx.needs_input_grad[3]
        if dres2 is not None and need_pos:
            gx, gpos = _lin_bwd(_rows(dq, E), x2, W[:E], dW[:E], db[:E], need_dx=True, accumulate=in_place, add=p2,
                                dx_add2=dres2, want_dx_b=True)
        else:
            gx = gpos = _lin_bwd(_rows(dq, E), x2, W[:E], dW[:E], db[:E], need_dx=True, accumulate=in_place, add=p2,
                                 dx_add=dres2)
        return (gx.view(ctx.shape),) + finish() + (gpos.view(ctx.pos_shape) if need_pos else None, None)


class _InProjKV(torch.autograd.Function):
    """k = (xk + pos) Wk^T + bk, v = xv Wv^T + bv with Wk, Wv = in_proj_weight[E:2E], [2E:3E]: the key / value thirds (in
    the decoder: over the sampled voxels of a pass, xk and xv one tensor).  `outs` (optional): (k, v) buffers to write
    into (the static inputs of a captured pass).  One tensor for both gets one summed gradient (k's part chained into
    v's launch)."""

    @staticmethod
    def forward(ctx, xk, xv, W, b, pos, outs=None):
        E = W.shape[1]
        ctx.shared = _same_tensor(xk, xv)
        k2, pk = _rows(xk, E), _rows(pos, E)
        v2 = k2 if ctx.shared else _rows(xv, E)
        if pk is not None and not _small_linear_ok(k2.shape[0], E, E):
            k2, pk = k2 + pk, None                  # (many rows: no fused add on those kernels)
        ok, ov = (None, None) if outs is None else (outs[0].detach().view(-1, E), outs[1].detach().view(-1, E))
        k = _lin_fwd(k2, W[E:2 * E], b[E:2 * E], add=pk, out=ok)
        v = _lin_fwd(v2, W[2 * E:], b[2 * E:], out=ov)
        ctx.save_for_backward(k2, v2, W, pk)
        ctx.shapes, ctx.pos_shape = (xk.shape, xv.shape), None if pos is None else pos.shape
        ctx.w_param, ctx.b_param = W, b
        return k.view(*xk.shape[:-1], E), v.view(*xv.shape[:-1], E)

    @staticmethod
    def backward(ctx, dk, dv):
        k2, v2, W, pk = ctx.saved_tensors
        E = W.shape[1]
        (dW, db), in_place, finish = _param_grads((ctx.w_param, ctx.b_param), zeros=True)
        need_k, need_v = ctx.needs_input_grad[:2]
        need_pos = ctx.pos_shape is not None and ctx.needs_input_grad[4]
        gk = _lin_bwd(_rows(dk, E), k2, W[E:2 * E], dW[E:2 * E], db[E:2 * E], need_dx=need_k or need_pos,
                      accumulate=in_place, add=pk)
        gv = _lin_bwd(_rows(dv, E), v2, W[2 * E:], dW[2 * E:], db[2 * E:], need_dx=need_v, accumulate=in_place,
                      dx_add=gk if ctx.shared else None)
        gpos = gk.view(ctx.pos_shape) if need_pos else None
        if ctx.shared:                              # gv is the sum: handed to the first of the two
            gk, gv = gv, None
        elif not need_k:
            gk = None
        return (None if gk is None else gk.view(ctx.shapes[0]), None if gv is None else gv.view(ctx.shapes[1])) \
            + finish() + (gpos, None)


def _in_proj_checks(name, W, b, x, pos):
    _chk(W, torch.float32, "in_proj_weight")
    _chk(b, torch.float32, "in_proj_bias")
    # the kernels read the positional term row for row: no broadcasting (a [Q,1,E] term with B > 1 would be read
    # out of bounds)
    if pos is not None and pos.shape != x.shape:
        raise RuntimeError(f"{name}: pos {tuple(pos.shape)} must have the shape of the input {tuple(x.shape)}")


def in_proj_q(x, W, b, pos=None, residual=False):
    _in_proj_checks("in_proj_q", W, b, x, pos)
    return _InProjQ.apply(x, W, b, pos, residual)


def in_proj_kv(x, W, b, pos=None, outs=None):
    _in_proj_checks("in_proj_kv", W, b, x, pos)
    return _InProjKV.apply(x, x, W, b, pos, outs)


def in_proj(xq, xk, xv, W, b, pos_q=None, pos_k=None, residual=False):
    """-> q, k, v (residual: and xq routed through the query's node).  One input for all three and one positional term
    (or none) for q and k: the self form; everything else: the query node and the key / value node."""
    _in_proj_checks("in_proj (query)", W, b, xq, pos_q)
    _in_proj_checks("in_proj (key)", W, b, xk, pos_k)
    if _same_tensor(xq, xk) and _same_tensor(xk, xv) and (pos_q is None) == (pos_k is None) \
            and (pos_q is None or _same_tensor(pos_q, pos_k)):
        return _InProjSelf.apply(xq, W, b, pos_q, residual)
    q = _InProjQ.apply(xq, W, b, pos_q, residual)
    k, v = _InProjKV.apply(xk, xv, W, b, pos_k, None)
    return (q[0], k, v, q[1]) if residual else (q, k, v)


ATTN_MAX_QUERIES = int(lib.usc_attn_max_queries())    # queries the fused attention and key-sampling kernels take (256)


class _MaskedCrossAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, num_heads):
        L, B, E = q.shape
        S = k.shape[0]
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        m8 = mask.contiguous().view(torch.uint8)
        o = torch.empty_like(q)
        lse = torch.empty((B * num_heads, lib.usc_attn_lse_stride(L)), dtype=torch.float32, device=q.device)
        wsb = lib.usc_attn_ws_bytes(L, S, B, num_heads)
        ws = _ws(wsb, q.device)
        check(lib.usc_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(m8), L, S, B, num_heads, E, _ptr(o), _ptr(lse), _ptr(ws),
                               wsb, _stream()), "usc_attn_fwd")
        ctx.save_for_backward(q, k, v, m8, o, lse, ws)       # ws: its head keeps the packed mask for the backward
        ctx.num_heads = num_heads
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, m8, o, lse, ws = ctx.saved_tensors
        L, B, E = q.shape
        S = k.shape[0]
        do = do.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        wsb = lib.usc_attn_ws_bytes(L, S, B, ctx.num_heads)
        check(lib.usc_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(m8), _ptr(o), _ptr(lse), _ptr(do), L, S, B, ctx.num_heads,
                               E, _ptr(dq), _ptr(dk), _ptr(dv), 1, _ptr(ws), wsb, _stream()), "usc_attn_bwd")
        return dq, dk, dv, None, None


def masked_cross_attention(q, k, v, mask_bsl, num_heads):
    """softmax(q k^T / 4 + mask) v per head for head dim 16: q [L,B,E], k/v [S,B,E] (f32, sequence-first),
    mask_bsl bool[B,S,L] with True = masked (the decoder's `batched_attn`, shared by all heads) -> [L,B,E]."""
    L, B, E = q.shape
    if (E != 16 * num_heads or L > ATTN_MAX_QUERIES or mask_bsl.dtype != torch.bool
            or tuple(mask_bsl.shape) != (B, k.shape[0], L)):
        raise RuntimeError(f"masked_cross_attention: needs head dim 16, <= {ATTN_MAX_QUERIES} queries and a bool[B,S,L] mask")
    return _MaskedCrossAttention.apply(q, k, v, mask_bsl, num_heads)


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, num_heads):
        L, B, E = q.shape
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o = torch.empty_like(q)
        lse = torch.empty((B * num_heads, lib.usc_attn_lse_stride(L)), dtype=torch.float32, device=q.device)
        check(lib.usc_self_attn_fwd(_ptr(q), _ptr(k), _ptr(v), L, B, num_heads, E, _ptr(o), _ptr(lse), _stream()),
              "usc_self_attn_fwd")
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.num_heads = num_heads
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        L, B, E = q.shape
        do = do.contiguous()
        d3 = torch.empty((3,) + tuple(q.shape), dtype=torch.float32, device=q.device)   # adjacent: the fused projection
        dq, dk, dv = d3[0], d3[1], d3[2]                                                # backward reads them as one table
        check(lib.usc_self_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(do), L, B, ctx.num_heads, E,
                                    _ptr(dq), _ptr(dk), _ptr(dv), _stream()), "usc_self_attn_bwd")
        return dq, dk, dv, None


def self_attention(q, k, v, num_heads):
    """softmax(q k^T / 4) v per head for head dim 16, no mask: q, k, v f32[L,B,E] (sequence-first) with the same
    L <= 256 — the attention core of the decoder's SelfAttentionLayer (reference models/mask3d.py:491-545), one
    launch each way, bit-reproducible."""
    L, B, E = q.shape
    if E != 16 * num_heads or L > ATTN_MAX_QUERIES or k.shape != q.shape or v.shape != q.shape:
        raise RuntimeError(f"self_attention: needs head dim 16, <= {ATTN_MAX_QUERIES} queries and q, k, v of one shape")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"self_attention: {name} must be an f32 HIP tensor")
    return _SelfAttention.apply(q, k, v, num_heads)


def lsap_batch(cost: torch.Tensor):
    """scipy.optimize.linear_sum_assignment of every matrix of cost f32[P, nr, nc] on the device ->
    (row_ind i64[P, m], col_ind i64[P, m], status i32[P]) with m = min(nr, nc); ties resolve like scipy's
    (usc_lsap_batch).  status != 0 marks an infeasible problem (infinite / NaN costs; scipy raises ValueError there) —
    it stays on the device: the caller decides when to look."""
    require_device()
    _chk(cost, torch.float32, "cost")
    if cost.dim() != 3:
        raise RuntimeError("lsap_batch: cost must be f32 [n_problems, nr, nc]")
    P, nr, nc = cost.shape
    m = min(nr, nc)
    row = torch.empty((P, m), dtype=torch.int64, device=cost.device)
    col = torch.empty((P, m), dtype=torch.int64, device=cost.device)
    status = torch.empty(max(P, 1), dtype=torch.int32, device=cost.device)
    check(lib.usc_lsap_batch(_ptr(cost), P, nr, nc, _ptr(row), _ptr(col), _ptr(status), _stream()), "usc_lsap_batch")
    return row, col, status[:P]
