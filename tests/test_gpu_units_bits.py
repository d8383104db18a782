"""GPU: the native unit path (csrc/units.hip, unscene3d_amd/units.py, program.py) returns the bits it returned before its
weight-gradient rule, its table-GEMM plan and its forward frame became one function each.

tests/golden/units_bits.json holds sha256 digests over shape, dtype and bytes of every output of the calls below,
recorded twice on the parent commit's library (both recordings agreed).  No tolerance: the change moved host code only;
each path launches the same kernels in the same order on the same operands and carves its scratch at the same offsets.
If a digest differs, the code is wrong, not the file.

The unit cases are the smallest that reach each branch of units.hip (see `unit_bits`); the trunk cases run the step
program with the lane and its hold schedule, with the lane off and grouped weight gradients, and the per-block path.
Row-order fallback widths: 20 -> 50, the pair every bounds-checked kernel (row-order, pair-list, weight gradient, weight
transpose) is tested at in tests/conv_cases.py; the unit call itself accepts any width >= 1."""
import hashlib
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

from oracle import sparse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "units_bits.json")
SAME, DOWN, UP = 0, 1, 2


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().cpu().contiguous()
        h.update(str(tuple(t.shape)).encode())
        h.update(str(t.dtype).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _scene(voxels, seed):
    from unscene3d_amd.synthetic import make_scene
    sc = make_scene(seed, target_voxels=voxels, tol=0.05)
    ec = R.voxel_floor(sc["xyz"], 0.02)
    eu, _ = R.sparse_quantize(ec)
    return R.sparse_collate([ec[eu]], [sc["colors"][eu]])


def _manager(n, seed, device):
    """Coordinate manager over exactly n voxels of a synthetic scene (the first n of a slightly larger one)."""
    from unscene3d_amd import MinkowskiEngine as ME
    coords4, feats = _scene(int(1.12 * n) + 64, seed)
    assert coords4.shape[0] >= n
    x = ME.SparseTensor(features=torch.from_numpy(feats[:n]).to(device),
                        coordinates=torch.from_numpy(coords4[:n]).to(device), device=device)
    assert x.F.shape[0] == n
    return x.coordinate_manager


def _first_row_count(pred, hi=1 << 22):
    """Smallest n in [1, hi] with pred(n), for a predicate that is a threshold in n."""
    lo = 1
    assert pred(hi) and not pred(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def _bn(c, g, device, training=True):
    bn = torch.nn.BatchNorm1d(c, eps=1e-5, momentum=0.02)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(c, generator=g))
        bn.bias.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
        bn.num_batches_tracked.fill_(7)
    return bn.to(device).train(training)


def _unit(bits, name, device, kmap, kind, cin, cout, seed, residual=True, need_dx=True, dx_acc=False, planes=0,
          modes=("inline", "lane")):
    """One unit forward, then its backward once per mode, on the same seeded inputs:
    inline  no gradient buffers -> dW_accumulate = 0, the weight gradient is issued in the call;
    lane    gradients added in place (non-zero buffers) with the weight-gradient lane on;
    held    as lane, under usc_wgrad_lane_hold with thresholds around the row count, released with mode 0."""
    from unscene3d_amd import ops, units
    from unscene3d_amd._lib import check, lib

    g = torch.Generator().manual_seed(seed)
    K = kmap.K
    n_in, n_out = (kmap.n_out, kmap.n_in) if kind == UP else (kmap.n_in, kmap.n_out)

    def rnd(*shape, scale=1.0):
        return (scale * torch.randn(shape, generator=g)).to(device)

    x = rnd(n_in, cin)
    W = torch.nn.Parameter(rnd(K, cin, cout, scale=1.0 / math.sqrt(K * cin)))
    res = rnd(n_out, cout) if residual else None
    dout, dx0 = rnd(n_out, cout), rnd(n_in, cin)
    gW0, gg0, gb0 = rnd(K, cin, cout), rnd(cout), rnd(cout)
    bn = _bn(cout, g, device)
    W3 = W.detach()
    y, stats, out = units.unit_forward(x, W3, bn, kmap, kind, res, True, None, planes)
    torch.cuda.synchronize()
    bits[f"{name}/fwd"] = _sha(y, stats, out, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    for mode in modes:
        in_place = mode != "inline"
        W.grad = gW0.clone() if in_place else None
        bn.weight.grad = gg0.clone() if in_place else None
        bn.bias.grad = gb0.clone() if in_place else None
        dy = torch.empty_like(y)
        dx = dx0.clone() if (dx_acc and need_dx) else None
        if mode == "held":
            assert units._lane(device) is not None, "the weight-gradient lane is on by default"
            big = max(n_in, n_out)
            check(lib.usc_wgrad_lane_hold(1, big, big // 2, ops._stream()), "usc_wgrad_lane_hold")
        dx, dres, dW, dg, db = units.unit_backward(x, W3, bn, kmap, kind, y, stats, out, dout, dy, residual, dx,
                                                   dx_acc and need_dx, need_dx, W, bn.weight, bn.bias, planes=planes)
        if mode == "held":
            assert lib.usc_wgrad_lane_holding() == 1
            check(lib.usc_wgrad_lane_hold(0, 0, 0, ops._stream()), "usc_wgrad_lane_hold")
        units.join_lane(device)
        torch.cuda.synchronize()
        if in_place:
            assert dW is None and dg is None and db is None
            dW, dg, db = W.grad, bn.weight.grad, bn.bias.grad
        bits[f"{name}/bwd-{mode}"] = _sha(dy, dres, dx, dW, dg, db)


def _unit_bf16(bits, name, device, kmap, kind, cin, cout, seed):
    """The bf16 inference forward (packed weights, running statistics)."""
    from unscene3d_amd import precision, units
    g = torch.Generator().manual_seed(seed)
    n_in, n_out = (kmap.n_out, kmap.n_in) if kind == UP else (kmap.n_in, kmap.n_out)
    x = torch.randn((n_in, cin), generator=g).to(device)
    W3 = (torch.randn((kmap.K, cin, cout), generator=g) / math.sqrt(kmap.K * cin)).to(device)
    res = torch.randn((n_out, cout), generator=g).to(device)
    bn = _bn(cout, g, device, training=False)
    y, stats, out = units.unit_forward(x, W3, bn, kmap, kind, res, True, precision.pack_weights(W3))
    torch.cuda.synchronize()
    bits[f"{name}/fwd-bf16"] = _sha(y, stats, out, bn.running_mean, bn.running_var, bn.num_batches_tracked)


def unit_bits(device):
    """name -> sha256 for the unit calls.  Row counts at the library's own boundaries are read from the library."""
    from unscene3d_amd import units
    from unscene3d_amd._lib import lib

    bits = {}
    both, held = ("inline", "lane"), ("inline", "lane", "held")
    # 700 rows: mask-sorted kernel, tile-form batch norm, split-K slices left behind
    cm = _manager(700, 4101, device)
    cube = cm.kmap_cube(1, 3)
    assert cube.K == 27 and cube.n_out == 700
    _unit(bits, "same27-700-64x64", device, cube, SAME, 64, 64, 1, modes=held)
    _unit(bits, "same27-700-64x64-dxacc", device, cube, SAME, 64, 64, 2, dx_acc=True, modes=both)
    # the stem: stem kernel forward, table-form weight gradient, no input gradient (as in the trunk)
    _unit(bits, "same27-700-3x32-stem", device, cube, SAME, 3, 32, 3, residual=False, need_dx=False, modes=held)
    # widths that are no multiple of 32: row-order fallback, explicit weight transpose
    _unit(bits, "same27-700-20x50", device, cube, SAME, 20, 50, 4, modes=both)
    # identity rows
    _unit(bits, "same1-700-64x128", device, units.kmap_identity(700), SAME, 64, 128, 5, modes=both)
    for P in (2, 3):
        _unit(bits, f"same27-700-64x64-split{P}", device, cube, SAME, 64, 64, 6 + P, planes=P, modes=both)
    _unit_bf16(bits, "same27-700-64x64", device, cube, SAME, 64, 64, 10)
    # just above the tile-form bound: mask-sorted kernel, two-launch batch norm
    n = int(lib.usc_bn_tile_max_rows()) + 1
    cm = _manager(n, 4102, device)
    _unit(bits, "same27-tile+1-32x64", device, cm.kmap_cube(1, 3), SAME, 32, 64, 11, modes=both)
    # the first row count at which the plan names the tile-compacted kernel for 64 input channels
    n = _first_row_count(lambda r: (lib.usc_spconv_plan(0, r, 64, 96, 27) >> 12) & 1) + 1
    assert (lib.usc_spconv_plan(0, n, 96, 64, 27) >> 12) & 1, "the input gradient takes the tile-compacted kernel too"
    cm = _manager(n, 4103, device)
    cube = cm.kmap_cube(1, 3)
    _unit(bits, "same27-compact+1-64x96", device, cube, SAME, 64, 96, 12, modes=both)
    for P in (2, 3):
        _unit(bits, f"same27-compact+1-64x96-split{P}", device, cube, SAME, 64, 96, 13 + P, planes=P, modes=both)
    # one stride-2 map of 2 800 fine rows, both directions
    cm = _manager(2800, 4104, device)
    down = cm.kmap_down(1)
    assert down.K == 8 and down.n_in == 2800
    _unit(bits, "down8-2800-32x64", device, down, DOWN, 32, 64, 17, residual=False, modes=both)
    _unit(bits, "up8-2800-128x64", device, down, UP, 128, 64, 18, residual=False, modes=both)
    _unit(bits, "up8-2800-128x64-dxacc", device, down, UP, 128, 64, 19, residual=False, dx_acc=True, modes=both)
    _unit_bf16(bits, "up8-2800-128x64", device, down, UP, 128, 64, 20)
    return bits


TRUNKS = (("Res16UNet14", 6_000), ("Res16UNet34C", 30_000))


def trunk_bits(device, arch, voxels):
    """name -> sha256 for one forward and backward pass of the trunk: the step program with the lane and the shipped hold
    schedule, the step program with the lane off (weight gradients deferred and grouped inside usc_program_run), and the
    per-block path with the lane off (units.py's own queue)."""
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import program, units
    from unscene3d_amd.models import res16unet

    coords4, feats = _scene(voxels, 4200 + voxels % 89)
    torch.manual_seed(9)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    model = getattr(res16unet, arch)(3, 20, cfg, out_fpn=True).to(device).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    saved = (units.LANE_MAX_ROWS, units.GROUP_WGRAD, program.ENABLED)
    bits = {}
    try:
        for name, lane_rows, prog in (("lane", saved[0], True), ("lane-off-grouped", 0, True), ("lane-off-blocks", 0, False)):
            units.set_lane_max_rows(lane_rows)
            units.GROUP_WGRAD, program.ENABLED = True, prog
            assert (units._lane(device) is not None) == (lane_rows > 0)
            model.load_state_dict(state)
            for p in model.parameters():
                p.grad = torch.zeros_like(p)
            x = ME.SparseTensor(features=torch.from_numpy(feats).to(device),
                                coordinates=torch.from_numpy(coords4).to(device), device=device)
            assert (program.usable(model, x) is not None) == prog
            out, fmaps = model(x)
            loss = sum(w * f.F.square().mean() for w, f in zip((0.5, 1.0, 1.5, 2.0, 0.25), fmaps)) + out.F.abs().mean()
            loss.backward()
            units.flush_deferred_wgrads(device)
            units.join_lane(device)
            torch.cuda.synchronize()
            assert len(fmaps) == 5
            stats = [v for k, v in sorted(model.state_dict().items()) if "running" in k or "num_batches" in k]
            key = f"{arch}-{voxels}/{name}"
            bits[f"{key}/levels"] = _sha(*[f.F for f in fmaps])
            bits[f"{key}/grads"] = _sha(*[p.grad for _, p in sorted(model.named_parameters())])
            bits[f"{key}/running"] = _sha(*stats)
    finally:
        units.GROUP_WGRAD, program.ENABLED = saved[1], saved[2]
        units.set_lane_max_rows(saved[0])
    return bits


def _expect(bits):
    want = json.load(open(GOLDEN))
    assert bits and set(bits) <= set(want), sorted(set(bits) - set(want))
    differ = sorted(k for k in bits if bits[k] != want[k])
    assert not differ, differ


@pytest.mark.gpu
def test_unit_calls_compute_the_recorded_bits(device):
    _expect(unit_bits(device))


@pytest.mark.gpu
@pytest.mark.parametrize("arch,voxels", TRUNKS)
def test_trunk_computes_the_recorded_bits(device, arch, voxels):
    _expect(trunk_bits(device, arch, voxels))


def test_every_recorded_case_is_still_computed():
    """Host side of the pin: the golden file's names are the cases above and nothing else (a case cannot drop out of the
    comparison by being renamed)."""
    want = json.load(open(GOLDEN))
    assert all(len(v) == 64 for v in want.values())
    names = {k.split("/")[0] for k in want}
    assert {f"{a}-{v}" for a, v in TRUNKS} <= names
    assert sum(1 for k in want if "/bwd-held" in k) == 2 and sum(1 for k in want if "/fwd-bf16" in k) == 2
    assert sum(1 for k in want if "split" in k) == 12 and len(want) == 2 * 9 + 46
