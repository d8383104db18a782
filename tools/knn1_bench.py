"""Exact 1-NN at the shapes this package runs: the brute-force kernel (`ops.knn1`, every pair in f64) against the grid
kernel (`ops.knn1_grid`), and the 3D branch of the scan builder (backbone forward + lift) with either.

    python tools/knn1_bench.py [--calls 15] [--out profiles/knn1_grid.txt]

Shapes, all from one synthetic 150 k-voxel room (unscene3d_amd.synthetic.make_scene):
  builder     the scene's integer voxels against the voxels of their stride-2 level, taken from the coordinate manager:
              what `encode_scene_feats_3d(resolution_scale=2)` searches; cell = the stride, as `nn="grid"` sets it
  segment     150 k surface points against 160 k other surface points, metres (points against mesh vertices); default cell
  save-time   240 k surface points, in voxel units, against the 150 k voxel centres (`masks_to_full_resolution`); default cell
Per shape the variants run one after the other inside every repeat (so drift hits all alike), each between HIP events
after 3 warm-ups: median (min ... max) over `--calls` repeats.  `grid` gets the reference box from the caller, `grid +
read-back` finds it with one aminmax and a host copy, `grid build only` is the call with no query (binning alone),
`bounds read-back` that aminmax and copy alone (host clock around a synchronise: it is host time).  The outputs of the two
kernels are compared index for index and bit for bit at every shape."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unscene3d_amd import MinkowskiEngine as ME  # noqa: E402
from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.synthetic import make_scene  # noqa: E402

VOXEL = 0.02


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, calls, warmup=3):
    """variants: [(name, fn, clock)] -> {name: [ms]}; every repeat runs each variant once, in order."""
    for _ in range(warmup):
        for _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(calls):
        for name, fn, clock in variants:
            ms[name].append(clock(fn))
    return ms


def fmt(v):
    return f"{np.median(v):9.3f} ms ({min(v):.3f} ... {max(v):.3f})"


def bounds_of(ref):
    lo, hi = torch.aminmax(ref, dim=0)
    return torch.stack([lo, hi]).cpu().numpy()


def bench_shape(name, query, ref, cell, calls):
    nq, nr = query.shape[0], ref.shape[0]
    lo, hi = bounds_of(ref)
    origin, used, dims = ops.knn1_grid_plan(lo, hi, nr, cell)
    cid = torch.floor((ref.double() - torch.from_numpy(origin).to(ref.device)) / used).long()
    occupied = torch.unique((cid[:, 0] * int(dims[1]) + cid[:, 1]) * int(dims[2]) + cid[:, 2]).numel()
    ws = ops.lib.usc_knn1_grid_ws_bytes(nr, dims.ctypes.data)
    empty = query[:0]
    variants = [("brute force", lambda: ops.knn1(query, ref), event_ms),
                ("grid", lambda: ops.knn1_grid(query, ref, cell=cell, bounds=(lo, hi)), event_ms),
                ("grid + read-back", lambda: ops.knn1_grid(query, ref, cell=cell), host_ms),
                ("grid build only", lambda: ops.knn1_grid(empty, ref, cell=cell, bounds=(lo, hi)), event_ms),
                ("bounds read-back", lambda: bounds_of(ref), host_ms)]
    ms = alternate(variants, calls)
    d_b, i_b = ops.knn1(query, ref)
    d_g, i_g = ops.knn1_grid(query, ref, cell=cell, bounds=(lo, hi))
    same = bool(torch.equal(i_b, i_g)) and bool(torch.equal(d_b.view(torch.int32), d_g.view(torch.int32)))
    lines = [f"{name}: nq = {nq}, nr = {nr} ({nq * nr:.2e} pairs); cell = {used:.5g}"
             f"{' (default)' if cell is None else ''}, grid {dims[0]} x {dims[1]} x {dims[2]} = {int(dims.prod())} cells, "
             f"{occupied} occupied, {nr / occupied:.2f} points per occupied cell, workspace {ws / 2 ** 20:.1f} MiB; "
             f"outputs equal: {same}"]
    lines += [f"  {n:18s}{fmt(v)}" for n, v in ms.items()]
    b, g = ms["brute force"], ms["grid"]
    lines.append(f"  brute / grid = {np.median(b) / np.median(g):.1f}; brute-force spread (max - min) "
                 f"{max(b) - min(b):.3f} ms, median difference {np.median(b) - np.median(g):.3f} ms")
    if not same:
        raise SystemExit("\n".join(lines) + "\nthe two kernels disagree")
    return lines, ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from unscene3d_amd import _lib
    from unscene3d_amd.models.res16unet import Res16UNet34CMultiRes
    from unscene3d_amd.pseudo_masks.pipeline import encode_scene_feats_3d

    lines = [f"tools/knn1_bench.py --calls {a.calls}; {torch.cuda.get_device_name(0)}; "
             f"library: {_lib.lib.usc_build_info().decode()}"]
    sc = make_scene(1000, target_voxels=150_000)
    xyz = sc["xyz"]
    vox = np.floor(xyz / VOXEL).astype(np.int64)
    _, first = np.unique(vox, axis=0, return_index=True)
    first.sort()
    coords = np.concatenate([np.zeros((first.shape[0], 1), np.int32), vox[first].astype(np.int32)], 1)
    colors = torch.from_numpy(sc["colors"][first].astype(np.float32)).to(dev)

    def sinput():
        return ME.SparseTensor(features=colors, coordinates=torch.from_numpy(coords).to(dev), device=dev)

    x = sinput()
    x.coordinate_manager.stride_map(1)
    fine = x.C[:, 1:].float().contiguous()
    coarse = x.coordinate_manager.coord_map(2).coords[:, 1:].float().contiguous()
    rng = np.random.default_rng(0)
    pick = rng.permutation(xyz.shape[0])
    assert xyz.shape[0] >= 310_000, xyz.shape
    surf = torch.from_numpy(xyz.astype(np.float32)).to(dev)
    pick = torch.from_numpy(pick).to(dev)
    seg_q, seg_r = surf[pick[:150_000]].contiguous(), surf[pick[150_000:310_000]].contiguous()
    save_q = (surf[pick[:240_000]] / VOXEL).contiguous()
    save_r = (fine + 0.5).contiguous()

    builder_ms = None
    for name, q, r, cell in (("builder", fine, coarse, 2.0), ("segment lift", seg_q, seg_r, None),
                             ("save-time lift", save_q, save_r, None)):
        out, ms = bench_shape(name, q, r, cell, a.calls)
        lines += out
        builder_ms = builder_ms or ms

    # the 3D branch of build_scene on this scene: forward of the frozen backbone + the lift, one box only
    torch.manual_seed(0)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    model = Res16UNet34CMultiRes(3, 20, cfg).to(dev).eval()
    ms = alternate([("forward + brute lift", lambda: encode_scene_feats_3d(model, sinput(), nn="brute"), host_ms),
                    ("forward + grid lift", lambda: encode_scene_feats_3d(model, sinput(), nn="grid"), host_ms)],
                   max(3, a.calls // 3), warmup=2)
    same = bool(torch.equal(encode_scene_feats_3d(model, sinput(), nn="brute"),
                            encode_scene_feats_3d(model, sinput(), nn="grid")))
    lines.append(f"3D branch, {coords.shape[0]} voxels, Res16UNet34CMultiRes f32, seeded weights (host clock around a "
                 f"synchronise, SparseTensor construction included); features equal: {same}")
    lines += [f"  {n:22s}{fmt(v)}" for n, v in ms.items()]
    b, g = builder_ms["brute force"], builder_ms["grid"]
    faster = np.median(b) - np.median(g) > max(b) - min(b)
    lines.append(f"builder shape: the grid kernel is {'FASTER' if faster else 'NOT faster'} than brute force by more than "
                 f"the spread of the brute-force repeats -> build_scene's lift: nn=\"{'grid' if faster else 'brute'}\"")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
