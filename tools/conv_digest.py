#!/usr/bin/env python
"""sha256 of kernel outputs on fixed inputs: two builds of the library must print the same digests when a change claims
bit-identical results.
    USC3D_LIB=build/ablate/<name>.so python tools/conv_digest.py           the tile-compacted f32 kernel (bench scene's
                                                                           stride-1 / stride-2 maps), with times
    USC3D_LIB=... python tools/conv_digest.py --bf16                       the bf16 matrix-core family (csrc/spconv_bf16.hip):
                                                                           converters, packers, gather-GEMMs, units"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from unscene3d_amd import MinkowskiEngine as ME  # noqa: E402
from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.synthetic import make_scene  # noqa: E402

dev = torch.device("cuda:0")


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous()
        h.update((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def f32_compacted():
    sc = make_scene(2000, target_voxels=150000)
    c3, _, _ = ME.utils.sparse_quantize(sc["xyz"], quantization_size=0.02, return_index=True, return_inverse=True, device="cuda:0")
    coords = torch.cat([torch.zeros((c3.shape[0], 1), dtype=torch.int32, device=dev), c3], 1).contiguous()
    x = ME.SparseTensor(features=torch.zeros(coords.shape[0], 3, device=dev), coordinates=coords, device=dev)
    cm = x.coordinate_manager
    cm.stride_map(1)
    for ts, (cin, cout) in ((1, (96, 96)), (1, (128, 96)), (1, (96, 128)), (2, (96, 96))):
        n = cm.coord_map(ts).n
        nbr = cm.cube_map(ts)["nbr"]
        g = torch.Generator(device="cpu").manual_seed(ts * 1000 + cin + cout)
        xin = torch.randn(n, cin, generator=g).to(dev)
        W = (torch.randn(27, cin, cout, generator=g) * 0.05).to(dev)
        out = ops.gather_gemm(xin, W, nbr, n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.gather_gemm(xin, W, nbr, n)
        e1.record()
        torch.cuda.synchronize()
        print(f"stride {ts} rows {n} {cin}->{cout}: sha256 {sha(out)}  {e0.elapsed_time(e1) * 100:.1f} us per launch")


def _table(n, seed):
    """i32[27, n] of a random voxel cluster followed by isolated voxels that fill the last 256-row block (n is not a
    multiple of 256): rows with missing neighbours, and a ragged block in which every offset but the centre is absent."""
    from oracle import sparse_ref as R
    rng = np.random.default_rng(seed)
    n_iso = n - (n - 1) // 256 * 256
    n_dense = n - n_iso
    side = int(np.ceil((n_dense / 0.3) ** (1 / 3)))
    cells = rng.choice(side ** 3, size=n_dense, replace=False)
    dense = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1)
    iso = np.stack([np.full(n_iso, 1000), 5 * np.arange(n_iso), np.zeros(n_iso, np.int64)], 1)
    coords4 = np.concatenate([np.zeros((n, 1), np.int64), np.concatenate([dense, iso], 0)], 1).astype(np.int32)
    nbr = R.kernel_map_cube(coords4, 1, 3).astype(np.int32)
    has = (nbr >= 0).sum(0)
    assert n % 256 and has.min() < 27 and has.max() > 1 and ((nbr[:, -n_iso:] >= 0).sum(1) == 0).any()
    return nbr


def _unit_scene(n, seed):
    rng = np.random.default_rng(seed)
    side = 13
    cells = rng.choice(side ** 3, size=n, replace=False)
    xyz = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1)
    coords4 = np.concatenate([np.zeros((n, 1), np.int64), xyz], 1).astype(np.int32)
    st = ME.SparseTensor(features=torch.zeros((n, 3), device=dev), coordinates=torch.from_numpy(coords4).to(dev), device=dev)
    return st.coordinate_manager, st._ts()


def _bn(cout, g, training):
    bn = torch.nn.BatchNorm1d(cout, momentum=0.02).to(dev).train(training)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    return bn


def _split_program(x, W, bn, kmap, res, dout, planes):
    """One stride-1 unit, forward then backward, as a two-step program (usc_program_run) in split precision."""
    import ctypes as C

    from unscene3d_amd import units
    from unscene3d_amd._lib import STEP_UNIT_BWD, STEP_UNIT_FWD, Step, check, lib
    n, cin = x.shape
    cout = W.shape[2]
    new = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    y, out, stats, dy, dres, dx = new(n, cout), new(n, cout), new(4, cout), new(n, cout), new(n, cout), new(n, cin)
    dW, dg, db = new(*W.shape), new(cout), new(cout)
    bdesc, _ = units._bn_desc(bn, True)
    steps = (Step * 2)()
    for st, op in zip(steps, (STEP_UNIT_FWD, STEP_UNIT_BWD)):
        st.op, st.kind, st.cin, st.cout, st.relu, st.split_planes = op, units.SAME, cin, cout, 1, planes
        st.map, st.bn = C.addressof(kmap.struct), C.addressof(bdesc)
        st.x, st.W, st.y, st.stats, st.out = x.data_ptr(), W.data_ptr(), y.data_ptr(), stats.data_ptr(), out.data_ptr()
        st.residual = res.data_ptr()
    b = steps[1]
    b.dout, b.dy, b.dres, b.dx = dout.data_ptr(), dy.data_ptr(), dres.data_ptr(), dx.data_ptr()
    b.dW, b.dgamma, b.dbeta = dW.data_ptr(), dg.data_ptr(), db.data_ptr()
    ws = units.workspace(lib.usc_program_ws_bytes(steps, 2), dev)
    check(lib.usc_program_run(steps, 0, 1, ws.data_ptr(), ws.numel(), ops._stream()), "usc_program_run")
    check(lib.usc_program_run(steps, 1, 2, ws.data_ptr(), ws.numel(), ops._stream()), "usc_program_run")
    torch.cuda.synchronize()
    return y, stats, out, dy, dres, dx, dW, dg, db


def bf16_family():
    from unscene3d_amd import precision, units
    g = torch.Generator(device="cpu").manual_seed(20)
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-40, 3.4e38, 1.0 + 2.0 ** -8,
                            1.0 + 3 * 2.0 ** -8, -1.5, 1.0 + 2.0 ** -9 + 2.0 ** -18])
    # converters: 4k + {0..3} elements (vector body / tail), rows of a width that is and is not a multiple of 4
    for n in (1024, 1025, 1026, 1027, 3):
        a = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
        a[:min(n, special.numel())] = special[:n]
        print(f"cast_bf16 n={n}: {sha(ops.cast_bf16(a.to(dev)))}")
        for P in (2, 3):
            print(f"split_bf16 P={P} n={n}: {sha(ops.split_bf16(a.to(dev), P))}")
    for rows, c in ((37, 48), (37, 50), (5, 7)):
        a = torch.randn((rows, c), generator=g)
        a[1, 3], a[4, 6] = float("inf"), 1e-40
        for P in (2, 3):
            print(f"split_bf16 P={P} rows={rows} c={c}: {sha(ops.split_bf16(a.to(dev), P))}")
    # packers
    for K, cin, cout in ((1, 16, 32), (27, 48, 96), (8, 96, 64), (27, 32, 32)):
        W = torch.randn((K, cin, cout), generator=g).to(dev)
        print(f"pack_weights K={K} {cin}->{cout}: {sha(precision.pack_weights(W))}")
        for P in (2, 3):
            print(f"pack_w_split P={P} K={K} {cin}->{cout}: {sha(ops.pack_w_split(W, P))}")
            if cin % 32 == 0 and cout % 16 == 0:
                print(f"pack_w_split P={P} K={K} {cin}->{cout} transposed: {sha(ops.pack_w_split(W, P, transposed=True))}")
    # gather-GEMMs: every CT (cout 96 / 64 / 32), K = 27 over the table and the K = 1 identity form, bias + accumulate
    n = 700
    nbr_all = torch.from_numpy(_table(n, 800)).to(dev)
    for cin, cout in ((48, 32), (96, 64), (80, 96), (16, 160)):
        for K in (27, 1):
            nbr = nbr_all if K == 27 else None
            x = torch.randn((n, cin), generator=g).to(dev)
            W = (torch.randn((K, cin, cout), generator=g) / (K * cin) ** 0.5).to(dev)
            bias, acc = torch.randn(cout, generator=g).to(dev), torch.randn((n, cout), generator=g).to(dev)
            for P in (1, 2, 3):
                if P == 1:
                    xs, Wp, gemm = ops.cast_bf16(x), precision.pack_weights(W), ops.gather_gemm_bf16
                else:
                    xs, Wp, gemm = ops.split_bf16(x, P), ops.pack_w_split(W, P), ops.gather_gemm_split
                y = gemm(xs, Wp, K, cout, nbr, n)
                y2 = acc.clone()
                gemm(xs, Wp, K, cout, nbr, n, bias=bias, out=y2, accumulate=True)
                print(f"gather_gemm P={P} K={K} {cin}->{cout}: {sha(y)}  bias+accumulate {sha(y2)}")
    # units: the bf16 forward of all three kinds (batch and running statistics), the split unit through usc_program_run
    cm, ts = _unit_scene(n, 31)
    same, down = cm.kmap_cube(ts, 3), cm.kmap_down(ts)
    for kind, kmap, tag in ((units.SAME, same, "same"), (units.DOWN, down, "down"), (units.UP, down, "up")):
        for cin, cout, training in ((96, 96, True), (32, 64, False)):
            n_in = kmap.n_out if kind == units.UP else kmap.n_in
            n_out = kmap.n_in if kind == units.UP else kmap.n_out
            x = torch.randn((n_in, cin), generator=g).to(dev)
            W = (torch.randn((kmap.K, cin, cout), generator=g) / (kmap.K * cin) ** 0.5).to(dev)
            res = torch.randn((n_out, cout), generator=g).to(dev)
            bn = _bn(cout, g, training)
            with torch.no_grad():
                r = units.unit_forward(x, W, bn, kmap, kind, res, True, precision.pack_weights(W))
            print(f"unit bf16 {tag} {cin}->{cout} {'train' if training else 'eval'}: {sha(*r)} "
                  f"running {sha(bn.running_mean, bn.running_var)}")
    for cin, cout in ((96, 96), (48, 96)):
        x = torch.randn((n, cin), generator=g).to(dev)
        W = (torch.randn((27, cin, cout), generator=g) / (27 * cin) ** 0.5).to(dev)
        res, dout = torch.randn((n, cout), generator=g).to(dev), torch.randn((n, cout), generator=g).to(dev)
        for P in (2, 3):
            bn = _bn(cout, g, True)
            r = _split_program(x, W, bn, same, res, dout, P)
            print(f"unit split P={P} {cin}->{cout} program: forward {sha(*r[:3])} backward {sha(*r[3:])}")
            bn.eval()
            with torch.no_grad():
                e = units.unit_forward(x, W, bn, same, units.SAME, None, False, None, P)
            print(f"unit split P={P} {cin}->{cout} eval forward: {sha(*e)}")


if __name__ == "__main__":
    bf16_family() if "--bf16" in sys.argv[1:] else f32_compacted()
