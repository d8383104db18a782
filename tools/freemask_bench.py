#!/usr/bin/env python
"""Time and peak memory of the FreeMask voxel-mode pipeline (unscene3d_amd.pseudo_masks.freemask.freemask: bit-packed
masks, no [Q,K] matrix) against a plain-torch-operator restatement of the same steps on the same GPU, which
materialises the f32 [Q,K] similarity, its bool masks, and runs the mask NMS as one `mask @ mask^T` product plus the
same greedy scan (on the host, over the n x n "would kill" matrix).

    python tools/freemask_bench.py                     # (2500, 10000, 96), (2500, 10000, 384) both paths;
                                                       # (10000, 40000, 96) device path only
    python tools/freemask_bench.py --shapes 300,4100,96 --repeats 3
    python tools/freemask_bench.py --mode segment --torch-repeats 5   # segment mode: S = 600 and S = 3200 over 38400 voxels

--mode segment times `freemask_segments` (S-bit rows, device components / split / weighted NMS) against the same
pipeline in torch operators: f32 [S,S] similarity, the connected parts by the float64 restatement's union-find on the
host (tests/freemask_segment_ref.py: the true undirected components, as on the device), f32 and bool [rows, K_voxels]
remapped masks, extent and `mask @ mask^T` NMS on those.  Scenes: a 40 x 40 x 24 voxel grid cut into box segments
(4 x 4 x 4 voxels: S = 600; 2 x 2 x 3: S = 3200), 8 x 8 x 8 objects of `--clusters` feature clusters, so a query's mask
is its cluster's few separate objects.

Per shape and path: median and min / max of `--repeats` timed calls after `--warmup` untimed ones, between two HIP
events on the current stream with a synchronise after the second (both paths read small results back to the host
inside the call, which the events include), and the peak of torch's allocated memory above the inputs.
Features: `--clusters` unit-variance centres + 0.3 noise per channel, 5 % all-zero keys, every cluster's keys inside a
box of a tenth of the scene, so that the extent filter passes them.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PARAMS = dict(hard_mask_threshold=0.35, min_mask_points=10, instance_to_scene_max_ratio=0.8, nms_thr=0.5,
              max_instance_num=50, nms_maskness_threshold=0.6)


def make_inputs(Q, K, C, clusters, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, C))
    lk, lq = rng.integers(0, clusters, K), rng.integers(0, clusters, Q)
    fk = centres[lk] + 0.3 * rng.standard_normal((K, C))
    fq = centres[lq] + 0.3 * rng.standard_normal((Q, C))
    fk[rng.random(K) < 0.05] = 0.0
    corner = rng.integers(0, 360, (clusters, 3))
    coords = corner[lk] + rng.integers(0, 40, (K, 3))
    ext = (coords.max(0) - coords.min(0)).astype(np.float32)
    dev = torch.device("cuda")
    return (torch.from_numpy(fk.astype(np.float32)).to(dev), torch.from_numpy(coords.astype(np.int32)).to(dev),
            torch.from_numpy(fq.astype(np.float32)).to(dev), torch.from_numpy(ext))


def torch_select(masks_of, maskness, carry, coords, ext, instance_to_scene_max_ratio, nms_thr, max_instance_num,
                 nms_maskness_threshold, counts=None):
    """Steps 5-7 of both modes with torch operators.  masks_of() -> bool[n,K] in maskness order (a function, so that the
    unfiltered masks die with the extent filter's copy), maskness f32[n], carry: index tensors [n] that go with the
    rows, counts: the masks' sizes as a table indexed by carry[0] (None: the row sums).
    -> (the survivors' carry, their maskness)."""
    m = masks_of()
    big, c = torch.iinfo(torch.int32).max, coords[:, :2].int()
    ok = torch.ones(len(m), dtype=torch.bool, device=m.device)
    for d in range(2):                                           # [n,K] temporaries, one axis at a time
        hi = torch.where(m, c[:, d][None, :], -big).amax(1)
        lo = torch.where(m, c[:, d][None, :], big).amin(1)
        ok &= ~((hi - lo).double() / float(ext[d]) > instance_to_scene_max_ratio)
    if bool(ok.any()):
        m, maskness, carry = m[ok], maskness[ok], [t[ok] for t in carry]
    mf = m.float()
    inter = mf @ mf.T
    n_i = mf.sum(1) if counts is None else counts[carry[0]].float()
    union = n_i[:, None] + n_i[None, :] - inter
    kill = torch.where(union > 0, inter / union > nms_thr, torch.ones_like(union, dtype=torch.bool)).cpu().numpy()
    dead = np.zeros(len(kill), bool)
    for i in range(len(kill)):
        if not dead[i]:
            dead[i + 1:] |= kill[i, i + 1:]
    maskness = torch.where(torch.from_numpy(~dead).to(m.device), maskness, torch.zeros_like(maskness))
    maskness, by = torch.sort(maskness, descending=True, stable=True)
    by = by[:max_instance_num]
    maskness, carry = maskness[:max_instance_num], [t[by] for t in carry]
    sel = maskness > nms_maskness_threshold
    return [t[sel] for t in carry], maskness[sel]


def torch_freemask(fk, coords, fq, ext, hard_mask_threshold, min_mask_points, instance_to_scene_max_ratio, nms_thr,
                   max_instance_num, nms_maskness_threshold):
    """Steps 1-4 with torch operators, then `torch_select`; [Q,K] in f32 and bool."""
    eps = 1e-9
    kh = fk / (fk.norm(dim=1, keepdim=True) + eps)
    qh = fq / (fq.norm(dim=1, keepdim=True) + eps)
    a = qh @ kh.T
    a -= a.min(-1, keepdim=True)[0]
    a /= a.max(-1, keepdim=True)[0] + eps
    a[:, torch.all(fk == 0, dim=-1)] = 0.0
    masks = a >= hard_mask_threshold
    counts = masks.sum(1)
    cand = torch.nonzero(counts > min_mask_points).flatten()
    if cand.numel() == 0:
        return cand, a.new_zeros(0)
    maskness = (a[cand] * masks[cand]).sum(1) / counts[cand]
    maskness, by = torch.sort(maskness, descending=True, stable=True)
    cand = cand[by]
    (cand,), maskness = torch_select(lambda: masks[cand], maskness, [cand], coords, ext, instance_to_scene_max_ratio,
                                     nms_thr, max_instance_num, nms_maskness_threshold, counts)
    return cand, maskness


def device_freemask(fk, coords, fq, ext, **p):
    from unscene3d_amd.pseudo_masks.freemask import freemask
    soft, maskness, qidx = freemask(fk, coords, fq, ext, **p)
    return qidx, maskness


SEGMENT_PARAMS = dict(hard_mask_threshold=0.35, min_mask_segments=2, min_part_segments=3,
                      instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6)
SEGMENT_SCENES = {"S600": (4, 4, 4), "S3200": (2, 2, 3)}


def make_segment_inputs(box, C, clusters, seed=0):
    """-> (key_feats f32[K,C], key_coords i32[K,3], ids i64[K], connectivity i64[P,2] (one direction per touching pair),
    extent)"""
    rng = np.random.default_rng(seed)
    G = np.array([40, 40, 24])
    g = np.stack(np.meshgrid(*[np.arange(n) for n in G], indexing="ij"), -1).reshape(-1, 3)
    nb = G // np.array(box)
    cell = g // np.array(box)
    seg = (cell[:, 0] * nb[1] + cell[:, 1]) * nb[2] + cell[:, 2]
    obj = g // 8
    cluster_of_obj = rng.integers(0, clusters, (5, 5, 3))
    lk = cluster_of_obj[obj[:, 0], obj[:, 1], obj[:, 2]]
    centres = rng.standard_normal((clusters, C))
    fk = centres[lk] + 0.3 * rng.standard_normal((len(g), C))
    fk[rng.random(len(g)) < 0.05] = 0.0
    grid = seg.reshape(G)
    pairs = [np.stack([np.moveaxis(grid, ax, 0)[:-1].ravel(), np.moveaxis(grid, ax, 0)[1:].ravel()], 1) for ax in range(3)]
    pairs = np.unique(np.concatenate(pairs), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    perm = rng.permutation(len(g))
    ids = (seg * 7 + 3)[perm]
    coords = (g * 2)[perm].astype(np.int32)
    ext = (coords.max(0) - coords.min(0)).astype(np.float32)
    dev = torch.device("cuda")
    return (torch.from_numpy(fk[perm].astype(np.float32)).to(dev), torch.from_numpy(coords).to(dev),
            torch.from_numpy(ids).to(dev), torch.from_numpy(pairs * 7 + 3).to(dev), torch.from_numpy(ext))


def _segment_ref():
    """tests/freemask_segment_ref.py (the float64 restatement: its union-find is the host scan), imported once."""
    if "freemask_segment_ref" not in sys.modules:
        tests = os.path.join(ROOT, "tests")
        if tests not in sys.path:
            sys.path.insert(0, tests)
        import freemask_segment_ref  # noqa: F401
    return sys.modules["freemask_segment_ref"]


def torch_freemask_segments(fk, coords, ids, conn, ext, hard_mask_threshold, min_mask_segments, min_part_segments,
                            instance_to_scene_max_ratio, nms_thr, max_instance_num, nms_maskness_threshold):
    """Segment mode with torch operators and the host union-find; [S,S] and [rows, K] in f32 and bool."""
    SR = _segment_ref()
    eps, dev = 1e-9, fk.device
    uniq, inv = torch.unique(ids, return_inverse=True)
    nz = (fk != 0).any(1)
    sums = torch.zeros((len(uniq), fk.shape[1]), device=dev).index_add_(0, inv[nz], fk[nz])
    feats = sums / torch.bincount(inv[nz], minlength=len(uniq)).clamp(min=1)[:, None]
    valid = (feats != 0).any(1)
    feats, uniq = feats[valid], uniq[valid]
    new_index = torch.cumsum(valid.long(), 0) - 1
    new_index[~valid] = -1
    idx = new_index[inv]
    S = len(uniq)
    h = feats / (feats.norm(dim=1, keepdim=True) + eps)
    a = h @ h.T
    a -= a.min(-1, keepdim=True)[0]
    a /= a.max(-1, keepdim=True)[0] + eps
    masks = a >= hard_mask_threshold
    cand = torch.nonzero(masks.sum(1) > min_mask_segments).flatten()
    none = (cand[:0], cand[:0], a.new_zeros(0))
    if cand.numel() == 0:
        return none
    adj = SR.undirected_adjacency(conn.cpu().numpy(), uniq.cpu().numpy())
    parts, query, root = [], [], []
    for q, m in zip(cand.tolist(), masks[cand].cpu().numpy()):
        label = SR.components(m, adj)
        for r in np.unique(label[label >= 0]):
            part = label == r
            if part.sum() > min_part_segments:
                parts.append(part)
                query.append(q)
                root.append(r)
    if not parts:
        return none
    part = torch.from_numpy(np.array(parts)).to(dev)
    query, root = torch.tensor(query, device=dev), torch.tensor(root, device=dev)
    rows = torch.where(part, a[query], a.new_zeros(()))
    maskness = rows.sum(1) / part.sum(1)
    maskness, by = torch.sort(maskness, descending=True, stable=True)
    rows, query, root = rows[by], query[by], root[by]
    vox = torch.cat([rows, rows.new_zeros((len(rows), 1))], 1)[:, torch.where(idx >= 0, idx, torch.full_like(idx, S))]
    (query, root), maskness = torch_select(lambda: vox >= hard_mask_threshold, maskness, [query, root], coords, ext,
                                           instance_to_scene_max_ratio, nms_thr, max_instance_num, nms_maskness_threshold)
    return uniq[query], uniq[root], maskness


def device_freemask_segments(fk, coords, ids, conn, ext, **p):
    from unscene3d_amd.pseudo_masks.freemask import freemask_segments
    r = freemask_segments(fk, coords, ids, conn, ext, **p)
    return r.query_segment, r.part_root, r.maskness


def measure(fn, args, warmup, repeats, params=PARAMS):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(warmup):
        out = fn(*args, **params)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **params)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, times, peak


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="*", default=["2500,10000,96", "2500,10000,384", "10000,40000,96:device"],
                    help="Q,K,C[:device] — ':device' skips the torch restatement (its [Q,K] buffers)")
    ap.add_argument("--mode", choices=("voxel", "segment"), default="voxel")
    ap.add_argument("--scenes", nargs="*", default=list(SEGMENT_SCENES), help="--mode segment: S600, S3200[:device]")
    ap.add_argument("--channels", type=int, default=96, help="--mode segment: feature channels")
    ap.add_argument("--torch-repeats", type=int, default=None,
                    help="--mode segment: timed calls of the torch path (its host scan takes seconds); default --repeats")
    ap.add_argument("--clusters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("freemask_bench: no HIP device; nothing is measured without one")
    print(f"device: {torch.cuda.get_device_name(0)}; warmup {args.warmup}, repeats {args.repeats}, "
          f"{args.clusters} feature clusters")
    if args.mode == "segment":
        return main_segment(args)
    for spec in args.shapes:
        shape, _, only = spec.partition(":")
        Q, K, C = (int(v) for v in shape.split(","))
        inputs = make_inputs(Q, K, C, args.clusters)
        flop = 2 * 2.0 * Q * K * C                               # the two matrix-core passes
        results = {}
        for name, fn in (("device", device_freemask), ("torch", torch_freemask)):
            if name == "torch" and only == "device":
                continue
            (qidx, maskness), times, peak = measure(fn, inputs, args.warmup, args.repeats)
            results[name] = qidx.cpu().tolist()
            med = statistics.median(times)
            print(f"Q={Q} K={K} C={C} {name:6s}: median {med:9.3f} ms (min {min(times):.3f}, max {max(times):.3f}), "
                  f"peak extra memory {peak / 2**20:9.1f} MiB = {peak / (Q * K):6.3f} x Q*K bytes, "
                  f"{len(qidx)} masks" + (f", two passes = {flop / 1e9:.1f} GFLOP -> {flop / med / 1e9:.2f} TFLOP/s "
                                          "over the whole call" if name == "device" else ""))
        if len(results) == 2:
            print(f"Q={Q} K={K} C={C} survivors agree: {results['device'] == results['torch']}; "
                  f"device first {results['device'][:6]}, torch first {results['torch'][:6]}")
    return 0


def main_segment(args):
    _segment_ref()                                               # outside the timed calls
    for spec in args.scenes:
        scene, _, only = spec.partition(":")
        inputs = make_segment_inputs(SEGMENT_SCENES[scene], args.channels, args.clusters)
        K, S = inputs[0].shape[0], len(torch.unique(inputs[2]))
        results = {}
        for name, fn in (("device", device_freemask_segments), ("torch", torch_freemask_segments)):
            if name == "torch" and only == "device":
                continue
            repeats = args.torch_repeats if name == "torch" and args.torch_repeats else args.repeats
            (query, root, maskness), times, peak = measure(fn, inputs, args.warmup, repeats, SEGMENT_PARAMS)
            results[name] = (list(zip(query.cpu().tolist(), root.cpu().tolist())), maskness.cpu().tolist())
            print(f"segment S={S} K={K} C={args.channels} {name:6s}: median {statistics.median(times):9.3f} ms "
                  f"(min {min(times):.3f}, max {max(times):.3f}; {repeats} calls), peak extra memory {peak / 2**20:9.1f} MiB, "
                  f"{len(query)} masks")
        if len(results) == 2:
            (dp, dm), (tp, tm) = results["device"], results["torch"]
            # the torch side's f32 sums differ in the last bit from run to run, so survivors whose maskness is one
            # ulp apart may swap places there: compare the sets, and the maskness position by position
            close = len(dm) == len(tm) and all(abs(a - b) <= 1e-6 for a, b in zip(dm, tm))
            print(f"segment S={S} K={K} survivors agree: same set {sorted(dp) == sorted(tp)}, same order {dp == tp}, "
                  f"maskness by position within 1e-6 {close}; device first {dp[:4]}, torch first {tp[:4]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
