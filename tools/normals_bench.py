"""Normals estimated from a point cloud on the device (`ops.knn_hybrid` + `ops.normals_pca`, csrc/normals.hip) against the
host route they replace (a k-d tree search and a batched eigen solve), at the shape of the mesh-only dataset builder.

    python tools/normals_bench.py [--calls 15] [--out profiles/normals_hybrid.txt]

Workload: a synthetic room of about 200 k mesh vertices — floor, ceiling, four walls and six boxes, each a jittered grid
of vertices at one spacing, 1 mm of noise off the plane — radius 0.1, 30 neighbours, cell = radius.
Device: search (binning included; the caller gives the box), PCA, and total (`ops.estimate_normals`: both, with the
read-back of the box in between), each between HIP events after 3 warm-ups: median (min ... max) over `--calls` repeats;
the three run one after the other inside every repeat.
Host, 16 threads: `scipy.spatial.cKDTree(points).query(points, k=30, distance_upper_bound=0.1, workers=16)` (the tree
build timed apart) and `numpy.linalg.eigh` on the stacked 3x3 covariances, same protocol, host clock.
Also recorded: points per occupied cell, the share of queries that fill all 30 places, and the largest angle between the
two routes' normals over the points whose two smallest eigenvalues are apart (as tests/test_gpu_normals.py leaves out
the others)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unscene3d_amd import ops  # noqa: E402

RADIUS, MAX_NN, HOST_THREADS = 0.1, 30, 16


def synthetic_room(n_target=200_000, seed=0):
    """-> f32[N,3], N about n_target: rectangles of a 6 x 5 x 2.7 m room and six boxes, sampled on jittered grids."""
    rng = np.random.default_rng(seed)
    rects = [((0, 0, 0), (6, 0, 0), (0, 5, 0)), ((0, 0, 2.7), (6, 0, 0), (0, 5, 0)),
             ((0, 0, 0), (6, 0, 0), (0, 0, 2.7)), ((0, 5, 0), (6, 0, 0), (0, 0, 2.7)),
             ((0, 0, 0), (0, 5, 0), (0, 0, 2.7)), ((6, 0, 0), (0, 5, 0), (0, 0, 2.7))]
    for _ in range(6):
        x, y = rng.random() * 4.5 + 0.2, rng.random() * 3.5 + 0.2
        a, b, h = rng.random(3) * 0.8 + 0.4
        rects += [((x, y, h), (a, 0, 0), (0, b, 0)), ((x, y, 0), (a, 0, 0), (0, 0, h)), ((x, y + b, 0), (a, 0, 0), (0, 0, h)),
                  ((x, y, 0), (0, b, 0), (0, 0, h)), ((x + a, y, 0), (0, b, 0), (0, 0, h))]
    area = sum(np.linalg.norm(np.cross(u, v)) for _, u, v in rects)
    h = np.sqrt(area / n_target)
    parts = []
    for o, u, v in rects:
        lu, lv = np.linalg.norm(u), np.linalg.norm(v)
        nu, nv = max(2, int(round(lu / h))), max(2, int(round(lv / h)))
        s, t = np.meshgrid((np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv, indexing="ij")
        s = s + rng.uniform(-0.3, 0.3, s.shape) / nu
        t = t + rng.uniform(-0.3, 0.3, t.shape) / nv
        p = np.asarray(o, float) + s[..., None] * np.asarray(u, float) + t[..., None] * np.asarray(v, float)
        parts.append(p.reshape(-1, 3) + rng.normal(0, 0.001, (nu * nv, 3)))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
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
    return f"{np.median(v):10.3f} ms ({min(v):.3f} ... {max(v):.3f})"


def host_route(points64):
    """-> (search fn, pca fn, state): the two host stages as closures over shared state."""
    from scipy.spatial import cKDTree

    state = {"tree": cKDTree(points64)}

    def search():
        d, i = state["tree"].query(points64, k=MAX_NN, distance_upper_bound=RADIUS, workers=HOST_THREADS)
        state["idx"], state["found"] = i, np.isfinite(d)

    def pca():
        i, found = state["idx"], state["found"]
        x = points64[np.where(found, i, 0)] - points64[:, None, :]           # a missing neighbour: index n, masked out
        w = found[..., None].astype(np.float64)
        m = np.maximum(found.sum(1), 1)[:, None]
        c = (x - (x * w).sum(1, keepdims=True) / m[..., None]) * w
        lam, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c) / m[..., None])
        state["normals"], state["lam"], state["count"] = vec[:, :, 0], lam, found.sum(1)

    return search, pca, state


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from unscene3d_amd import _lib

    pts = synthetic_room(a.points)
    n = pts.shape[0]
    p = torch.from_numpy(pts).to(dev)
    lo, hi = pts.min(0), pts.max(0)
    origin, cell, dims = ops.knn1_grid_plan(lo, hi, n, RADIUS)
    cid = np.floor((pts.astype(np.float64) - origin) / cell).astype(np.int64)
    occupied = np.unique((cid[:, 0] * int(dims[1]) + cid[:, 1]) * int(dims[2]) + cid[:, 2]).size
    idx, count = ops.knn_hybrid(p, p, MAX_NN, RADIUS, bounds=(lo, hi))
    lines = [f"tools/normals_bench.py --calls {a.calls} --points {a.points}; {torch.cuda.get_device_name(0)}; "
             f"library: {_lib.lib.usc_build_info().decode()}",
             f"synthetic room: {n} points, radius {RADIUS}, max_nn {MAX_NN}; cell = {cell:.5g}, grid {dims[0]} x {dims[1]} x "
             f"{dims[2]} = {int(dims.prod())} cells, {occupied} occupied, {n / occupied:.1f} points per occupied cell, "
             f"workspace {ops.lib.usc_knn_hybrid_grid_ws_bytes(n, dims.ctypes.data) / 2 ** 20:.1f} MiB",
             f"queries that fill all {MAX_NN} places: {float((count == MAX_NN).float().mean()) * 100:.1f} %; with fewer than 3 "
             f"neighbours: {int((count < 3).sum())}; mean neighbours listed {float(count.float().mean()):.1f}"]
    ms = alternate([("search", lambda: ops.knn_hybrid(p, p, MAX_NN, RADIUS, bounds=(lo, hi)), event_ms),
                    ("pca", lambda: ops.normals_pca(p, p, idx, count), event_ms),
                    ("total", lambda: ops.estimate_normals(p, RADIUS, MAX_NN), event_ms)], a.calls)
    lines.append("device, between HIP events (search is given the box; total = ops.estimate_normals, which reads the box back):")
    lines += [f"  {k:14s}{fmt(v)}" for k, v in ms.items()]

    points64 = pts.astype(np.float64)
    t0 = time.perf_counter()
    search, pca, state = host_route(points64)
    build_ms = (time.perf_counter() - t0) * 1e3
    hs = alternate([("search", search, wall_ms), ("pca", pca, wall_ms)], a.calls)
    hs["total"] = [s + q for s, q in zip(hs["search"], hs["pca"])]
    lines.append(f"host ({HOST_THREADS} threads: cKDTree.query(k={MAX_NN}, distance_upper_bound={RADIUS}, workers={HOST_THREADS}) + "
                 f"batched numpy.linalg.eigh; tree build, once: {build_ms:.1f} ms, not in the total):")
    lines += [f"  {k:14s}{fmt(v)}" for k, v in hs.items()]
    lines.append(f"host total / device total (medians): {np.median(hs['total']) / np.median(ms['total']):.1f}")

    got = ops.estimate_normals(p, RADIUS, MAX_NN).cpu().numpy().astype(np.float64)
    lam, ref = state["lam"], state["normals"]
    same_count = bool(np.array_equal(state["count"], count.cpu().numpy()))
    keep = (state["count"] >= 3) & (lam[:, 1] - lam[:, 0] >= 2.0 ** -20 * lam.sum(1))
    theta = np.arctan2(np.linalg.norm(np.cross(got[keep], ref[keep]), axis=1), np.abs((got[keep] * ref[keep]).sum(1)))
    lines.append(f"neighbour counts equal on both routes: {same_count}; largest angle between the routes' normals over "
                 f"{int(keep.sum())} points with separated eigenvalues: {theta.max():.3e} rad")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
