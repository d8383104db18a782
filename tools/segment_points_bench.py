"""The point-cloud over-segmentation (`felzenszwalb_cpp.segment_points`, csrc/felz_points.hip) at scan
sizes, against the host route to the same graph.

    python tools/segment_points_bench.py [--points 200000 1000000] [--calls 7] [--out profiles/felz_points.txt]

Workload: tools/normals_bench.py's synthetic room (floor, ceiling, walls, six boxes on jittered grids) at about 200 k and
1 M points, colours that follow position in steps, normals estimated once on the device and then GIVEN (oriented weights,
the mode of a file that carries normals); k = 8, radius = 0.1, kthr 0.005, segMinVerts 50.
Device, host clock around work that ends in a device synchronise, after 2 warm-ups, median (min ... max) over --calls:
    graph      ops.knn_hybrid(k + 1) + knn_edges (one read-back of the edge total) + point_edge_weights + stable sort
    segment    the whole segment_points: graph, one device-to-host copy, the host merge, relabel
    estimated  segment_points(normals=None): the same plus ops.estimate_normals, unoriented weights
Host, 16 threads: scipy.spatial.cKDTree(points).query(points, k + 1, distance_upper_bound=radius, workers=16) and the
oriented weights of all directed pairs in numpy float32 (tree build timed apart; no deduplication, no sort, no merge: the
host column is the graph's raw material only, so the comparison favours it).
Also recorded: edges, share of full rows, segments found."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from normals_bench import alternate, fmt, synthetic_room, wall_ms  # noqa: E402
from unscene3d_amd import felzenszwalb_cpp as felz  # noqa: E402
from unscene3d_amd import ops  # noqa: E402

K, RADIUS, KTHR, MIN_VERTS, HOST_THREADS = 8, 0.1, 0.005, 50, 16


def host_weights(P, C, N, idx, found):
    """Oriented Felzenszwalb weights of the directed pairs (row, idx[row, p]) in float32 -> f32[n, k+1] (0 where not found)."""
    b = np.where(found, idx, 0)
    n1, n2 = N[:, None, :], N[b]
    dot = (n1 * n2).sum(-1)
    cd = np.abs(C[:, None, :] - C[b]).sum(-1)
    w = (np.float32(1) - dot) * cd
    d = P[b] - P[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        along = (n2 * d).sum(-1) / np.sqrt((d * d).sum(-1))
    w = np.where((along > 0) & (cd < 0.05), w * w, w)
    return np.where(found, w, np.float32(0))


def measure(n_target, calls, dev):
    from scipy.spatial import cKDTree

    pts = synthetic_room(n_target)
    n = pts.shape[0]
    colors = (np.floor(pts * 2.0) % 4 / 4.0 + 0.1).astype(np.float32)        # 0.5 m blocks of one colour
    p, c = torch.from_numpy(pts).to(dev), torch.from_numpy(colors).to(dev)
    normals = ops.estimate_normals(p)
    state = {}

    def graph():
        idx, count = ops.knn_hybrid(p, p, K + 1, RADIUS)
        ea, eb = felz.knn_edges(idx, count, check_range=False)
        w = felz.point_edge_weights(p, c, normals, ea, eb, oriented=True)
        state["order"] = torch.sort(w, stable=True).indices
        state["edges"], state["full"] = ea.shape[0], float((count == K + 1).float().mean())
        torch.cuda.synchronize()

    def segment():
        state["labels"] = felz.segment_points(p, c, normals, K, RADIUS, KTHR, MIN_VERTS, device=dev)[0]

    def estimated():
        state["labels_est"] = felz.segment_points(p, c, None, K, RADIUS, KTHR, MIN_VERTS, device=dev)[0]

    ms = alternate([("graph", graph, wall_ms), ("segment", segment, wall_ms), ("estimated", estimated, wall_ms)], calls, warmup=2)
    lines = [f"{n} points: {state['edges']} edges ({state['edges'] / n:.2f} per point), rows with all {K + 1} places filled "
             f"{state['full'] * 100:.1f} %, segments {int(state['labels'].max()) + 1} (given normals) / "
             f"{int(state['labels_est'].max()) + 1} (estimated normals)",
             "  device (host clock, ends in a synchronise):"]
    lines += [f"    {k:12s}{fmt(v)}" for k, v in ms.items()]

    P, C, N = pts, colors, normals.cpu().numpy()
    t0 = wall_ms(lambda: state.update(tree=cKDTree(P.astype(np.float64))))
    points64 = P.astype(np.float64)

    def search():
        d, i = state["tree"].query(points64, k=K + 1, distance_upper_bound=RADIUS, workers=HOST_THREADS)
        state["idx"], state["found"] = i, np.isfinite(d) & (i != np.arange(n)[:, None])

    def weights():
        state["w"] = host_weights(P, C, N, state["idx"], state["found"])

    torch.set_num_threads(HOST_THREADS)
    hs = alternate([("search", search, wall_ms), ("weights", weights, wall_ms)], max(3, calls // 2), warmup=1)
    hs["total"] = [s + q for s, q in zip(hs["search"], hs["weights"])]
    lines.append(f"  host ({HOST_THREADS} threads: cKDTree.query(k={K + 1}, distance_upper_bound={RADIUS}) + numpy float32 weights of "
                 f"the directed pairs; tree build, once: {t0:.1f} ms, not in the total):")
    lines += [f"    {k:12s}{fmt(v)}" for k, v in hs.items()]
    lines.append(f"  host total / device graph (medians): {np.median(hs['total']) / np.median(ms['graph']):.1f}; "
                 f"share of segment_points spent after the graph (copy, host merge, relabel): "
                 f"{(1 - np.median(ms['graph']) / np.median(ms['segment'])) * 100:.0f} %")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segment_points_bench.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    from unscene3d_amd import _lib

    lines = [f"tools/segment_points_bench.py --points {' '.join(map(str, a.points))} --calls {a.calls}; "
             f"{torch.cuda.get_device_name(0)}; library: {_lib.lib.usc_build_info().decode()}",
             f"k = {K}, radius = {RADIUS}, kthr = {KTHR}, segMinVerts = {MIN_VERTS}; median (min ... max)"]
    for n in a.points:
        lines += measure(n, a.calls, dev)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
