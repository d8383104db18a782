"""Seeded cases of the batched DBSCAN split (ops.dbscan_masks, postprocess.dbscan_split_batched): f32 coordinates
[N,3] and mask logits [N,Q] (a point is on where the logit is > 0), the (eps, min_samples) pairs they are run with,
and sklearn's labels for them.

Every case keeps out of the band |d - eps| <= 1e-6 eps for every pair of points and every eps of PARAMS (d in f64 on
the f32 coordinates): sklearn treats f32 input in f32 and f64 input in f64, and the kernels compare against the f32
eps squared in f64, so inside the band the reference is not defined by its text.  `band_pairs` counts the pairs in
it (test_dbscan_host.py asserts zero); the seeds below were picked so that it is empty.  sklearn always gets f64
copies of the f32 coordinates."""
import functools

import numpy as np

PARAMS = ((0.95, 1), (0.21, 1), (0.3, 4), (0.3, 10))
BAND = 1e-6


def band_pairs(xyz, eps, chunk=512):
    """Number of point pairs with |d - eps| <= BAND * eps."""
    x = np.asarray(xyz, np.float64)
    n = 0
    for i in range(0, len(x), chunk):
        d = np.sqrt(((x[i:i + chunk, None, :] - x[None, :, :]) ** 2).sum(-1))
        n += int((np.abs(d - eps) <= BAND * eps).sum())
    return n // 2 if eps > 0 else n


def _logits(rng, on):
    """Random logits with the given sign pattern, never zero."""
    mag = rng.uniform(0.1, 6.0, on.shape).astype(np.float32)
    return np.where(on, mag, -mag).astype(np.float32)


def _tiny():
    return np.array([[0.3, -1.2, 2.0]], np.float32), np.array([[2.5]], np.float32)


def _wide(seed=3):
    """Q = 65 (one more than a 64-bit word) on 131 points: query 0 empty, query 1 all on, the rest random."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.5, 1.5, (5, 3))
    xyz = (centres[rng.integers(0, 5, 131)] + rng.normal(0, 0.12, (131, 3))).astype(np.float32)
    on = rng.random((131, 65)) < rng.uniform(0.2, 0.9, 65)
    on[:, 0] = False
    on[:, 1] = True
    return xyz, _logits(rng, on)


def _blobs(seed=11):
    """2111 points (not a multiple of 64) around the origin: Gaussian blobs, isolated points, exact duplicates.
    Queries: 0 empty, 1 all on, 2 only far-apart points (all noise at min_samples = 10: no column), 3-7 unions of
    blobs with points dropped at random."""
    rng = np.random.default_rng(seed)
    n_blob, n_iso, n_dup, k = 1900, 150, 61, 14
    centres = rng.uniform(-3.0, 3.0, (k, 3))
    sigma = rng.uniform(0.08, 0.35, k)
    which = rng.integers(0, k, n_blob)
    blob = centres[which] + rng.normal(0, 1, (n_blob, 3)) * sigma[which, None]
    iso = rng.uniform(-6.0, 6.0, (n_iso, 3))
    xyz = np.concatenate([blob, iso]).astype(np.float32)
    src = rng.integers(0, len(xyz), n_dup)
    xyz = np.concatenate([xyz, xyz[src]])                      # exact duplicates, far from their originals in index
    which = np.concatenate([which, np.full(n_iso, -1), np.where(src < n_blob, which[np.minimum(src, n_blob - 1)], -1)])
    perm = rng.permutation(len(xyz))
    xyz, which = xyz[perm], which[perm]
    n = len(xyz)
    on = np.zeros((n, 8), bool)
    on[:, 1] = True
    far = np.flatnonzero(which == -1)
    keep = []
    for i in far:                                               # a subset with every pair more than 1 m apart
        if all(np.linalg.norm(xyz[i].astype(np.float64) - xyz[j].astype(np.float64)) > 1.0 for j in keep):
            keep.append(i)
    on[keep, 2] = True
    for q in range(3, 8):
        chosen = rng.choice(k, rng.integers(2, 6), replace=False)
        on[:, q] = np.isin(which, chosen) & (rng.random(n) < rng.uniform(0.3, 1.0))
        on[:, q] |= (which == -1) & (rng.random(n) < 0.2)
    return xyz, _logits(rng, on)


def _shapes(seed=5):
    """Hand-built structures, 3 m apart along z so that none sees another; the scene's lowest corner is (-5, -5, -5)
    and three rows of points start on it at multiples of h = eps / 2 (points on cell faces).  Queries: 0 everything,
    then one per group of structures, the last one everything with points dropped at random."""
    rng = np.random.default_rng(seed)
    pts, tag = [], []

    def add(name, p, z):
        p = np.asarray(p, np.float64).reshape(-1, 3) + np.array([0.0, 0.0, z])
        pts.append(p)
        tag.extend([name] * len(p))

    # points on cell faces: x = -5 + k h, one row per eps (y drifts so that no distance is a multiple of h)
    for r, eps in enumerate((0.95, 0.21, 0.3)):
        kk = np.arange(12)
        add("faces", np.stack([-5 + kk * (np.float32(eps).astype(np.float64) / 2), -5 + 0.05 * kk, np.full(12, -5.0)], 1),
            3.0 * r)
    z = 6.0

    def ball(c, r, m):                                          # m points uniform in the ball of radius r around c
        v = rng.normal(0, 1, (m, 3))
        return c + v / np.linalg.norm(v, axis=1, keepdims=True) * r * rng.random((m, 1)) ** (1 / 3)

    # two balls joined by one bridge point
    z += 3.0
    add("bridge", np.concatenate([ball(np.array([0.0, 0, 0]), 0.1, 50), ball(np.array([0.7, 0, 0]), 0.1, 50),
                                  [[0.35, 0.0, 0.0]]]), z)
    # a 40-hop chain at spacing 0.205 (one cluster at eps = 0.21, more than 32 cells long)
    z += 3.0
    kk = np.arange(41)
    add("chain", np.stack([-4 + 0.205 * kk, 0.004 * (kk % 2), np.zeros(41)], 1), z)
    # isolated single points
    z += 3.0
    add("singles", np.stack([-4 + 1.7 * np.arange(6), np.zeros(6), np.zeros(6)], 1), z)
    # more than 256 points in one cell, single points in the cells next to it, and a tail of border points
    z += 3.0
    add("dense", np.concatenate([ball(np.array([0.05, 0.05, 0.05]), 0.02, 300),
                                 [[0.30, 0.05, 0.05], [-0.2, 0.05, 0.05], [0.05, 0.3, 0.05], [0.05, 0.05, -0.2],
                                  [0.55, 0.05, 0.05], [0.05, 0.52, 0.05]]]), z)
    # cross: the centre is core at min_samples = 4 only through its three arms, which lie in other cells
    z += 3.0
    add("cross", [[0.0, 0, 0], [0.25, 0, 0], [-0.25, 0.01, 0], [0.0, 0.26, 0]], z)
    # a non-core point within eps of core points of two clusters: the cluster of the earlier core point (at +x, the
    # farther one) must take it.  The four points of a group are 0.06 apart: all core at min_samples = 4.
    z += 3.0
    add("between", np.concatenate([np.stack([0.27 + 0.06 * np.arange(4), np.zeros(4), np.zeros(4)], 1),
                                   np.stack([-0.25 - 0.06 * np.arange(4), np.zeros(4), np.zeros(4)], 1),
                                   [[0.0, 0.0, 0.0]]]), z)
    # two crosses P and R in index order: arm of P (border), all of R (centre first), rest of P.  P holds the lowest
    # index, R the lowest core index, so R is cluster 0.
    z += 3.0
    cross = np.array([[0.0, 0, 0], [0.25, 0, 0], [-0.25, 0.01, 0], [0.0, 0.26, 0]])
    P, R = cross + np.array([-1.0, 0, 0]), cross + np.array([1.0, 0, 0])
    add("numbering", np.concatenate([P[1:2], R, P[0:1], P[2:]]), z)
    xyz = np.concatenate(pts).astype(np.float32)
    tag = np.array(tag)
    groups = (("faces",), ("bridge", "chain"), ("singles", "dense"), ("cross", "between", "numbering"),
              ("numbering", "between", "faces"))
    on = np.zeros((len(xyz), 2 + len(groups)), bool)
    on[:, 0] = True
    for q, g in enumerate(groups):
        on[:, 1 + q] = np.isin(tag, g)
    on[:, -1] = rng.random(len(xyz)) < 0.7
    return xyz, _logits(rng, on)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz f32[N,3], logits f32[N,Q]); built once, never modified."""
    out = {"tiny": _tiny(), "wide": _wide(), "blobs": _blobs(), "shapes": _shapes()}
    for xyz, logits in out.values():
        xyz.setflags(write=False)
        logits.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sklearn_labels(name, eps, min_samples):
    """sklearn's labels of every query of a case: list over q of i64[n_on_q] (the on-points in index order)."""
    from sklearn.cluster import DBSCAN

    xyz, logits = cases()[name]
    out = []
    for q in range(logits.shape[1]):
        on = logits[:, q] > 0
        out.append(DBSCAN(eps=eps, min_samples=min_samples).fit(xyz[on].astype(np.float64)).labels_.astype(np.int64)
                   if on.any() else np.zeros(0, np.int64))
    return out


def lattice_scene(n_side=100, Q=24, seed=2):
    """About 20 000 voxels of a floor and two walls on a 0.02 m lattice, and Q planted masks (query 0: the floor, the
    others boxes cut out of the scene, some made of two parts).  Lattice distances are 0.02 sqrt(integer) and
    (eps / 0.02)^2 = 2256.25 for eps = 0.95, so no pair comes nearer to eps than 5e-5 eps."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    floor = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3)
    wall_a = np.stack([i, np.zeros_like(i), j + 1], -1).reshape(-1, 3)[:: 2]
    wall_b = np.stack([np.zeros_like(i), i + 1, j + 1], -1).reshape(-1, 3)[:: 2]
    vox = np.unique(np.concatenate([floor, wall_a, wall_b]), axis=0)
    vox = vox[rng.permutation(len(vox))]
    xyz = (vox * 0.02).astype(np.float32)
    on = np.zeros((len(xyz), Q), bool)
    on[:, 0] = vox[:, 2] == 0
    for q in range(1, Q):
        for _ in range(1 + q % 3):
            c = vox[rng.integers(0, len(vox))]
            on[:, q] |= (np.abs(vox - c) <= rng.integers(4, 20)).all(1)
    return xyz, _logits(rng, on)
