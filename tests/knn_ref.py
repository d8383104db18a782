"""Reference and inputs of the exact 1-NN tests (tests/test_gpu_knn1_grid.py).

`knn1_f64` is the contract of usc_knn1 / usc_knn1_grid in numpy: squared distances in float64 on the float32 inputs,
summed x, y, z in that order, the lowest reference index among equidistant points (np.argmin returns the first minimum),
dist2 rounded once to float32.  The cases are small on purpose: each is built so that a grid search that stops too early,
compares ties in visiting order or mishandles a clamped query returns another index than the brute-force search."""
import numpy as np

MAX_PAIRS = 2 * 10 ** 7          # above this many (query, reference) pairs only the device brute force is the reference


def knn1_f64(query, ref, chunk=512):
    """-> (idx i64[nq], dist2 f32[nq])."""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    r = np.asarray(ref, np.float32).astype(np.float64).reshape(-1, 3)
    idx = np.empty(q.shape[0], np.int64)
    d2 = np.empty(q.shape[0], np.float32)
    for s in range(0, q.shape[0], chunk):
        d = q[s:s + chunk, None, :] - r[None, :, :]
        d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        j = d.argmin(1)
        idx[s:s + chunk] = j
        d2[s:s + chunk] = d[np.arange(d.shape[0]), j].astype(np.float32)
    return idx, d2


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3), dtype=np.float32)


def lattice_ties(seed=11):
    """ref: the even-coordinate points of a random 60 % occupancy of a 12^3 box; queries: every integer point of the
    box, so almost every query has 2 to 8 equidistant neighbours."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    occ = g[rng.random(g.shape[0]) < 0.6]
    ref = occ[(occ % 2 == 0).all(1)]
    ref = ref[rng.permutation(ref.shape[0])]           # index order unrelated to position
    return _f32(g), _f32(ref)


def wall_ties(cell=0.5):
    """Queries on cell walls (every coordinate an exact multiple of `cell`) with one reference point at +d and one at
    -d along an axis, in both index orders.  A query on a wall is the lowest point of its cell, so for d > cell the
    point at -d lies one ring further out than the point at +d; with order 1 that later point has the lower index."""
    query, ref = [], []
    n = 0
    for axis in range(3):
        for d in (0.25 * cell, 1.0 * cell, 1.5 * cell, 2.5 * cell, 3.25 * cell):
            for order in (0, 1):
                p = np.array([16.0 * cell * n, 8.0 * cell, 8.0 * cell])
                e = np.zeros(3)
                e[axis] = d
                pair = [p + e, p - e]
                ref += pair if order == 0 else pair[::-1]
                query.append(p)
                n += 1
    return _f32(query), _f32(ref)


def duplicates(seed=12):
    """The same reference point five times at scattered indices; queries on it, near it and elsewhere."""
    rng = np.random.default_rng(seed)
    ref = rng.random((500, 3)) * 2.0
    for i in (491, 17, 333, 250, 88):
        ref[i] = ref[40]
    query = np.concatenate([ref[40][None], ref[40][None] + rng.normal(0, 0.02, (200, 3)), rng.random((300, 3)) * 2.0])
    return _f32(query), _f32(ref)


def far_queries(cell=0.1, seed=13):
    """Reference points in a unit box, queries 50 cells outside it on every axis, both ways, and on the diagonals (the
    clamped start cell, the streaming pass), between queries inside the box (same blocks as the far ones)."""
    rng = np.random.default_rng(seed)
    ref = rng.random((2000, 3))
    inside = rng.random((300, 3))
    far = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if sx or sy or sz:
                    off = np.array([sx, sy, sz]) * 50 * cell
                    far.append(np.where(off > 0, 1.0 + off, off) + (off == 0) * rng.random((8, 3)))
    query = np.concatenate([inside[:150]] + far + [inside[150:]])
    return _f32(query), _f32(ref)


def two_clusters(cell=0.125):
    """Two slabs of lattice points 100 cells apart and queries on and around the plane halfway between the facing
    layers: the nearest point is ~50 cells away and every query on the plane has equidistant points in both slabs, the
    lower index sometimes in one, sometimes in the other."""
    ys = np.arange(0, 8) * 0.5
    a = np.array([[x, y, z] for x in (0.0, cell) for y in ys for z in ys])
    b = np.array([[x, y, z] for x in (101 * cell, 102 * cell) for y in ys for z in ys])
    ref = np.empty((a.shape[0] + b.shape[0], 3))
    ref[0::2], ref[1::2] = a, b[::-1]                   # interleaved: ties go to either slab
    mid = (cell + 101 * cell) / 2.0                     # 6.375: exact in binary
    query = np.array([[mid + dx, y, z] for dx in (0.0, -cell, cell, -0.03125, 0.03125)
                      for y in np.arange(-1, 9) * 0.5 for z in np.arange(0, 8) * 0.5 + 0.25])
    return _f32(query), _f32(ref)


def random_box(nq=5000, nr=3000, seed=14):
    """f32 uniform in a 4 x 3 x 2.5 box."""
    rng = np.random.default_rng(seed)
    box = np.array([4.0, 3.0, 2.5])
    return _f32(rng.random((nq, 3)) * box), _f32(rng.random((nr, 3)) * box)
