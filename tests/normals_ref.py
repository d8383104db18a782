"""Reference and inputs of the neighbour-list and normal tests (tests/test_gpu_knn_hybrid.py, tests/test_gpu_normals.py,
tests/test_normals_host.py): numpy float64, brute force.

`knn_hybrid_f64` is the contract of usc_knn_hybrid_grid: squared distances in float64 on the float32 inputs, summed
x, y, z in that order; candidates have d2 < r2, strictly, with r2 = float64(float32(radius)) ** 2; they are ordered by
(d2, index); the first min(k, m) are listed, the rest of the row is -1.  `pca_f64` is the contract of usc_normals_pca
up to the eigen solve, which is numpy.linalg.eigh here."""
import numpy as np


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3)).astype(np.float64)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3), dtype=np.float32)


def knn_hybrid_f64(query, ref, k, radius, chunk=256):
    """-> (idx i32[nq,k], count i32[nq])."""
    q, r = _f64(query), _f64(ref)
    r2 = float(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))
    idx = np.full((q.shape[0], k), -1, np.int32)
    count = np.zeros(q.shape[0], np.int32)
    index = np.arange(r.shape[0])
    for s in range(0, q.shape[0], chunk):
        d = q[s:s + chunk, None, :] - r[None, :, :]
        d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        for i in range(d.shape[0]):
            cand = np.nonzero(d[i] < r2)[0]
            order = cand[np.lexsort((index[cand], d[i, cand]))][:k]
            idx[s + i, :order.shape[0]] = order
            count[s + i] = order.shape[0]
    return idx, count


def pca_f64(query, ref, idx, count):
    """Per query: covariance of x_j = ref[idx_j] - query over the listed neighbours, its eigenvalues ascending and the
    eigenvector of the smallest, and s = sum |x_j|^2 / m.
    -> (normal f64[nq,3], lam f64[nq,3], s f64[nq]); rows with count < 3 hold (0, 0, 1), zeros and 0."""
    q, r = _f64(query), _f64(ref)
    nq = q.shape[0]
    normal = np.tile(np.array([0.0, 0.0, 1.0]), (nq, 1))
    lam = np.zeros((nq, 3))
    s = np.zeros(nq)
    for i in range(nq):
        m = int(count[i])
        if m < 3:
            continue
        x = r[idx[i, :m]] - q[i]
        c = x - x.mean(0)
        w, v = np.linalg.eigh(c.T @ c / m)
        normal[i], lam[i], s[i] = v[:, 0], w, (x * x).sum() / m
    return normal, lam, s


def sign_rule_holds(n):
    """The stored component of largest magnitude, the lowest axis among equals, is >= 0: bool[nq]."""
    n = np.asarray(n)
    lead = np.abs(n).argmax(1)                         # argmax returns the first maximum
    return n[np.arange(n.shape[0]), lead] >= 0


# ---------------------------------------------------------------------------------------------------- inputs (r = 0.1)
def noisy_plane(seed=21):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.random((2500, 2)), rng.normal(0, 0.002, (2500, 1))], 1)
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return _f32(p @ rot.T + np.array([3.0, 5.0, 1.0]))


def sphere(seed=22):
    v = np.random.default_rng(seed).normal(size=(3000, 3))
    return _f32(0.5 * v / np.linalg.norm(v, axis=1, keepdims=True))


def two_planes(seed=23):
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.random((1200, 2)) * [1.0, 0.6], np.zeros((1200, 1))], 1)
    b = np.concatenate([rng.random((1200, 1)), np.zeros((1200, 1)), rng.random((1200, 1)) * 0.6], 1)
    return _f32(np.concatenate([a, b]) + rng.normal(0, 0.001, (2400, 3)))


def planar_lattice():
    """20 x 20, spacing 0.03, in the plane z = 0.25: many neighbours at equal distances."""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2) * 0.03
    return _f32(np.concatenate([g, np.full((400, 1), 0.25)], 1))


def slab_lattice():
    """12 x 12 x 3, spacing 1/32: coordinates and squared distances are exact in binary."""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    return _f32(g / 32.0)


def sparse_cube(seed=24):
    return _f32(np.random.default_rng(seed).random((300, 3)) * 1.2)


def line():
    return _f32(np.outer(np.arange(200) * 0.01, [1.0, 2.0, -0.5]) + [0.5, 0.25, 1.0])


NORMAL_CASES = {"noisy_plane": noisy_plane, "sphere": sphere, "two_planes": two_planes,
                "planar_lattice": planar_lattice, "slab_lattice": slab_lattice, "sparse_cube": sparse_cube}
