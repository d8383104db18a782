"""Brute-force f64 restatement of sklearn.cluster.DBSCAN's labels, with no order of traversal left open — the rule
the kernels of csrc/dbscan.hip implement (test_dbscan_host.py pins it to sklearn itself on every case):

  neighbours  d^2 <= eps^2, the point itself included
  core        at least min_samples neighbours
  clusters    connected components of the core points under the neighbour relation,
              numbered by ascending lowest-index core point
  border      a non-core point with a core neighbour takes the lowest cluster number among its core neighbours
  noise       a non-core point without a core neighbour: -1

Distances as the kernels take them: differences and squares of the f32 coordinates in f64, against the square in
f64 of eps rounded to f32."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components


def dbscan_ref(xyz, eps, min_samples):
    x = np.asarray(xyz, np.float32).astype(np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0, np.int64)
    e = float(np.float32(eps))
    d = x[:, None, :] - x[None, :, :]
    near = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2] <= e * e
    core = near.sum(1) >= min_samples
    labels = np.full(n, -1, np.int64)
    idx = np.flatnonzero(core)
    if len(idx) == 0:
        return labels
    _, comp = connected_components(csr_matrix(near[np.ix_(idx, idx)]), directed=False)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, idx)                       # lowest-index core point of every component
    number = np.empty_like(first)
    number[np.argsort(first)] = np.arange(len(first))
    labels[idx] = number[comp]
    for i in np.flatnonzero(~core):
        nb = np.flatnonzero(near[i] & core)
        if len(nb):
            labels[i] = labels[nb].min()
    return labels
