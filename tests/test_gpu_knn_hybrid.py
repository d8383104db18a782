"""usc_knn_hybrid_grid (ops.knn_hybrid) against numpy float64 brute force (tests/normals_ref.py): idx and count of EVERY
query are equal to the oracle's, exactly, in every case below."""
import numpy as np
import pytest
import torch

import knn_ref as K
import normals_ref as N

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _check(query, ref, k, radius, device, **kw):
    from unscene3d_amd import ops
    idx, count = ops.knn_hybrid(_dev(query, device), _dev(ref, device), k, radius, **kw)
    assert idx.dtype == torch.int32 and count.dtype == torch.int32
    assert idx.shape == (query.shape[0], k) and count.shape == (query.shape[0],)
    idx_n, count_n = N.knn_hybrid_f64(query, ref, k, radius)
    assert np.array_equal(count.cpu().numpy(), count_n), "count differs from the float64 oracle"
    assert np.array_equal(idx.cpu().numpy(), idx_n), "idx differs from the float64 oracle"
    return idx_n, count_n


def test_one_point(device):
    p = np.array([[0.5, -1.0, 2.0]], np.float32)
    idx, count = _check(p, p, 3, 0.1, device)
    assert idx.tolist() == [[0, -1, -1]] and count.tolist() == [1]
    _check(np.array([[0.7, -1.0, 2.0]], np.float32), p, 3, 0.1, device)        # nothing inside the radius


def test_no_query(device):
    from unscene3d_amd import ops
    idx, count = ops.knn_hybrid(torch.zeros((0, 3), device=device), _dev(np.random.default_rng(2).random((100, 3)), device),
                                5, 0.1)
    assert idx.shape == (0, 5) and count.shape == (0,)


def test_k1_finds_the_point_itself(device):
    _, ref = K.random_box(nq=1, nr=2000)
    idx, count = _check(ref, ref, 1, 0.1, device)
    assert np.array_equal(idx[:, 0], np.arange(2000)) and (count == 1).all()


def test_k64(device):
    _, ref = K.random_box(nq=1, nr=2500)
    _, count = _check(ref[:800], ref, 64, 0.6, device)
    assert (count == 64).sum() > 400 and (count < 64).sum() > 0             # both kinds of row


def test_tiny_radius(device):
    _, ref = K.random_box(nq=1, nr=1500)
    _, count = _check(ref, ref, 30, 1e-6, device)
    assert (count == 1).all()


def test_radius_covering_everything(device):
    query, ref = K.random_box(nq=400, nr=700)
    _, count = _check(query, ref, 30, 10.0, device)
    assert (count == 30).all()
    _, count = _check(query[:50], ref[:20], 30, 10.0, device)                # fewer points than k
    assert (count == 20).all()


def test_duplicates(device):
    query, ref = K.duplicates()
    idx, _ = _check(query, ref, 8, 0.25, device)
    assert idx[0, :6].tolist() == [17, 40, 88, 250, 333, 491]               # d2 = 0 six times: index order
    _check(query, ref, 3, 0.25, device, cell=0.05)                           # the tie is cut at the k-th place


def test_lattice_ties(device):
    p = N.slab_lattice()
    idx, count = _check(p, p, 30, 0.1, device)
    P = p.astype(np.float64)
    d = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)                        # exact: multiples of 2^-10
    kth = np.sort(d, 1)[:, 29:31]
    assert (count == 30).all() and (kth[:, 0] == kth[:, 1]).mean() > 0.25    # the cut falls inside a tie
    _check(p, p, 30, 0.1, device, cell=1.0 / 32)


def test_queries_outside_the_box(device):
    query, ref = K.far_queries(cell=0.1)
    _, count = _check(query, ref, 30, 0.1, device, cell=0.1)
    assert (count == 0).sum() >= 26 * 8 and (count > 0).sum() > 0
    _check(query, ref, 30, 0.1, device, cell=0.1, bounds=([0, 0, 0], [1, 1, 1]))
    _check(query, ref, 30, 6.0, device, cell=0.1, bounds=([0, 0, 0], [1, 1, 1]))   # far queries that reach the box


@pytest.mark.parametrize("cell", [1e-4, 1e3])
def test_bad_grids(device, cell):
    query, ref = K.random_box(nq=1500, nr=1500)
    _check(query, ref, 30, 0.3, device, cell=cell)


def test_small_cell_through_the_abi(device):
    """A cell far below the radius, given to the library as it is (ops would coarsen it): every query's ball reaches
    past the bounded walk, so every query reads all reference points."""
    from unscene3d_amd._lib import lib
    query, ref = K.random_box(nq=300, nr=400)
    q, r = _dev(query, device), _dev(ref, device)
    origin = np.zeros(3)
    dims = np.array([100, 75, 63], np.int32)                                 # cell 0.04 over the 4 x 3 x 2.5 box
    nbytes = lib.usc_knn_hybrid_grid_ws_bytes(400, dims.ctypes.data)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    idx = torch.empty((300, 30), dtype=torch.int32, device=device)
    count = torch.empty(300, dtype=torch.int32, device=device)
    rc = lib.usc_knn_hybrid_grid(q.data_ptr(), 300, r.data_ptr(), 400, 0.5, 30, origin.ctypes.data, 0.04,
                                 dims.ctypes.data, idx.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    idx_n, count_n = N.knn_hybrid_f64(query, ref, 30, 0.5)
    assert np.array_equal(idx.cpu().numpy(), idx_n) and np.array_equal(count.cpu().numpy(), count_n)


def test_bounds_that_miss_points(device):
    query, ref = K.random_box(nq=1500, nr=1500)
    _check(query, ref, 30, 0.3, device, bounds=([1.0, 1.0, 1.0], [2.0, 1.5, 1.25]))


def test_random(device):
    query, ref = K.random_box(nq=3000, nr=3000)
    _, count = _check(query, ref, 30, 0.4, device)
    assert (count == 30).sum() > 100 and (count < 30).sum() > 100


def test_two_calls_are_identical(device):
    from unscene3d_amd import ops
    query, ref = K.random_box(nq=3000, nr=3000)
    q, r = _dev(query, device), _dev(ref, device)
    i0, c0 = ops.knn_hybrid(q, r, 30, 0.4)
    i1, c1 = ops.knn_hybrid(q, r, 30, 0.4)
    assert torch.equal(i0, i1) and torch.equal(c0, c1)


def test_refusals_write_nothing(device):
    from unscene3d_amd import ops
    from unscene3d_amd._lib import last_error, lib
    query, ref = K.random_box(nq=300, nr=200)
    q, r = _dev(query, device), _dev(ref, device)
    origin, cell, dims = ops.knn1_grid_plan(ref.min(0), ref.max(0), 200, 0.25)
    nbytes = lib.usc_knn_hybrid_grid_ws_bytes(200, dims.ctypes.data)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    idx = torch.full((300, 64), -7, dtype=torch.int32, device=device)
    count = torch.full((300,), -7, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream().cuda_stream

    def call(radius, k, ws_bytes):
        rc = lib.usc_knn_hybrid_grid(q.data_ptr(), 300, r.data_ptr(), 200, radius, k, origin.ctypes.data, cell,
                                     dims.ctypes.data, idx.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes, stream)
        torch.cuda.synchronize()
        return rc

    for radius, k, ws_bytes, word in [(0.25, 0, nbytes, "k must be"), (0.25, 65, nbytes, "k must be"),
                                      (0.0, 30, nbytes, "radius"), (float("nan"), 30, nbytes, "radius"),
                                      (float("inf"), 30, nbytes, "radius"), (-1.0, 30, nbytes, "radius"),
                                      (0.25, 30, nbytes - 1, "workspace too small")]:
        assert call(radius, k, ws_bytes) == -1 and word in last_error(), (radius, k, ws_bytes)
        assert int((idx != -7).sum()) == 0 and int((count != -7).sum()) == 0 and int(ws.sum()) == 0   # nothing ran
    for bad in (dict(k=0), dict(k=65), dict(radius=0.0), dict(radius=float("nan"))):
        with pytest.raises(RuntimeError):
            ops.knn_hybrid(q, r, **{"k": 30, "radius": 0.25, **bad})
    assert call(0.25, 30, nbytes) == 0
    idx_n, count_n = N.knn_hybrid_f64(query, ref, 30, 0.25)
    got = idx.cpu().numpy().reshape(-1)[:300 * 30].reshape(300, 30)          # k = 30 rows are packed: 30 per query
    assert np.array_equal(got, idx_n) and np.array_equal(count.cpu().numpy(), count_n)
