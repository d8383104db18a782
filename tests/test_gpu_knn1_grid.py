"""usc_knn1_grid (ops.knn1_grid) against the brute-force kernel usc_knn1 (ops.knn1) and against numpy float64
(tests/knn_ref.py): the index of EVERY query is equal and dist2 carries the same f32 bits — in every case below."""
import numpy as np
import pytest
import torch

import knn_ref as K

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _check(query, ref, device, **kw):
    """ops.knn1_grid(query, ref, **kw) == ops.knn1 == numpy f64, index for index and bit for bit."""
    from unscene3d_amd import ops
    q, r = _dev(query, device), _dev(ref, device)
    d, i = ops.knn1_grid(q, r, **kw)
    d_b, i_b = ops.knn1(q, r)
    assert i.dtype == torch.int64 and d.dtype == torch.float32 and i.shape == d.shape == (query.shape[0],)
    assert np.array_equal(i.cpu().numpy(), i_b.cpu().numpy()), "index differs from usc_knn1"
    assert np.array_equal(_bits(d), _bits(d_b)), "dist differs from usc_knn1"
    if query.shape[0] * ref.shape[0] <= K.MAX_PAIRS:
        i_n, d2_n = K.knn1_f64(query, ref)
        assert np.array_equal(i.cpu().numpy(), i_n), "index differs from the float64 argmin"
        assert np.array_equal(_bits(d), _bits(torch.from_numpy(d2_n).to(device).sqrt())), "dist2 differs from float64"
    return d, i


def test_single_point_single_query(device):
    _check(np.array([[0.5, -1.0, 2.0]]), np.array([[1.0, 1.0, 1.0]]), device)
    _check(np.array([[1.0, 1.0, 1.0]]), np.array([[1.0, 1.0, 1.0]]), device, cell=0.25)


def test_single_reference_point(device):
    rng = np.random.default_rng(1)
    _, i = _check(rng.normal(0, 3, (1000, 3)), np.array([[0.25, 0.5, -0.75]]), device)
    assert int(i.max()) == 0


def test_no_query(device):
    from unscene3d_amd import ops
    d, i = ops.knn1_grid(torch.zeros((0, 3), device=device), _dev(np.random.default_rng(2).random((100, 3)), device))
    assert d.shape == i.shape == (0,)


@pytest.mark.parametrize("cell", [1.0, 2.0, 3.7])
def test_lattice_ties(device, cell):
    query, ref = K.lattice_ties()
    _check(query, ref, device, cell=cell)


def test_wall_ties(device):
    query, ref = K.wall_ties(cell=0.5)
    _, i = _check(query, ref, device, cell=0.5)
    assert np.array_equal(i.cpu().numpy(), 2 * np.arange(query.shape[0])), "the lower index of each pair wins"


def test_duplicate_reference_points(device):
    query, ref = K.duplicates()
    _, i = _check(query, ref, device)
    assert int(i[0]) == 17                                   # the lowest of the five copies (40 itself is higher)
    _check(query, ref, device, cell=0.05)


def test_far_queries(device):
    query, ref = K.far_queries(cell=0.1)
    _check(query, ref, device, cell=0.1)
    _check(query, ref, device, cell=0.1, bounds=([0, 0, 0], [1, 1, 1]))


def test_two_clusters(device):
    query, ref = K.two_clusters(cell=0.125)
    _check(query, ref, device, cell=0.125)


@pytest.mark.parametrize("cell", [0.05, 1e3, 1e-4, None])
def test_random_box(device, cell):
    from unscene3d_amd import ops
    from unscene3d_amd._lib import lib
    query, ref = K.random_box()
    _check(query, ref, device, cell=cell)
    origin, used, dims = ops.knn1_grid_plan(ref.min(0), ref.max(0), ref.shape[0], cell)
    nbytes = lib.usc_knn1_grid_ws_bytes(ref.shape[0], dims.ctypes.data)
    assert 0 < nbytes < 64 << 20                             # cell = 1e-4 on a 4 m box: coarsened, not 10^13 cells
    assert int(dims.prod()) <= ops.KNN1_GRID_CELL_BUDGET
    if cell == 1e3:
        assert dims.tolist() == [1, 1, 1] and used == 1e3
    if cell == 1e-4:
        assert used > 1e-4


def test_bounds_that_miss_points(device):
    """Bounds are a hint: reference points outside them are binned into the boundary cells."""
    query, ref = K.random_box(nq=2000, nr=1500)
    _check(query, ref, device, cell=0.1, bounds=([1.0, 1.0, 1.0], [2.0, 1.5, 1.25]))


def test_two_calls_are_identical(device):
    from unscene3d_amd import ops
    query, ref = K.random_box()
    query[:1728], _ = K.lattice_ties()
    ref[:100] = K.lattice_ties()[1][:100]
    q, r = _dev(query, device), _dev(ref, device)
    d0, i0 = ops.knn1_grid(q, r, cell=0.5)
    d1, i1 = ops.knn1_grid(q, r, cell=0.5)
    assert torch.equal(i0, i1) and np.array_equal(_bits(d0), _bits(d1))


def test_short_workspace_is_refused_before_any_launch(device):
    from unscene3d_amd import ops
    from unscene3d_amd._lib import last_error, lib
    query, ref = K.random_box(nq=300, nr=200)
    q, r = _dev(query, device), _dev(ref, device)
    origin, cell, dims = ops.knn1_grid_plan(ref.min(0), ref.max(0), ref.shape[0], 0.25)
    nbytes = lib.usc_knn1_grid_ws_bytes(ref.shape[0], dims.ctypes.data)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    idx = torch.full((300,), -7, dtype=torch.int64, device=device)
    d2 = torch.full((300,), -7.0, dtype=torch.float32, device=device)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.usc_knn1_grid(q.data_ptr(), 300, r.data_ptr(), 200, origin.ctypes.data, cell, dims.ctypes.data,
                           idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes - 1, stream)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace too small" in last_error()
    assert int((idx != -7).sum()) == 0 and int((d2 != -7.0).sum()) == 0 and int(ws.sum()) == 0    # nothing ran
    rc = lib.usc_knn1_grid(q.data_ptr(), 300, r.data_ptr(), 200, origin.ctypes.data, cell, dims.ctypes.data,
                           idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert rc == 0
    assert torch.equal(idx, ops.knn1(q, r)[1])
