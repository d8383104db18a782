"""usc_normals_pca / ops.estimate_normals (radius 0.1, 30 neighbours) against numpy float64 (tests/normals_ref.py).

Accuracy: with s = sum |x_j|^2 / m, lam1 <= lam2 the two smallest eigenvalues of the float64 covariance and theta the
angle to +-(its eigenvector), theta <= 2^-21 + 2048 * 2^-53 * s / (lam2 - lam1).  The first term is four times the
rounding of the f32 store; the second is Davis-Kahan for a covariance summed from at most 64 f64 terms and a
backward-stable solve, with 4x headroom.  Points with lam2 - lam1 < 2^-20 * s have no direction to compare and are left
out; at most 1 % of a case may be.  Every point of every case: finite, unit length within 2^-22, the sign rule on the
stored values, (0, 0, 1) exactly where fewer than 3 neighbours were found, and estimate_normals equal to the two calls."""
import numpy as np
import pytest
import torch

import normals_ref as N

pytestmark = pytest.mark.gpu

RADIUS, MAX_NN = 0.1, 30
_REF = {}


def _reference(name, idx):
    """(normal, lam, s) in float64 from the neighbour lists the device returned: computed once per case, read-only.
    The lists themselves are compared with the oracle in tests/test_gpu_knn_hybrid.py, on inputs whose squared distances
    are exact or all different; on the f32 lattices here two neighbours can be equidistant in numpy's unfused sum and
    one ulp apart in the kernel's fused one, which is usc_knn1's."""
    if name not in _REF:
        p = _points(name)
        idx_n, count_n = N.knn_hybrid_f64(p, p, MAX_NN, RADIUS)
        out = (count_n,) + N.pca_f64(p, p, idx, count_n)
        for a in out:
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


def _points(name):
    return (N.NORMAL_CASES.get(name) or N.line)()


def _device_normals(p, device):
    from unscene3d_amd import ops
    pts = torch.from_numpy(p).to(device)
    idx, count = ops.knn_hybrid(pts, pts, MAX_NN, RADIUS)
    two = ops.normals_pca(pts, pts, idx, count)
    one = ops.estimate_normals(pts, RADIUS, MAX_NN)
    assert one.dtype == torch.float32 and one.shape == p.shape
    assert np.array_equal(one.cpu().numpy().view(np.uint32), two.cpu().numpy().view(np.uint32))
    return one.cpu().numpy(), idx.cpu().numpy(), count.cpu().numpy()


def _check_rules(n, count):
    assert np.isfinite(n).all()
    n64 = n.astype(np.float64)
    assert np.abs(np.sqrt((n64 * n64).sum(1)) - 1.0).max() <= 2.0 ** -22
    assert N.sign_rule_holds(n).all()
    few = count < 3
    assert np.array_equal(n[few], np.tile(np.array([0, 0, 1], np.float32), (int(few.sum()), 1)))


@pytest.mark.parametrize("name", sorted(N.NORMAL_CASES))
def test_normals_against_float64(device, name):
    p = _points(name)
    n, idx, count = _device_normals(p, device)
    count_n, normal, lam, s = _reference(name, idx)
    assert np.array_equal(count, count_n)
    _check_rules(n, count)
    have = count >= 3
    gap = lam[:, 1] - lam[:, 0]
    keep = have & (gap >= 2.0 ** -20 * s)
    assert (have & ~keep).sum() <= 0.01 * p.shape[0]
    n64 = n.astype(np.float64)[keep]
    theta = np.arctan2(np.linalg.norm(np.cross(n64, normal[keep]), axis=1), np.abs((n64 * normal[keep]).sum(1)))
    bound = 2.0 ** -21 + 2048 * 2.0 ** -53 * s[keep] / gap[keep]
    worst = int(np.argmax(theta / bound))
    print(f"{name}: {int(keep.sum())} of {p.shape[0]} compared, {int((count < 3).sum())} with fewer than 3 neighbours, "
          f"max theta {theta.max():.3e}, max theta/bound {theta[worst] / bound[worst]:.3f}, "
          f"min relative gap {(gap[keep] / s[keep]).min():.3e}")
    assert (theta <= bound).all()
    if name == "sparse_cube":
        assert (count < 3).sum() > 200 and keep.sum() > 10


def test_line_follows_the_rules(device):
    """Collinear points: two zero eigenvalues, no direction to compare."""
    p = _points("line")
    n, idx, count = _device_normals(p, device)
    assert np.array_equal(count, _reference("line", idx)[0]) and (count >= 3).all()
    _check_rules(n, count)


def test_degenerate_lists(device):
    """Fewer than 3 neighbours, coincident neighbours (a zero covariance) and an index that is no reference point."""
    from unscene3d_amd import ops
    ref = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]], device=device)
    q = torch.zeros((4, 3), device=device)
    idx = torch.tensor([[0, 1, -1, -1], [0, 0, 0, 0], [0, 1, 2, 9], [0, 1, 2, 3]], dtype=torch.int32,
                       device=device)
    count = torch.tensor([2, 4, 4, 4], dtype=torch.int32, device=device)
    n = ops.normals_pca(q, ref, idx, count).cpu().numpy()
    assert np.array_equal(n, np.tile(np.array([0, 0, 1], np.float32), (4, 1)))          # row 3: the plane z = 0
