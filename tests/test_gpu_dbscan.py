"""GPU: the batched DBSCAN split (csrc/dbscan.hip) against sklearn itself on the cases of dbscan_cases.py, against
the per-query route it replaces, through export_instances, run twice for identical bytes, and within a memory bound
that no [N,N] table fits in."""
import numpy as np
import pytest
import torch

import dbscan_cases as DC

pytestmark = pytest.mark.gpu

CASES = list(DC.cases())


def _on_device(name, device):
    xyz, logits = DC.cases()[name]
    return torch.from_numpy(xyz.copy()).to(device), torch.from_numpy(logits.copy()).to(device)


@pytest.mark.parametrize("eps, min_samples", DC.PARAMS)
@pytest.mark.parametrize("name", CASES)
def test_labels_equal_sklearn(device, name, eps, min_samples):
    from unscene3d_amd import ops

    xyz, logits = _on_device(name, device)
    labels, n_clusters = ops.dbscan_masks(xyz, logits, eps, min_samples)
    assert labels.shape == logits.shape and labels.dtype == torch.int32 and n_clusters.dtype == torch.int32
    labels, n_clusters = labels.cpu().numpy(), n_clusters.cpu().numpy()
    want = DC.sklearn_labels(name, eps, min_samples)
    on = DC.cases()[name][1] > 0
    assert (labels[~on] < 0).all()
    for q in range(on.shape[1]):
        assert np.array_equal(labels[on[:, q], q], want[q]), (name, eps, min_samples, q)
        assert n_clusters[q] == (int(want[q].max()) + 1 if len(want[q]) else 0), (name, eps, min_samples, q)


@pytest.mark.parametrize("eps", [0.95, 0.21])
@pytest.mark.parametrize("name", CASES)
def test_batched_split_equals_per_query_split(device, name, eps):
    from unscene3d_amd.trainer import postprocess as PP

    xyz, masks = _on_device(name, device)
    cls = torch.randn(masks.shape[1], 3, generator=torch.Generator().manual_seed(1)).to(device)
    want_masks, want_logits = PP.dbscan_split(masks, cls, xyz, eps)
    got_masks, got_logits = PP.dbscan_split_batched(masks, cls, xyz, eps, min_points=1)
    assert got_masks.shape[1] > 0
    assert torch.equal(got_masks, want_masks) and torch.equal(got_logits, want_logits)


def test_all_noise_query_yields_no_column_and_empty_split(device):
    from unscene3d_amd.trainer import postprocess as PP

    xyz, masks = _on_device("blobs", device)
    cls = torch.randn(masks.shape[1], 3, generator=torch.Generator().manual_seed(1)).to(device)
    new_masks, new_logits = PP.dbscan_split_batched(masks[:, :3].contiguous(), cls[:3], xyz, 0.3, min_points=10)
    want = DC.sklearn_labels("blobs", 0.3, 10)
    assert new_masks.shape[1] == int(want[1].max()) + 1 and len(want[0]) == 0 and (want[2] == -1).all()
    assert torch.equal(new_logits, cls[1:2].expand(new_masks.shape[1], -1))
    empty_masks, empty_logits = PP.dbscan_split_batched(masks[:, 2:3].contiguous(), cls[2:3], xyz, 0.3, min_points=10)
    assert empty_masks.shape == (masks.shape[0], 0) and empty_logits.shape == (0, 3)


def test_export_golden_through_the_batched_split(device, monkeypatch):
    """The recorded reference export with use_dbscan; the per-query route must not be what runs."""
    import test_export as TE
    from unscene3d_amd.trainer import postprocess as PP

    def forbidden(*a, **k):
        raise AssertionError("export_instances took the per-query split on device tensors")

    monkeypatch.setattr(PP, "dbscan_split", forbidden)
    scenes, general = TE._load(np.load(TE.GOLD), "dbscan")
    TE._check(TE._run(scenes, general, device), scenes)


def test_export_with_min_points_4_equals_export_from_sklearn_labels(device, monkeypatch):
    import test_export as TE
    from sklearn.cluster import DBSCAN
    from unscene3d_amd.trainer import postprocess as PP

    scenes, general = TE._load(np.load(TE.GOLD), "dbscan")
    general.dbscan_min_points = 4
    got = TE._run(scenes, general, device)
    seen = []

    def split_from_sklearn(masks, logits, coords, eps, min_points=1):
        seen.append(min_points)
        m, xyz = masks.cpu().numpy(), coords.cpu().numpy().astype(np.float64)
        cols, rows = [], []
        for q in range(m.shape[1]):
            on = m[:, q] > 0
            if not on.any():
                continue
            lab = np.full(len(m), -1)
            lab[on] = DBSCAN(eps=eps, min_samples=min_points).fit(xyz[on]).labels_
            for c in range(lab.max() + 1):
                cols.append(np.where(lab == c, m[:, q], 0).astype(np.float32))
                rows.append(q)
        return (torch.from_numpy(np.stack(cols, 1)).to(masks.device),
                logits.index_select(0, torch.as_tensor(rows, device=logits.device)))

    monkeypatch.setattr(PP, "dbscan_split_batched", split_from_sklearn)
    want = TE._run(scenes, general, device)
    assert seen == [4, 4]
    for g, w in zip(got, want):
        assert torch.equal(g["pred_masks"], w["pred_masks"]) and g["pred_masks"].shape[1] > 0
        assert np.array_equal(g["pred_scores"], w["pred_scores"])
        assert np.array_equal(np.asarray(g["pred_classes"]), np.asarray(w["pred_classes"]))
        assert np.array_equal(g["pred_boxes"], w["pred_boxes"])


@pytest.mark.parametrize("eps, min_samples", [(0.21, 1), (0.3, 4)])
def test_two_runs_give_identical_bytes(device, eps, min_samples):
    from unscene3d_amd import ops

    xyz, logits = _on_device("blobs", device)
    a = ops.dbscan_masks(xyz, logits, eps, min_samples)
    b = ops.dbscan_masks(xyz, logits, eps, min_samples)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bad_arguments_raise(device):
    from unscene3d_amd import ops

    xyz, logits = _on_device("wide", device)
    bad = xyz.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.dbscan_masks(bad, logits, 0.95)
    bad[7, 1] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.dbscan_masks(bad, logits, 0.95)
    with pytest.raises(RuntimeError, match="eps"):
        ops.dbscan_masks(xyz, logits, 0.0)
    with pytest.raises(RuntimeError, match="min_samples"):
        ops.dbscan_masks(xyz, logits, 0.95, 0)
    far = xyz.clone()
    far[0, 0] = 1.0e6
    with pytest.raises(RuntimeError, match="cells"):
        ops.dbscan_masks(far, logits, 0.21)


def test_no_quadratic_buffer_and_large_scene_equals_per_query(device):
    """About 20 000 lattice voxels: the additional peak memory of dbscan_masks stays below 64 N Q bytes (labels, bit
    rows and per-cell tables fit in that, an [N,N] table of any type does not: N > 64 Q), and cells holding several
    hundred points give the labels of the per-query route."""
    from unscene3d_amd import ops

    xyz, logits = DC.lattice_scene()
    N, Q = logits.shape
    assert 18000 <= N <= 22000 and N > 64 * Q
    xyz_d, masks = torch.from_numpy(xyz).to(device), torch.from_numpy(logits).to(device)
    ops.dbscan_masks(xyz_d[:64].contiguous(), masks[:64].contiguous(), 0.95)      # load kernels outside the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, n_clusters = ops.dbscan_masks(xyz_d, masks, 0.95, 1)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"dbscan_masks N={N} Q={Q}: additional peak {extra} bytes, bound {64 * N * Q}")
    assert extra < 64 * N * Q
    for q in (0, 1, 2, 5):
        on = masks[:, q] > 0
        want = ops.cc_eps(xyz_d[on].contiguous(), 0.95)
        assert torch.equal(labels[on, q].long(), want)
        assert int(n_clusters[q]) == int(want.max()) + 1
    noisy = ops.dbscan_masks(xyz_d, masks, 0.95, 4)[0]
    assert torch.equal(noisy, labels)                    # on a 2 cm lattice every on-point has 4 neighbours within eps
