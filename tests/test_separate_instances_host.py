"""CPU: `general.separate_instances` without a device.  The numpy restatement tests/separate_ref.py reproduces the parts
the reference's own `separate_segments` gave on the planted scene (tests/golden/separate_instances.npz, written by
tests/golden/make_golden_separate.py); `segment_adjacency(mutual=True)` on CPU tensors equals the restatement's
adjacency and `mutual=False` is the call without the keyword; the configuration keys, the argument checks that come
before any launch, and rule 6 (the flag without the overlap filter does nothing and warns once)."""
import os
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import separate_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "separate_instances.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def reference_part_sets(z, j):
    ids, off = z["ref_part_ids"], z["ref_part_off"]
    return {tuple(ids[off[r]:off[r + 1]]) for r in np.nonzero(z["ref_src"] == j)[0]}


def test_planted_scene_is_what_the_generator_describes(golden):
    z = golden
    uniq = np.unique(z["seg"])
    assert len(z["seg"]) == 1200 and len(uniq) == 80 and not np.array_equal(uniq, np.arange(80))
    assert z["masks"].shape == (1200, 6) and z["masks"].any(0).all()
    assert np.bincount(z["ref_src"]).tolist()[:5] == [2, 2, 1, 1, 1]
    half = z["masks"][:, 3] & (z["seg"] == uniq[50])
    assert 0 < half.sum() < (z["seg"] == uniq[50]).sum()               # a partly covered segment


def test_restatement_reproduces_the_reference_parts(golden):
    z = golden
    cols, src, parts, uniq = R.separate_ref(z["masks"], z["seg"], z["conn"])
    for j in range(z["masks"].shape[1]):
        mine = {tuple(uniq[p]) for p, s in zip(parts, src) if s == j}
        assert mine == reference_part_sets(z, j), j
    # the same columns as the reference's np.isin, instance by instance, as sets
    assert cols.shape == z["ref_masks"].shape
    for j in range(z["masks"].shape[1]):
        a = {c.tobytes() for c in cols[:, src == j].T}
        b = {c.tobytes() for c in z["ref_masks"][:, z["ref_src"] == j].T}
        assert a == b, j
    # rule 4's order: ascending smallest segment index inside an instance; instances ascending
    assert (np.diff(src) >= 0).all()
    roots = np.array([p.min() for p in parts])
    assert all((np.diff(roots[src == j]) > 0).all() for j in range(z["masks"].shape[1]))
    # the partly covered segment comes back whole
    assert (cols[:, src == 3].any(1) & ~z["masks"][:, 3]).sum() > 0


def test_restatement_on_the_triple_bridge_gives_true_components():
    """Deviation: a segment that joins three blobs leaves two of them apart in the reference's scan (pop, then advance);
    the restatement, like the device path, gives one part."""
    ids = np.arange(7)
    pairs = [(0, 6), (2, 6), (4, 6), (0, 1), (2, 3), (4, 5)]
    conn = np.array(pairs + [(b, a) for a, b in pairs])
    adj = R.mutual_adjacency(conn, ids)
    assert (R.components(np.ones(7, bool), adj) == 0).all()


CONN_CASES = {
    "mixed": np.array([[10, 20], [20, 10], [30, 10], [40, 30], [30, 40], [20, 20], [20, 99], [99, 20], [60, 50], [50, 60],
                       [50, 60], [5, 60]], np.int64),
    "one_way_only": np.array([[10, 20], [20, 30], [30, 40]], np.int64),
    "empty": np.zeros((0, 2), np.int64),
}


@pytest.mark.parametrize("name", sorted(CONN_CASES))
def test_segment_adjacency_mutual_on_cpu_tensors(name):
    from unscene3d_amd.pseudo_masks import freemask as fm

    ids = np.array([10, 20, 30, 40, 50, 60], np.int64)
    conn = CONN_CASES[name]
    off, adj = fm.segment_adjacency(torch.from_numpy(conn), torch.from_numpy(ids), mutual=True)
    want_off, want_adj = R.adjacency_csr(R.mutual_adjacency(conn, ids))
    assert off.dtype == torch.int64 and adj.dtype == torch.int32
    assert off.tolist() == want_off.tolist() and adj.tolist() == want_adj.tolist()
    if name == "mixed":
        assert off.tolist() == [0, 1, 2, 3, 4, 5, 6] and adj.tolist() == [1, 0, 3, 2, 5, 4]
    # the default is today's call, bit for bit
    off0, adj0 = fm.segment_adjacency(torch.from_numpy(conn), torch.from_numpy(ids))
    off1, adj1 = fm.segment_adjacency(torch.from_numpy(conn), torch.from_numpy(ids), mutual=False)
    assert torch.equal(off0, off1) and torch.equal(adj0, adj1) and adj0.dtype == adj1.dtype


def test_segment_adjacency_mutual_on_the_golden_scene(golden):
    from unscene3d_amd.pseudo_masks import freemask as fm

    uniq = np.unique(golden["seg"])
    off, adj = fm.segment_adjacency(torch.from_numpy(golden["conn"]), torch.from_numpy(uniq), mutual=True)
    want_off, want_adj = R.adjacency_csr(R.mutual_adjacency(golden["conn"], uniq))
    assert off.tolist() == want_off.tolist() and adj.tolist() == want_adj.tolist()
    assert int(off[10]) == int(off[9]) + 1                    # segment 9: only 8; the one-way pair to 10 is not there


def test_config_keys_and_interpolation():
    from unscene3d_amd.config import apply_overrides, default_config

    cfg = default_config()
    assert cfg.general.separate_instances is False and cfg.data.resegment_mesh is False
    assert cfg.data.segment_min_vert_num == 20
    cfg = apply_overrides(default_config(), ["general.separate_instances=true"])
    assert cfg.general.separate_instances is True and cfg.data.resegment_mesh is True
    assert apply_overrides(default_config(), ["general.num_targets=3"]).data.resegment_mesh is False
    # like the YAML's interpolation, the derived key can be overridden, either way round
    cfg = apply_overrides(default_config(), ["data.resegment_mesh=true"])
    assert cfg.data.resegment_mesh is True and cfg.general.separate_instances is False
    cfg = apply_overrides(default_config(), ["general.separate_instances=true", "data.resegment_mesh=false"])
    assert cfg.data.resegment_mesh is False and cfg.general.separate_instances is True


def test_arguments_are_checked_before_any_launch():
    from unscene3d_amd.trainer.separate import separate_instances

    masks = torch.zeros((8, 2), dtype=torch.bool)
    with pytest.raises(RuntimeError, match="HIP"):             # CPU tensor: no device path, nothing launched
        separate_instances(masks, np.zeros(8, np.int64), np.zeros((0, 2), np.int64))
    with pytest.raises(RuntimeError, match="bool or uint8"):
        separate_instances(masks.float(), np.zeros(8, np.int64), np.zeros((0, 2), np.int64))


def test_flag_without_overlap_filter_does_nothing_and_warns_once(monkeypatch):
    import test_export as TE
    from unscene3d_amd.trainer import postprocess as PP

    TE._cpu_row_ops(monkeypatch)
    scenes, general = TE._load(np.load(TE.GOLD), "plain")
    assert not general.filter_out_instances
    base = TE._run(scenes, general, "cpu")
    flagged = NS(**vars(general), separate_instances=True)
    monkeypatch.setattr(PP, "_warned_separate", False)
    with pytest.warns(UserWarning, match="filter_out_instances"):
        again = TE._run(scenes, flagged, "cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # the second call is silent
        TE._run(scenes, flagged, "cpu")
    for a, b in zip(base, again):
        assert torch.equal(a["pred_masks"], b["pred_masks"]) and np.array_equal(a["pred_scores"], b["pred_scores"])
        assert torch.equal(a["pred_classes"], b["pred_classes"]) and np.array_equal(a["pred_boxes"], b["pred_boxes"])


def test_flag_off_or_no_connectivity_is_todays_result_on_the_host_logic(monkeypatch):
    """With the filter on, the flag on and no connectivity (None, [] or a list of empties) nothing is split and the
    device path is never entered (these are CPU tensors)."""
    import test_export as TE
    from unscene3d_amd.trainer import postprocess as PP

    TE._cpu_row_ops(monkeypatch)
    scenes, general = TE._load(np.load(TE.GOLD), "freemask")
    assert general.filter_out_instances
    base = TE._run(scenes, general, "cpu")
    flagged = NS(**vars(general), separate_instances=True)
    real = PP.export_instances
    for conn in (None, [], [[], []], [np.zeros((0, 2), np.int64)] * 2):
        monkeypatch.setattr(PP, "export_instances", lambda *a, _c=conn, **k: real(*a, segment_connectivity=_c, **k))
        again = TE._run(scenes, flagged, "cpu")
        for a, b in zip(base, again):
            assert torch.equal(a["pred_masks"], b["pred_masks"]) and np.array_equal(a["pred_scores"], b["pred_scores"])
            assert torch.equal(a["pred_classes"], b["pred_classes"])
            assert np.array_equal(a["pred_boxes"], b["pred_boxes"])
