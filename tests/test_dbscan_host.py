"""CPU side of the batched DBSCAN split: the cases keep out of the band in which the reference is undefined, the
f64 restatement of sklearn's rule (dbscan_ref.py) equals sklearn on every case, the new entry points are exported and
validate their arguments before any HIP call, and export_instances refuses dbscan_min_points > 1 on CPU tensors
instead of ignoring it."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import dbscan_cases as DC
import dbscan_ref as DR

NEW_SYMBOLS = ("usc_dbscan_cell_keys", "usc_dbscan_neighbor_table", "usc_dbscan_ws_bytes", "usc_dbscan_labels",
               "usc_dbscan_expand")


@pytest.mark.parametrize("name", list(DC.cases()))
def test_cases_keep_out_of_the_band(name):
    xyz, _ = DC.cases()[name]
    for eps in sorted({e for e, _ in DC.PARAMS}):
        assert DC.band_pairs(xyz, eps) == 0, (name, eps)


def test_lattice_scene_keeps_out_of_the_band():
    """Lattice distances are 0.02 sqrt(k), k integer: the nearest to 0.95 is k = 2256 against 2256.25."""
    k = (0.95 / 0.02) ** 2
    gap = min(abs(np.sqrt(np.floor(k)) * 0.02 - 0.95), abs(np.sqrt(np.ceil(k)) * 0.02 - 0.95)) / 0.95
    assert gap > 20 * DC.BAND          # f32 rounding of coordinates below 2.5 m moves a distance by < 5e-7


@pytest.mark.parametrize("eps, min_samples", DC.PARAMS)
@pytest.mark.parametrize("name", list(DC.cases()))
def test_rule_equals_sklearn(name, eps, min_samples):
    xyz, logits = DC.cases()[name]
    want = DC.sklearn_labels(name, eps, min_samples)
    for q in range(logits.shape[1]):
        got = DR.dbscan_ref(xyz[logits[:, q] > 0], eps, min_samples)
        assert np.array_equal(got, want[q]), (name, eps, min_samples, q)


def test_cases_cover_what_they_claim():
    xyz, logits = DC.cases()["blobs"]
    assert len(xyz) % 64 != 0 and (xyz < 0).any()
    assert len(np.unique(xyz, axis=0)) < len(xyz)                                   # exact duplicates
    assert not (logits[:, 0] > 0).any() and (logits[:, 1] > 0).all()               # empty and all-on queries
    noise = DC.sklearn_labels("blobs", 0.3, 10)[2]
    assert len(noise) > 50 and (noise == -1).all()                                  # all noise: no column
    assert DC.cases()["wide"][1].shape[1] == 65 and DC.cases()["tiny"][0].shape == (1, 3)
    lab = DC.sklearn_labels("shapes", 0.3, 4)
    on4 = np.flatnonzero(DC.cases()["shapes"][1][:, 4] > 0)                          # cross, between, numbering
    chain = DC.sklearn_labels("shapes", 0.21, 1)[2][101:142]                        # after the 101 bridge points
    assert len(chain) == 41 and (chain == chain[0]).all()                           # 40 hops, one cluster
    between = lab[4][4:13]                                                          # 4 + 4 core points, then the border
    assert between[8] == between[0] != between[4]                                   # the farther, lower-numbered one
    numbering = lab[4][13:21]                                                       # P's arm first, then all of R
    assert numbering[0] > numbering[1] and len(on4) == 21


def test_new_symbols_are_exported():
    from unscene3d_amd import _lib, ops
    from unscene3d_amd.trainer import postprocess as PP

    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert callable(ops.dbscan_masks) and callable(ops.dbscan_expand) and callable(PP.dbscan_split_batched)
    assert _lib.lib.usc_dbscan_ws_bytes(1000, 4, 10, 1) > 0
    assert _lib.lib.usc_dbscan_ws_bytes(1000, 4, 10, 4) > _lib.lib.usc_dbscan_ws_bytes(1000, 4, 10, 1)


def _addr():
    buf = (ctypes.c_float * 1024)()            # a host address: never dereferenced, the calls fail before a launch
    return buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.mark.parametrize("what, kw", [
    ("eps = 0", dict(eps=0.0)), ("eps < 0", dict(eps=-1.0)), ("eps = nan", dict(eps=float("nan"))),
    ("eps = inf", dict(eps=float("inf"))), ("min_samples = 0", dict(ms=0)), ("n = 0", dict(n=0)), ("q = 0", dict(q=0)),
    ("more cells than points", dict(m=65)), ("null masks", dict(null=5)), ("null labels", dict(null=13)),
    ("workspace too small", dict(ws_bytes=16))])
def test_dbscan_labels_rejects_bad_arguments_without_a_device(what, kw):
    from unscene3d_amd import _lib

    buf, a = _addr()
    n, q, m, ms = kw.get("n", 64), kw.get("q", 2), kw.get("m", 3), kw.get("ms", 1)
    args = [a, a, a, a, a, a, n, q, m, kw.get("eps", 0.95), ms, a, kw.get("ws_bytes", 1 << 20), a, a, None]
    if "null" in kw:
        args[kw["null"]] = None
    assert _lib.lib.usc_dbscan_labels(*args) == -1, what
    assert "usc_dbscan_labels" in _lib.last_error()


def test_dbscan_helpers_reject_bad_arguments_without_a_device():
    from unscene3d_amd import _lib

    buf, a = _addr()
    L = _lib.lib
    for args in ((a, 8, 0.0, 0.0, 0.0, 0.0, 1, 1, 1, a, None), (a, 8, 0.95, 0.0, 0.0, 0.0, (1 << 20) + 1, 1, 1, a, None),
                 (a, 8, 0.95, float("nan"), 0.0, 0.0, 1, 1, 1, a, None), (None, 8, 0.95, 0.0, 0.0, 0.0, 1, 1, 1, a, None),
                 (a, -1, 0.95, 0.0, 0.0, 0.0, 1, 1, 1, a, None)):
        assert L.usc_dbscan_cell_keys(*args) == -1 and "usc_dbscan_cell_keys" in _lib.last_error()
    for args in ((a, -1, 1, 1, 1, a, None), (a, 4, 0, 1, 1, a, None), (None, 4, 1, 1, 1, a, None)):
        assert L.usc_dbscan_neighbor_table(*args) == -1 and "usc_dbscan_neighbor_table" in _lib.last_error()
    for args in ((a, a, a, -1, 2, 3, a, None), (a, a, a, 4, 0, 3, a, None), (a, None, a, 4, 2, 3, a, None)):
        assert L.usc_dbscan_expand(*args) == -1 and "usc_dbscan_expand" in _lib.last_error()
    assert L.usc_dbscan_ws_bytes(-1, 1, 1, 1) == -1


def test_export_on_cpu_refuses_min_points_above_one():
    from unscene3d_amd.trainer import postprocess as PP

    rng = np.random.default_rng(0)
    S, Q, N, NF = 20, 10, 200, 300
    general = NS(use_dbscan=True, dbscan_eps=0.95, dbscan_min_points=4, topk_per_image=100, filter_out_instances=True,
                 scores_threshold=0.1, iou_threshold=0.66)
    output = {"aux_outputs": [], "pred_logits": torch.randn(1, Q, 3), "pred_masks": [torch.randn(N, Q)]}
    low = [{"point2segment": torch.from_numpy(rng.integers(0, S, N))}]
    with pytest.raises(RuntimeError, match="needs the device"):
        PP.export_instances(output, low, low, [rng.integers(0, N, NF)], rng.random((N, 3)), general, num_classes=3,
                            train_on_segments=False)
