"""CPU: usc_attn_mask_rows refuses what it does not cover — pooling depths outside 1..4, query counts that are no multiple
of 4 or above 128, more than 16 scenes, null tables — with the library's argument error, before any launch (so without
a device); the workspace size; and the hand-built tree of the GPU test makes the summation order visible."""
import ctypes

import pytest

import attn_mask_rows_cases as cases

USC_ERR_ARG = -1
PTR = 0x10000          # never dereferenced: every call here is refused before the launch


def _call(d=2, q=100, ld=128, B=1, K=8, tabs="ok", n_valid=None, logits=PTR):
    from unscene3d_amd import _lib

    nt = max(1, min(d, 4))
    if tabs == "ok":
        tabs = (ctypes.c_void_p * nt)(*([PTR] * nt))
    rows = (ctypes.c_int64 * nt)(*([64] * nt))
    nv = (ctypes.c_int32 * max(B, 1))(*(n_valid or [K] * max(B, 1)))
    rc = _lib.lib.usc_attn_mask_rows(logits, ld, q, d, tabs, rows, PTR, B, K, nv, PTR, PTR, 1 << 20, 0, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("d", [0, 5, -1])
def test_depth_outside_1_to_4(d):
    rc, msg = _call(d=d)
    assert rc == USC_ERR_ARG and "usc_attn_mask_rows" in msg and "pooling steps" in msg


@pytest.mark.parametrize("q", [0, 3, 99, 102, 130, 132, 256])
def test_query_counts(q):
    rc, msg = _call(q=q, ld=256)
    assert rc == USC_ERR_ARG and "queries" in msg


@pytest.mark.parametrize("B", [0, 17])
def test_scene_counts(B):
    rc, msg = _call(B=B)
    assert rc == USC_ERR_ARG and "scenes" in msg


def test_null_tables_and_pointers():
    rc, msg = _call(tabs=None)
    assert rc == USC_ERR_ARG and "null" in msg
    for d, hole in ((1, 0), (3, 1), (4, 3)):
        tabs = (ctypes.c_void_p * d)(*[None if j == hole else PTR for j in range(d)])
        rc, msg = _call(d=d, tabs=tabs)
        assert rc == USC_ERR_ARG and f"child table {hole} is null" in msg
    rc, msg = _call(logits=None)
    assert rc == USC_ERR_ARG and "null" in msg


def test_leading_dimension_alignment_and_empty_scene():
    assert _call(ld=98)[0] == USC_ERR_ARG and _call(ld=102)[0] == USC_ERR_ARG        # below q; no multiple of 4
    assert _call(logits=PTR + 4)[0] == USC_ERR_ARG                                    # 16-byte rows
    rc, msg = _call(B=2, n_valid=[8, 0])
    assert rc == USC_ERR_ARG and "without rows" in msg


def test_workspace_bytes():
    from unscene3d_amd import _lib

    ws = _lib.lib.usc_attn_mask_rows_ws_bytes
    assert ws(1, 200, 100, 0) == -1 and ws(1, 200, 100, 5) == -1
    # one row of q bytes per workgroup and scene; 64 / 16 / 4 / 1 keys per workgroup at depth 1 / 2 / 3 / 4
    assert [ws(2, 37, 100, d) for d in (1, 2, 3, 4)] == [2 * n * 100 for n in (1, 3, 10, 37)]


def test_wrapper_refuses_what_the_entry_refuses():
    import torch
    from unscene3d_amd import ops

    t = [torch.zeros((8, 4), dtype=torch.int32)]
    assert not ops.attn_mask_rows_applies(torch.zeros(5, 100), t, 1)                  # not on the device
    with pytest.raises(RuntimeError, match="attn_mask_rows"):
        ops.attn_mask_rows(torch.zeros(5, 100), t, torch.zeros(8, dtype=torch.int64), 1, 8, [4])


def test_the_hand_built_tree_pins_the_summation_order():
    logits, tabs = cases.order_tree()
    assert tabs[0].shape == (8, 9) and tabs[1].shape == (8, 2)
    assert int((tabs[1][:, 0] >= 0).sum()) == 8 and int((tabs[1][:, 1] >= 0).sum()) == 1
    assert all(int((tabs[0][:, c] >= 0).sum()) == 8 for c in range(8)) and int((tabs[0][:, 8] >= 0).sum()) == 1
    want = cases.emulate_chain(logits, tabs)
    assert want[0].any() and not want[0].all()
    for rev in ((0,), (1,), (0, 1)):
        assert int((cases.emulate_chain(logits, tabs, reverse=rev) != want).sum()) >= 1, rev
