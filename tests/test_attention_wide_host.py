"""CPU: the ABI of the fused decoder attention for up to 256 queries — the query limit, the row stride of lse, the
workspace size (unchanged up to 128 queries, larger above) and the argument check of usc_attn_fwd, which comes before
any launch and therefore runs without a device."""
import pytest

USC_ERR_ARG = -1


def test_query_limit_and_lse_stride():
    from unscene3d_amd import _lib, ops

    lib = _lib.lib
    assert lib.usc_abi_version() >= 4
    assert lib.usc_attn_max_queries() == 256
    assert ops.ATTN_MAX_QUERIES == 256
    for L, want in ((1, 128), (128, 128), (129, 256), (256, 256)):
        assert lib.usc_attn_lse_stride(L) == want


@pytest.mark.parametrize("S,B,H", [(200, 1, 8), (3200, 2, 8), (40000, 1, 8)])
def test_workspace_depends_on_the_query_group_only(S, B, H):
    from unscene3d_amd import _lib

    lib = _lib.lib
    assert lib.usc_attn_ws_bytes(1, S, B, H) == lib.usc_attn_ws_bytes(128, S, B, H) == lib.usc_attn_ws_bytes(100, S, B, H)
    assert lib.usc_attn_ws_bytes(129, S, B, H) == lib.usc_attn_ws_bytes(256, S, B, H)
    assert lib.usc_attn_ws_bytes(129, S, B, H) > lib.usc_attn_ws_bytes(128, S, B, H)


def test_more_than_256_queries_is_an_argument_error():
    from unscene3d_amd import _lib

    rc = _lib.lib.usc_attn_fwd(None, None, None, None, 257, 200, 1, 8, 128, None, None, None, 0, None)
    assert rc == USC_ERR_ARG
    assert "256" in _lib.last_error() and "usc_attn_fwd" in _lib.last_error()


def test_switch_selects_the_decoder_limit(monkeypatch):
    from unscene3d_amd.models import mask3d

    monkeypatch.setattr(mask3d, "_FUSED_ATTN_WIDE", True)
    assert mask3d.fused_attn_max_queries() == 256
    monkeypatch.setattr(mask3d, "_FUSED_ATTN_WIDE", False)
    assert mask3d.fused_attn_max_queries() == 128
