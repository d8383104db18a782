"""CPU side of the opt-in bf16 inference precision (unscene3d_amd/precision.py, csrc/spconv_bf16.hip): the C ABI of
the new entry points, the public switch, the config key and the rounding oracle the GPU tests compare against."""
import ctypes

import numpy as np
import pytest
import torch

from bf16_ref import bf16_bits, bf16_round

NEW = ("usc_spconv_pack_w_bf16", "usc_cast_bf16", "usc_spconv_gather_gemm_bf16_ws_bytes", "usc_spconv_gather_gemm_bf16",
       "usc_unit_bf16_ws_bytes", "usc_conv_bn_act_forward_bf16")


def test_new_entry_points_are_declared_bound_and_exported():
    import os
    import re

    from unscene3d_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "usc3d.h")).read(), flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(so, name), name
    assert "USC_STEP_UNIT_FWD_BF16 = 5" in header
    assert _lib.STEP_UNIT_FWD_BF16 == 5
    assert _lib.lib.usc_step_size() == ctypes.sizeof(_lib.Step)          # the step layout did not change


def test_shape_query_and_argument_checks_without_a_device():
    from unscene3d_amd import _lib, precision
    lib = _lib.lib
    for K, cin, cout in ((27, 32, 32), (27, 96, 96), (8, 256, 256), (8, 384, 256), (1, 192, 96), (27, 16, 32)):
        assert lib.usc_spconv_gather_gemm_bf16_ws_bytes(1000, cin, cout, K) >= 0, (K, cin, cout)
        assert precision.shape_ok(K, cin, cout)
    for K, cin, cout in ((27, 3, 32), (27, 24, 32), (27, 96, 48), (65, 32, 32)):
        assert lib.usc_spconv_gather_gemm_bf16_ws_bytes(1000, cin, cout, K) < 0, (K, cin, cout)
        assert not precision.shape_ok(K, cin, cout)
    # refused before any HIP call
    assert lib.usc_spconv_gather_gemm_bf16(None, 10, 96, None, 27, 48, None, 10, None, None, 0, None, 0, None) == -1
    assert "shape not covered" in _lib.last_error()
    assert lib.usc_spconv_pack_w_bf16(None, 27, 3, 32, None, None) == -1
    assert "usc_spconv_pack_w_bf16" in _lib.last_error()


def test_inference_precision_rejects_unknown_values_and_restores_the_previous_one():
    import unscene3d_amd
    from unscene3d_amd import precision
    for bad in ("fp16", "bfloat16", "", None, 16):
        with pytest.raises(ValueError):
            unscene3d_amd.inference_precision(bad)
    assert precision.current() == "f32"
    with unscene3d_amd.inference_precision("bf16"):
        assert precision.current() == "bf16"
        with torch.no_grad():
            assert precision.bf16_active()
        assert not precision.bf16_active()                  # autograd on: always f32
        with unscene3d_amd.inference_precision("f32"):
            assert precision.current() == "f32"
        assert precision.current() == "bf16"
    assert precision.current() == "f32"
    with pytest.raises(RuntimeError):
        with unscene3d_amd.inference_precision("bf16"):
            raise RuntimeError("boom")
    assert precision.current() == "f32"


def test_eval_precision_config_key_round_trips():
    from unscene3d_amd.config import apply_overrides, default_config
    assert default_config().general.eval_precision == "f32"
    assert apply_overrides(default_config(), ["general.eval_precision=bf16"]).general.eval_precision == "bf16"
    assert apply_overrides(default_config(), ["general.eval_precision=f32"]).general.eval_precision == "f32"
    with pytest.raises(ValueError):
        apply_overrides(default_config(), ["general.eval_precision=fp16"])


def _torch_bits(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_numpy_rne_rounding_agrees_with_torch_bfloat16():
    f = np.float32
    tiny = np.finfo(np.float32).tiny
    edge = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf,
            # ties: exactly half an ulp of bf16 -> to even (down from an even, up from an odd mantissa)
            np.uint32(0x3F808000).view(f), np.uint32(0x3F818000).view(f), np.uint32(0xBF808000).view(f),
            np.uint32(0x3F808001).view(f), np.uint32(0x3F807FFF).view(f),
            # subnormals, the smallest normal, the largest finite and the overflow to inf
            np.uint32(0x00000001).view(f), np.uint32(0x00008000).view(f), np.uint32(0x00018000).view(f),
            np.uint32(0x807FFFFF).view(f), tiny, -tiny, np.finfo(np.float32).max, np.uint32(0x7F7F8000).view(f),
            np.uint32(0x7F7FFFFF).view(f), np.uint32(0xFF7FFFFF).view(f)]
    rng = np.random.default_rng(0)
    rand = rng.standard_normal(100_000).astype(np.float32) * np.exp2(rng.integers(-140, 120, 100_000)).astype(np.float32)
    vals = np.concatenate([np.asarray(edge, np.float32), rand, rng.integers(0, 2**32, 100_000, dtype=np.uint64)
                           .astype(np.uint32).view(np.float32)])
    finite_or_inf = ~np.isnan(vals)
    assert np.array_equal(bf16_bits(vals)[finite_or_inf], _torch_bits(vals)[finite_or_inf])
    nan = np.array([np.nan, -np.nan, np.uint32(0x7F800001).view(f), np.uint32(0xFFC12345).view(f)], np.float32)
    assert np.isnan(bf16_round(nan)).all() and np.isnan(torch.from_numpy(nan).to(torch.bfloat16).float().numpy()).all()
    # rounded values are fixed points and sit on the bf16 grid
    r = bf16_round(vals[finite_or_inf])
    assert np.array_equal(bf16_round(r).view(np.uint32), r.view(np.uint32))
    assert not (r.view(np.uint32) & 0xFFFF).any()
