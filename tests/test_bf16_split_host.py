"""CPU: the arithmetic of the split-bf16 training precision (tests/bf16_split_ref.py, the oracle of
tests/test_gpu_bf16_split.py) and its switches (unscene3d_amd/precision.py, general.train_precision)."""
import ctypes

import numpy as np
import pytest

from bf16_ref import bf16_round
from bf16_split_ref import kept_pairs, split_bits, split_conv_ref, split_planes
from unscene3d_amd.precision import TRAIN_PRECISIONS      # the plane counts under test are the ones the package ships

PLANES = [int(p[-1]) for p in TRAIN_PRECISIONS if p != "f32"]


def _data():
    rng = np.random.default_rng(11)
    n = 200_000
    gauss = rng.standard_normal(n).astype(np.float32)
    wide = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))).astype(np.float32)
    relu = np.maximum(rng.standard_normal(n), 0).astype(np.float32)
    return {"gauss": gauss, "wide": wide, "relu": relu}


DATA = _data()


@pytest.mark.parametrize("kind", sorted(DATA))
def test_three_planes_sum_back_exactly_and_each_plane_is_bf16(kind):
    a = DATA[kind]
    assert PLANES == [2, 3]
    p = split_planes(a, 3)
    assert np.array_equal(bf16_round(p), p)                                   # every plane is a bf16 value
    assert np.array_equal((p[0].astype(np.float64) + p[1] + p[2]), a.astype(np.float64))
    assert np.array_equal(split_planes(a, 2), p[:2])
    nz = a != 0
    assert (np.abs(p[1][nz]) <= 2.0 ** -8 * np.abs(a[nz])).all() and (np.abs(p[2][nz]) <= 2.0 ** -16 * np.abs(a[nz])).all()


def test_non_finite_first_plane_zeroes_the_others():
    a = np.array([np.inf, -np.inf, 3.4e38, -3.4e38, np.nan, 1.0], np.float32)
    p = split_planes(a, 3)
    assert 3 in PLANES
    assert np.isinf(p[0][:4]).all() and np.isnan(p[0][4]) and (p[1:, :5] == 0).all() and p[0][5] == 1
    assert split_bits(a, 3).dtype == np.uint16


@pytest.mark.parametrize("P", PLANES)
def test_kept_products_are_exact_and_the_dropped_ones_are_bounded(P):
    """Every kept product is exact in f32; per product, kept sum against the float64 product of the unsplit operands:
    <= 2^-23 |x||w| (P = 3), <= 3 * 2^-16 |x||w| (P = 2) — the derived bounds (|x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|).
    Measured here: 2^-24.4 and 2^-15.2."""
    worst = 0.0
    for kx, kw in (("gauss", "gauss"), ("wide", "gauss"), ("relu", "wide")):
        x, w = DATA[kx], DATA[kw][::-1]
        xp, wp = split_planes(x, P), split_planes(w, P)
        kept = np.zeros(x.shape, np.float64)
        for i, j in kept_pairs(P):
            prod64 = xp[i].astype(np.float64) * wp[j].astype(np.float64)
            assert np.array_equal((xp[i] * wp[j]).astype(np.float64), prod64)    # exact in f32
            kept += prod64
        full = x.astype(np.float64) * w.astype(np.float64)
        nz = full != 0
        worst = max(worst, float((np.abs(kept - full)[nz] / np.abs(full)[nz]).max()))
    bound = 2.0 ** -23 if P == 3 else 3 * 2.0 ** -16
    print(f"P={P}: worst per-product truncation 2^{np.log2(worst):.1f} (bound 2^{np.log2(bound):.1f})")
    assert worst <= bound
    assert sorted(kept_pairs(P)) == sorted((i, j) for i in range(P) for j in range(P) if i + j < P)


def test_oracle_is_the_sum_of_the_kept_products():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 16)).astype(np.float32)
    W = rng.standard_normal((2, 16, 32)).astype(np.float32)
    nbr = np.array([[0, 1, 2, -1, 4, 5, 6], [-1, 0, 0, 3, -1, 2, 1]], np.int32)
    for P in PLANES:
        y, mag = split_conv_ref(x, W, nbr, 7, P)
        xp, wp = split_planes(x, P).astype(np.float64), split_planes(W, P).astype(np.float64)
        want = np.zeros((7, 32))
        for k in range(2):
            for o in range(7):
                if nbr[k, o] >= 0:
                    for i, j in kept_pairs(P):
                        want[o] += xp[i][nbr[k, o]] @ wp[j][k]
        assert np.allclose(y, want, rtol=1e-14, atol=1e-14)
        full = sum(np.where((nbr[k] >= 0)[:, None], x[np.maximum(nbr[k], 0)].astype(np.float64) @ W[k].astype(np.float64), 0)
                   for k in range(2))
        assert (np.abs(y - full) <= (2.0 ** -23 if P == 3 else 3 * 2.0 ** -16) * mag).all()


def test_train_precision_is_validated():
    from unscene3d_amd.config import apply_overrides, default_config
    assert default_config().general.train_precision == "f32"
    for ok in ("f32", "bf16x2", "bf16x3"):
        assert apply_overrides(default_config(), [f"general.train_precision={ok}"]).general.train_precision == ok
    for bad in ("bf16", "fp16", "bf16x4"):
        with pytest.raises(ValueError, match="train_precision"):
            apply_overrides(default_config(), [f"general.train_precision={bad}"])


def test_training_precision_nests_and_restores():
    import torch

    import unscene3d_amd
    from unscene3d_amd import precision
    assert unscene3d_amd.training_precision is precision.training_precision
    assert precision.current_training() == "f32" and precision.TRAIN_PRECISIONS == ("f32", "bf16x2", "bf16x3")
    with pytest.raises(ValueError):
        precision.training_precision("bf16")
    W = torch.zeros((27, 96, 96))
    with precision.training_precision("bf16x3"):
        assert precision.current_training() == "bf16x3"
        with precision.training_precision("bf16x2"):
            assert precision.current_training() == "bf16x2"
            with precision.training_precision("f32"):
                assert precision.current_training() == "f32" and precision.train_planes(W, True, 1 << 30) == 0
            assert precision.current_training() == "bf16x2"
        assert precision.current_training() == "bf16x3"
        with pytest.raises(RuntimeError):
            with precision.training_precision("bf16x2"):
                raise RuntimeError("x")
        assert precision.current_training() == "bf16x3"
        # independent of the inference switch
        with precision.inference_precision("bf16"):
            assert precision.current_training() == "bf16x3" and precision.current() == "bf16"
        assert precision.current() == "f32"
    assert precision.current_training() == "f32"


def test_policy_covers_only_large_stride1_units_with_autograd(monkeypatch):
    import warnings

    import torch

    from unscene3d_amd import precision
    W = torch.zeros((27, 96, 96))
    big = max(precision.TRAIN_MIN_ROWS, 1) + (1 << 20)
    assert precision.train_planes(W, True, big) == 0                         # default precision
    monkeypatch.setattr(precision, "TRAIN_MIN_ROWS", 32768)
    monkeypatch.setattr(precision, "TRAIN_MIN_CIN", 96)
    for name, planes in (("bf16x2", 2), ("bf16x3", 3)):
        with precision.training_precision(name):
            assert precision.train_planes(W, True, 40000) == planes
            assert precision.train_planes(W, True, 32767) == 0               # below TRAIN_MIN_ROWS
            assert precision.train_planes(torch.zeros((27, 64, 96)), True, 40000) == 0        # below TRAIN_MIN_CIN
            assert precision.train_planes(torch.zeros((8, 96, 96)), False, 40000) == 0        # strided
            assert precision.train_planes(torch.zeros((1, 96, 96)), True, 40000) == 0         # K = 1
            assert precision.train_planes(torch.zeros((96, 96)), True, 40000) == 0
            with torch.no_grad():
                assert precision.train_planes(W, True, 40000) == 0           # only with autograd
    monkeypatch.setattr(precision, "TRAIN_MIN_ROWS", 0)
    monkeypatch.setattr(precision, "TRAIN_MIN_CIN", 0)
    precision.FALLBACKS.discard((27, 96, 48))
    with precision.training_precision("bf16x3"):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            assert precision.train_planes(torch.zeros((27, 96, 48)), True, 1000) == 0
            assert precision.train_planes(torch.zeros((27, 96, 48)), True, 1000) == 0
            assert precision.train_planes(torch.zeros((27, 3, 32)), True, 1000) == 0          # the stem: f32 by design
        assert sum("runs in f32" in str(r.message) for r in rec) == 1
        assert (27, 96, 48) in precision.FALLBACKS and (27, 3, 32) not in precision.FALLBACKS
        # covered forward, uncovered input gradient (48 output columns there): the whole unit stays f32, and says so
        precision.FALLBACKS.discard((27, 48, 96))
        with warnings.catch_warnings(record=True) as rec2:
            warnings.simplefilter("always")
            assert precision.train_planes(torch.zeros((27, 48, 96)), True, 1000) == 0
        assert len(rec2) == 1 and (27, 48, 96) in precision.FALLBACKS
        precision.FALLBACKS.discard((27, 48, 96))
    precision.FALLBACKS.discard((27, 96, 48))


def test_step_record_carries_the_planes_at_its_end():
    from unscene3d_amd import _lib
    assert _lib.lib.usc_step_size() == ctypes.sizeof(_lib.Step)
    assert _lib.Step._fields_[-2][0] == "split_planes" and _lib.Step.split_planes.offset > _lib.Step.cb.offset
    assert _lib.lib.usc_spconv_gather_gemm_split_ws_bytes(0, 96, 96, 27, 3) == 0
    for bad in ((96, 96, 27, 1), (96, 96, 27, 4), (8, 96, 27, 3), (96, 48, 27, 2), (96, 96, 65, 3)):
        assert _lib.lib.usc_spconv_gather_gemm_split_ws_bytes(0, *bad) == -1
    # argument validation happens before any HIP call
    assert _lib.lib.usc_split_bf16(None, 8, 5, None, None) != 0 and "P must be 2 or 3" in _lib.last_error()
    assert _lib.lib.usc_spconv_pack_w_split(None, 27, 96, 96, 3, 0, None, None) != 0 and "null pointer" in _lib.last_error()
