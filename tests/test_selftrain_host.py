"""CPU: the numpy oracle of the self-training merge (selftrain_cases.py) covers every branch of the rule and agrees
with `load_self_train_masks`, which tests/golden/dataset.npz pins; `save_for_freemask(fmt="npy")` writes what it wrote
before the bit-row format existed; the new C entry points refuse bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import selftrain_cases as S


def test_every_branch_of_the_merge_occurs_in_the_cases():
    total = dict.fromkeys(S.BRANCHES, 0)
    for exp in S.merge_expectations().values():
        for b in S.BRANCHES:
            total[b] += exp["census"][b]
    assert all(total[b] > 0 for b in S.BRANCHES), total
    # and inside single runs, not only over the union: one planted run takes every in-walk branch and ends at the cap
    c = S.merge_expectations()[("planted4099", 5, 100)]["census"]
    assert c["added"] == 5 and c["empty"] >= 1 and c["tie"] >= 2 and c["less"] >= 1 and c["cap"] >= 3
    assert S.merge_expectations()[("planted256", 0, 100)]["census"]["cap"] >= 1
    for a in S.MAX_ADD:
        assert S.merge_expectations()[("planted1000", a, 0)]["picked"] == []


def test_pack_and_unpack_are_inverse_and_leave_the_tail_zero():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 130):
        m = rng.random((n, 7)) < 0.5
        bits = S.numpy_pack(m)
        assert bits.dtype == np.uint64 and bits.shape == (7, (n + 63) // 64)
        assert np.array_equal(S.numpy_unpack(bits, n), m)
        assert np.array_equal(S.numpy_popcount(bits), m.sum(0))
        if n % 64:
            assert not (bits[:, -1] >> np.uint64(n % 64)).any()
    one = np.zeros((70, 1), bool)
    one[65] = True
    assert S.numpy_pack(one)[0].tolist() == [0, 2]


@pytest.mark.parametrize("max_add", S.MAX_ADD)
def test_numpy_merge_equals_load_self_train_masks(max_add):
    """Same cloud on both sides, so the 1-NN transfer (a device kernel) is not needed: `load_self_train_masks` on the
    CPU is the host rule as shipped."""
    from unscene3d_amd.datasets.freemask import load_self_train_masks

    for name, st, cov in S.merge_cases():
        n = st.shape[0]
        pts = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
        for kp in S.KP:
            exp = S.merge_expectations()[(name, max_add, kp)]
            got = load_self_train_masks(pts, cov[:, None], pts, st[:, :kp], max_add, device="cpu")
            assert got.dtype == bool and np.array_equal(got[:, :1], cov[:, None]), name
            assert np.array_equal(got[:, 1:], exp["fresh"]), (name, max_add, kp)
            assert np.array_equal(got.any(1), exp["covered"])
            assert exp["census"]["added"] == len(exp["picked"]) == exp["fresh"].shape[1]


def test_save_for_freemask_npy_writes_the_two_files_as_before(tmp_path):
    import torch

    from unscene3d_amd.trainer.postprocess import save_for_freemask

    rng = np.random.default_rng(1)
    coords = rng.standard_normal((50, 3)).astype(np.float32)
    masks = rng.random((50, 4)) < 0.3
    save_for_freemask(str(tmp_path / "a"), "scene0000_00", coords, torch.from_numpy(masks.astype(np.float32)))
    save_for_freemask(str(tmp_path / "b"), "scene0000_00", coords, masks, fmt="npy")
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d / "freemasks")) == ["scene0000_00_cloud.npy", "scene0000_00_masks.npy"]
        got = np.load(tmp_path / d / "freemasks" / "scene0000_00_masks.npy")
        assert got.dtype == bool and np.array_equal(got, masks)
        assert np.array_equal(np.load(tmp_path / d / "freemasks" / "scene0000_00_cloud.npy"), coords)
    # byte for byte what np.save writes for the bool table and the cloud
    np.save(tmp_path / "ref_masks.npy", masks)
    np.save(tmp_path / "ref_cloud.npy", coords)
    for d in ("a", "b"):
        assert (tmp_path / d / "freemasks" / "scene0000_00_masks.npy").read_bytes() == (tmp_path / "ref_masks.npy").read_bytes()
        assert (tmp_path / d / "freemasks" / "scene0000_00_cloud.npy").read_bytes() == (tmp_path / "ref_cloud.npy").read_bytes()
    with pytest.raises(ValueError, match="fmt"):
        save_for_freemask(str(tmp_path / "c"), "scene0000_00", coords, masks, fmt="packed")


def test_freemask_format_is_a_config_key_with_the_old_default():
    from unscene3d_amd.config import apply_overrides, default_config

    assert default_config().general.freemask_format == "npy"
    assert apply_overrides(default_config(), ["general.freemask_format=bits"]).general.freemask_format == "bits"
    with pytest.raises(ValueError, match="freemask_format"):
        apply_overrides(default_config(), ["general.freemask_format=zip"])


def test_new_entry_points_refuse_bad_arguments_before_any_hip_call():
    from unscene3d_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "usc_mask_columns_to_bits": [lambda: lib.usc_mask_columns_to_bits(p, 0, 1, p, p, None),
                                     lambda: lib.usc_mask_columns_to_bits(p, 1, 0, p, p, None),
                                     lambda: lib.usc_mask_columns_to_bits(None, 1, 1, p, p, None)],
        "usc_mask_bits_gather": [lambda: lib.usc_mask_bits_gather(p, 0, p, 1, 1, p, p, None),
                                 lambda: lib.usc_mask_bits_gather(p, 1, p, 0, 1, p, p, None),
                                 lambda: lib.usc_mask_bits_gather(p, 1, None, 1, 1, p, p, None)],
        "usc_mask_bits_count": [lambda: lib.usc_mask_bits_count(p, 1, 0, p, None),
                                lambda: lib.usc_mask_bits_count(p, -1, 1, p, None),
                                lambda: lib.usc_mask_bits_count(None, 1, 1, p, None)],
        "usc_selftrain_merge": [lambda: lib.usc_selftrain_merge(p, p, -1, 1, p, 1, p, p, p, None),
                                lambda: lib.usc_selftrain_merge(p, p, 1, 0, p, 1, p, p, p, None),
                                lambda: lib.usc_selftrain_merge(p, p, 1, 1, p, -1, p, p, p, None),
                                lambda: lib.usc_selftrain_merge(p, p, 1, 1, None, 1, p, p, p, None),
                                lambda: lib.usc_selftrain_merge(p, None, 1, 1, p, 1, p, p, p, None),
                                lambda: lib.usc_selftrain_merge(p, p, 1, 1, p, 1, None, p, p, None)],
        "usc_mask_bits_to_columns": [lambda: lib.usc_mask_bits_to_columns(p, p, 1, -1, p, 1, 0, None),
                                     lambda: lib.usc_mask_bits_to_columns(p, p, 2, 1, p, 1, 0, None),
                                     lambda: lib.usc_mask_bits_to_columns(p, p, 1, 1, p, 2, -1, None),
                                     lambda: lib.usc_mask_bits_to_columns(p, None, 1, 1, p, 1, 0, None)],
        "usc_mask_bits_to_columns_u8": [lambda: lib.usc_mask_bits_to_columns_u8(p, p, 1, 1, p, 1, 1, None),
                                        lambda: lib.usc_mask_bits_to_columns_u8(None, p, 1, 1, p, 1, 0, None)],
    }
    for name, bad in calls.items():
        for call in bad:
            assert call() == -1
            assert _lib.last_error().startswith(name + ":"), _lib.last_error()
    # the size knob: clamped to the default, a negative value only reads it
    default = lib.usc_selftrain_merge_lds_words(-1)
    assert default == 7168
    assert lib.usc_selftrain_merge_lds_words(0) == default and lib.usc_selftrain_merge_lds_words(1 << 30) == 0
    assert lib.usc_selftrain_merge_lds_words(-1) == default
