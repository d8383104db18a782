"""device_max_targets, the opt-in of the device set criterion for 33 .. 128 targets per scene, on the host: the default,
the constructor's range check and the way from the config through the trainer.  What the setting does on the device is
tests/test_gpu_criterion_wide.py."""
import pytest

from unscene3d_amd.config import apply_overrides, default_config


def _criterion(**kw):
    from unscene3d_amd.models.criterion import SetCriterion
    from unscene3d_amd.models.matcher import HungarianMatcher
    matcher = HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, cost_noise_robust=0.0, num_points=-1)
    return SetCriterion(num_classes=3, matcher=matcher, weight_dict={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0},
                        eos_coef=0.1, losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                        importance_sample_ratio=0.75, class_weights=-1, **kw)


def test_the_default_is_32_targets():
    assert _criterion().device_max_targets == 32
    assert default_config().loss.device_max_targets == 32


@pytest.mark.parametrize("n", [32, 33, 100, 128])
def test_the_constructor_keeps_a_value_in_range(n):
    assert _criterion(device_max_targets=n).device_max_targets == n


@pytest.mark.parametrize("n", [0, 31, 129, 1000, -1, 64.0, "64", None, True])
def test_the_constructor_rejects_everything_else(n):
    with pytest.raises(ValueError, match="device_max_targets"):
        _criterion(device_max_targets=n)


def test_the_trainer_hands_the_config_value_through():
    from unscene3d_amd.trainer.trainer import InstanceSegmentation
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "loss.device_max_targets=128"])
    assert InstanceSegmentation(cfg).criterion.device_max_targets == 128
    cfg = apply_overrides(default_config(), ["general.num_targets=3"])
    assert InstanceSegmentation(cfg).criterion.device_max_targets == 32
    del cfg.loss.device_max_targets                     # a config node written before the setting existed
    assert InstanceSegmentation(cfg).criterion.device_max_targets == 32
    with pytest.raises(ValueError, match="device_max_targets"):
        InstanceSegmentation(apply_overrides(default_config(), ["general.num_targets=3", "loss.device_max_targets=129"]))


def test_the_wide_entry_points_check_their_arguments_without_a_device():
    """Argument validation happens before any HIP call: 1 <= T <= max_targets, and max_targets itself in 32 .. 128."""
    from unscene3d_amd import _lib
    assert _lib.lib.usc_criterion_target_bits(None, 129, 128, 10, None, None, None) != 0
    assert "usc_criterion_target_bits" in _lib.last_error() and "1..128" in _lib.last_error()
    assert _lib.lib.usc_criterion_target_bits(None, 0, 128, 10, None, None, None) != 0
    assert _lib.lib.usc_criterion_target_bits(None, 33, 32, 10, None, None, None) != 0
    assert "1..32" in _lib.last_error()
    for m in (31, 129):
        assert _lib.lib.usc_criterion_target_bits(None, 1, m, 10, None, None, None) != 0
        assert "usc_criterion_target_bits" in _lib.last_error() and "32..128" in _lib.last_error()
    # the workspace is reused per 32-target word: above 32 targets it is the 32-target size
    ws = _lib.lib.usc_criterion_ws_bytes
    assert ws(13, 3000, 33) == ws(13, 3000, 128) == ws(13, 3000, 32) > ws(13, 3000, 16)
