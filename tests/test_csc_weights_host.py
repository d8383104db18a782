"""CPU: published CSC checkpoints load as they are (unscene3d_amd/models/weights.py; reference utils/utils.py:146-192,
pseudo_masks/unscene3d_pseudo_main.py:60-68): wrapper prefixes are stripped, tensors of the same name and shape are
taken bit for bit, everything else is reported and left alone — nothing raises."""
from types import SimpleNamespace

import pytest
import torch

WRONG_SHAPE, UNKNOWN = "block1.0.conv1.kernel", "projection_head.weight"


def _model(seed, labels=20):
    from unscene3d_amd.models.res16unet import Res16UNet34CMultiRes
    torch.manual_seed(seed)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    return Res16UNet34CMultiRes(3, labels, cfg)


@pytest.fixture(scope="module")
def source():
    """The state of a backbone trained for 41 labels, with one tensor of another shape and one unknown key."""
    state = {k: v.clone() for k, v in _model(1, labels=41).state_dict().items()}
    assert WRONG_SHAPE in state
    state[WRONG_SHAPE] = torch.zeros(tuple(state[WRONG_SHAPE].shape) + (2,))
    state[UNKNOWN] = torch.ones(4, 4)
    return state


@pytest.mark.parametrize("prefix", ["", "module.", "model.", "encoder.", "module.model.encoder."])
def test_load_csc_backbone_takes_what_fits_and_reports_the_rest(tmp_path, source, prefix):
    from unscene3d_amd.models.weights import load_csc_backbone

    path = str(tmp_path / "csc.pth")
    torch.save({"state_dict": {prefix + k: v for k, v in source.items()}, "epoch": 3}, path)
    torch.manual_seed(2)
    model = load_csc_backbone(path, device="cpu")
    initial = _model(2).state_dict()                            # what the constructor gave before loading
    assert not model.training
    got, rep = model.state_dict(), model.load_report
    left = [k for k in got if k.startswith("final.")] + [WRONG_SHAPE]
    assert sorted(rep["shape_mismatch"]) == sorted(left)
    assert rep["unexpected"] == [UNKNOWN] and rep["missing"] == []
    assert sorted(rep["loaded"]) == sorted(k for k in got if k not in left)
    assert len(rep["loaded"]) > 300
    for k, v in got.items():
        want = initial[k] if k in left else source[k]
        assert v.dtype == want.dtype and torch.equal(v, want), k


def test_explicit_prefix_and_plain_state_dict(source):
    from unscene3d_amd.models.weights import load_csc_backbone, load_state_with_same_shape

    model = load_csc_backbone({"backbone." + k: v for k, v in source.items()}, num_labels=41, device="cpu",
                              prefix="backbone.")
    assert model.load_report["shape_mismatch"] == [WRONG_SHAPE]
    assert torch.equal(model.state_dict()["final.kernel"], source["final.kernel"])
    matched, rep = load_state_with_same_shape(_model(3), {"bn0.bn.weight": torch.zeros(32)})
    assert list(matched) == ["bn0.bn.weight"] == rep["loaded"] and "conv0p1s1.kernel" in rep["missing"]
