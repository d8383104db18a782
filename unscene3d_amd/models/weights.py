"""Published checkpoints -> the backbones of this package (reference utils/utils.py:146-192
`load_state_with_same_shape`, pseudo_masks/unscene3d_pseudo_main.py:55-68).

The CSC (Contrastive Scene Contexts) Res16UNet34C checkpoints the reference's pseudo-mask scripts use are files of
`{"state_dict": {...}}` whose keys carry the wrapper they were trained in (`module.` of DataParallel, `model.` of a
Lightning module, `encoder.`), and whose `final` layer is sized for the label set of their own task.  Module names here
equal the reference's (models/res16unet.py), so after the prefixes are gone the keys match; what does not match in name
or shape is reported and left at its initial value — never raised, as in the reference."""
from __future__ import annotations

import logging
from types import SimpleNamespace

import torch

log = logging.getLogger(__name__)
WRAPPER_PREFIXES = ("module.", "model.", "encoder.")


def load_state_with_same_shape(model, weights, prefix=""):
    """The tensors of `weights` that `model` can take -> (matched {key: tensor}, report).

    As utils/utils.py:146-192: a `module.`, a `model.` and an `encoder.` prefix are stripped, in this order, each when the
    FIRST key starts with it (`k.partition(p)[2]` on every key, like the reference), then an explicit `prefix`; a tensor
    is kept when its key exists in `model.state_dict()` with the same shape.  The reference's two branches for a
    checkpoint of a whole 2D+3D Lightning module (`model_3d.` / `model_2d.` keys) are not carried over: no model of this
    package has such keys.
    report: {"loaded": [...], "missing": [...] (keys of the model no tensor was found for), "shape_mismatch": [...],
    "unexpected": [...] (keys of the checkpoint the model does not have)}, each in the order of its source."""
    state = model.state_dict()
    weights = dict(weights)
    for p in WRAPPER_PREFIXES + ((prefix,) if prefix else ()):
        if weights and (p == prefix or next(iter(weights)).startswith(p)):
            weights = {k.partition(p)[2]: v for k, v in weights.items()}
    matched, mismatch, unexpected = {}, [], []
    for k, v in weights.items():
        if k not in state:
            unexpected.append(k)
        elif tuple(v.shape) != tuple(state[k].shape):
            mismatch.append(k)
        else:
            matched[k] = v
    report = {"loaded": list(matched), "missing": [k for k in state if k not in matched and k not in mismatch],
              "shape_mismatch": mismatch, "unexpected": unexpected}
    log.info("loading weights for %d/%d tensors (%d of another shape, %d unknown)", len(matched), len(state),
             len(mismatch), len(unexpected))
    return matched, report


def load_csc_backbone(path_or_state, in_channels=3, num_labels=20, conv1_kernel_size=3, bn_momentum=0.02, device="cuda",
                      prefix=""):
    """The frozen 3D feature extractor of the pseudo-mask path (unscene3d_pseudo_main.py:55-68):
    `Res16UNet34CMultiRes(in_channels, num_labels, config.net)` with the tensors of a CSC checkpoint that fit, in eval mode
    on `device`.  path_or_state: a file `torch.load` reads, or the loaded object; either `{"state_dict": {...}}` or the
    state dict itself.  The defaults are the reference's config.net (conv1_kernel_size 3, bn_momentum 0.02) and ScanNet's
    20 labels; a checkpoint whose `final` layer has another label count keeps this model's own `final` (its output is
    not used by `encode_scene_feats_3d`).
    -> the model; `model.load_report` is the report of `load_state_with_same_shape`."""
    from .res16unet import Res16UNet34CMultiRes

    state = path_or_state
    if not isinstance(state, dict):
        state = torch.load(state, map_location="cpu")
    if "state_dict" in state:
        state = state["state_dict"]
    cfg = SimpleNamespace(bn_momentum=bn_momentum, conv1_kernel_size=conv1_kernel_size, dilations=[1, 1, 1, 1])
    model = Res16UNet34CMultiRes(in_channels, num_labels, cfg)
    matched, report = load_state_with_same_shape(model, state, prefix=prefix)
    full = model.state_dict()
    full.update(matched)
    model.load_state_dict(full)
    model.load_report = report
    for kind in ("missing", "shape_mismatch", "unexpected"):
        if report[kind]:
            log.warning("load_csc_backbone: %d %s keys, e.g. %s", len(report[kind]), kind.replace("_", "-"),
                        report[kind][0])
    return model.to(device).eval()
