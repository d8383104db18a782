"""GPU: the backward pass returns the bits it returned before its end-of-pass callbacks became one helper
(ops.at_end_of_backward) and its parameter-gradient rule one function (ops._param_grads).

tests/golden/backward_bits.json holds sha256 digests over shape, dtype and bytes (test_gpu_units_bits._sha), recorded
twice on the parent commit in two separate processes (both recordings agreed on every digest).  No tolerance: the change
moved host code only; every path issues the same native calls in the same order on the same streams.  If a digest
differs, the code is wrong, not the file.

Two groups, which tests/test_gpu_units_bits.py and tests/test_gpu_decoder_bits.py do not reach:
* the per-operator path (units.ENABLED = False: ops._ConvSame / _ConvDown2 / _ConvTrUp2 / _BatchNormAct), Res16UNet14 at
  6 000 voxels on the scene and loss of `trunk_bits`, with every p.grad allocated (gradients added in place) and with
  every p.grad None (gradients handed back through autograd);
* the whole training step on the fixture and three-step loop of tests/test_gpu_early_stage.py::_three_steps (flat
  gradients, FlatAdamW with enable_early), 1 and 2 scenes, program.EARLY_STAGE on and off: the early-stage gate, the
  1x1 mask head's backward with a bias, the key samples' grad sinks and the side-stream join."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "backward_bits.json")
ARCH, VOXELS = "Res16UNet14", 6_000
GRAD_MODES = ("in-place", "autograd")
STEP_CASES = tuple((n, sw) for n in (1, 2) for sw in (1, 0))


def per_operator_bits(device, mode):
    """name -> sha256 for one forward and backward pass of the trunk on the per-operator path."""
    from test_gpu_units_bits import _scene, _sha
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import program, units
    from unscene3d_amd.models import res16unet

    coords4, feats = _scene(VOXELS, 4200 + VOXELS % 89)
    torch.manual_seed(9)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    model = getattr(res16unet, ARCH)(3, 20, cfg, out_fpn=True).to(device).train()
    saved = units.ENABLED
    units.ENABLED = False
    try:
        for p in model.parameters():
            p.grad = torch.zeros_like(p) if mode == "in-place" else None
        x = ME.SparseTensor(features=torch.from_numpy(feats).to(device), coordinates=torch.from_numpy(coords4).to(device),
                            device=device)
        assert program.usable(model, x) is None and not units.usable(x.F, None)
        out, fmaps = model(x)
        loss = sum(w * f.F.square().mean() for w, f in zip((0.5, 1.0, 1.5, 2.0, 0.25), fmaps)) + out.F.abs().mean()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        units.ENABLED = saved
    assert len(fmaps) == 5 and model.conv0p1s1.kernel.grad is not None     # (a parameter nothing reads keeps grad None)
    stats = [v for k, v in sorted(model.state_dict().items()) if "running" in k or "num_batches" in k]
    key = f"per-operator/{mode}"
    return {f"{key}/levels": _sha(*[f.F for f in fmaps]),
            f"{key}/grads": _sha(*[p.grad for _, p in sorted(model.named_parameters())]),
            f"{key}/running": _sha(*stats)}


def step_bits(device, monkeypatch, n_scenes, switch):
    """name -> sha256 for three training steps: each loss, the flat gradient after each backward, parameters and buffers
    after the third step."""
    import test_gpu_early_stage as es
    from test_gpu_units_bits import _sha
    seen, ran = es._three_steps(device, monkeypatch, n_scenes, switch)
    assert ran == (3 if switch else 0), ran
    key = f"step/{n_scenes}-scenes/early-{'on' if switch else 'off'}"
    bits = {}
    for k, (total, grads, _, _) in enumerate(seen):
        bits[f"{key}/loss-{k + 1}"] = _sha(total)
        bits[f"{key}/grad-{k + 1}"] = _sha(grads)
    bits[f"{key}/params"] = _sha(*seen[-1][2])
    bits[f"{key}/buffers"] = _sha(*seen[-1][3])
    return bits


def _names():
    names = {f"per-operator/{m}/{what}" for m in GRAD_MODES for what in ("levels", "grads", "running")}
    for n, sw in STEP_CASES:
        key = f"step/{n}-scenes/early-{'on' if sw else 'off'}"
        names |= {f"{key}/{what}-{k}" for what in ("loss", "grad") for k in (1, 2, 3)} | {f"{key}/params", f"{key}/buffers"}
    return names


def _expect(bits):
    want = json.load(open(GOLDEN))
    assert bits and set(bits) <= set(want), sorted(set(bits) - set(want))
    differ = sorted(k for k in bits if bits[k] != want[k])
    assert not differ, differ


@pytest.mark.gpu
@pytest.mark.parametrize("mode", GRAD_MODES)
def test_per_operator_path_computes_the_recorded_bits(device, mode):
    _expect(per_operator_bits(device, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("n_scenes,switch", STEP_CASES)
def test_training_steps_compute_the_recorded_bits(device, monkeypatch, n_scenes, switch):
    _expect(step_bits(device, monkeypatch, n_scenes, switch))


def test_every_recorded_case_is_still_computed():
    """Host side of the pin: the golden file's names are exactly the cases above (a case cannot drop out of the
    comparison by being renamed, and no digest was left out when the file was recorded)."""
    want = json.load(open(GOLDEN))
    assert all(len(v) == 64 for v in want.values())
    assert set(want) == _names() and len(want) == 2 * 3 + 4 * 8

