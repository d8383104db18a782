"""The finest U-Net stage's backward beside the decoder's (USC3D_EARLY_STAGE): the one-launch input
gradient of the mask heads (csrc/decoder.hip: usc_linear_heads_dx), a backward range issued on the weight-gradient lane
(csrc/units.hip: usc_program_run_lane, program.early_backward), the whole training step with the switch on and off, and
a backward pass that raises between the early part and its continuation.  Everything bit for bit: the early path moves
launches to another stream and sums nothing in another order."""
from types import SimpleNamespace

import pytest
import torch

from oracle import sparse_ref as R

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -20          # tests/decoder_cases.py: |got - f64| <= BOUND * (sum of the absolute values of every term)


# ------------------------------------------------------------------------------------------- 1. heads input gradient
def _heads_case(device, L, S, Q=100, d=128):
    g = torch.Generator().manual_seed(7919 * L + S)
    Qp = Q + (-Q) % 32
    feats = torch.randn(S, d, generator=g).to(device)
    Ws, dys = [], []
    for _ in range(L):
        W = torch.zeros(Qp, d)
        W[:Q] = torch.randn(Q, d, generator=g)             # the zero-extended embeddings of models.mask3d._PaddedRows
        Ws.append(W.to(device))
        dys.append(torch.randn(S, Qp, generator=g).to(device))
    return feats, Ws, dys


def _chained(feats, Ws, dys):
    """What models.mask3d._mask_logits(chain=True) builds: every product hands the table on as its second output, the
    last one takes it plainly; d feats comes out of the chained input-gradient launches."""
    from unscene3d_amd import ops
    x = feats.clone().requires_grad_(True)
    cur, outs = x, []
    for l, W in enumerate(Ws):
        if l + 1 < len(Ws):
            out, cur = ops.linear(cur, W, passthrough=True)
        else:
            out = ops.linear(cur, W)
        outs.append(out)
    torch.autograd.backward(outs, dys)
    return x.grad


def _small_rows():
    from unscene3d_amd import ops
    return ops.SMALL_ROWS


@pytest.mark.parametrize("L", [1, 13])
@pytest.mark.parametrize("S", [1, 37, 700, "above"])
def test_heads_input_gradient_has_the_bits_of_the_chain(device, L, S):
    from unscene3d_amd import ops
    S = _small_rows() + 1 if S == "above" else S
    feats, Ws, dys = _heads_case(device, L, S)
    want = _chained(feats, Ws, dys)
    got = ops.linear_heads_dx(dys, Ws)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(ops.linear_heads_dx(dys, Ws), got)                  # and run to run
    ref = sum(dy.double() @ W.double() for dy, W in zip(dys, Ws))
    mag = sum(dy.double().abs() @ W.double().abs() for dy, W in zip(dys, Ws))
    frac = float(((got.double() - ref).abs() / (BOUND * mag + 1e-30)).max())
    print(f"heads dx L={L} S={S}: {frac:.3f} of the bound")
    assert frac <= 1.0, frac


def test_heads_input_gradient_refusals(device):
    from unscene3d_amd import ops
    from unscene3d_amd._lib import lib
    feats, Ws, dys = _heads_case(device, 2, 5)
    with pytest.raises(RuntimeError):
        ops.linear_heads_dx(dys, [Ws[0], Ws[1][:64]])
    many = int(lib.usc_linear_heads_max()) + 1
    with pytest.raises(RuntimeError, match="heads"):
        ops.linear_heads_dx([dys[0]] * many, [Ws[0]] * many)


# ------------------------------------------------------------------------------------------- 2. the lane range, native
def _scene(voxels, seed):
    from unscene3d_amd.synthetic import make_scene
    sc = make_scene(seed, target_voxels=voxels, tol=0.05)
    ec = R.voxel_floor(sc["xyz"], 0.02)
    eu, _ = R.sparse_quantize(ec)
    return R.sparse_collate([ec[eu]], [sc["colors"][eu]])


def _trunk_pass(model, coords4, feats, device, ext, early):
    """Forward, then the backward for one external gradient per level output (as tests/test_gpu_program.py::_run gives every
    level its own); early: the last stage is issued on the lane first, the engine runs the rest."""
    from unscene3d_amd import MinkowskiEngine as ME
    from unscene3d_amd import program
    x = ME.SparseTensor(features=torch.from_numpy(feats).to(device), coordinates=torch.from_numpy(coords4).to(device),
                        device=device)
    _, fmaps = model(x)
    outs = [f.F for f in fmaps]
    if ext is None:
        g = torch.Generator().manual_seed(11)
        ext = [torch.randn(o.shape, generator=g).to(device) * w for o, w in zip(outs, (0.5, 1.0, 1.5, 2.0, 0.25))]
    if early:
        handle = program.handle_of(outs[-1])
        assert program.early_possible(handle)
        n0 = program.EARLY_RUNS
        program.early_backward(handle, ext[-1])
        assert program.EARLY_RUNS == n0 + 1
        torch.autograd.backward(outs[:-1], ext[:-1])
    else:
        torch.autograd.backward(outs, ext)
    return ext, [o.shape[0] for o in outs]


@pytest.mark.parametrize("voxels", [3_000, 40_000])
def test_last_stage_on_the_lane_changes_no_bit(device, monkeypatch, voxels):
    """40 000 voxels put the tile-compacted input-gradient kernel into the early range; the low hold bounds put the
    continuation's weight gradients through the lane's hold at these sizes."""
    from unscene3d_amd import program, units
    from unscene3d_amd._lib import lib
    from unscene3d_amd.models.res16unet import Res16UNet34C

    coords4, feats = _scene(voxels, 4100 + voxels % 89)
    torch.manual_seed(9)
    cfg = SimpleNamespace(bn_momentum=0.02, conv1_kernel_size=3, dilations=[1, 1, 1, 1])
    model = Res16UNet34C(3, 20, cfg, out_fpn=True).to(device).train()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    monkeypatch.setattr(program, "ENABLED", True)
    monkeypatch.setattr(program, "EARLY_STAGE", True)
    assert units._lane(torch.device(device)) is not None
    res, ext, rows = {}, None, None
    for name, early, low_hold in (("plain", False, False), ("early", True, False), ("early-held", True, True),
                                  ("plain-held", False, True)):
        if low_hold:        # s4 and finer are noted until the walk reaches the s8 map
            monkeypatch.setattr(units, "LANE_HOLD_MIN_ROWS", rows[2])
            monkeypatch.setattr(units, "LANE_RELEASE_ROWS", rows[1])
            assert rows[2] > rows[1] > 0
        model.load_state_dict(state)
        for p in model.parameters():
            p.grad.zero_()
        ext, rows = _trunk_pass(model, coords4, feats, device, ext, early)
        torch.cuda.synchronize()
        assert lib.usc_wgrad_lane_holding() == 0 and not program._EARLY_OPEN
        res[name] = ({n: p.grad.clone() for n, p in model.named_parameters() if not n.startswith("final.")},
                     {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k})
    assert float(res["plain"][0]["block8.0.conv1.kernel"].abs().sum()) > 0
    assert float(res["plain"][0]["conv0p1s1.kernel"].abs().sum()) > 0
    for name in ("early", "early-held", "plain-held"):
        for n, g in res["plain"][0].items():
            assert torch.equal(g, res[name][0][n]), (name, n)
        for k, v in res["plain"][1].items():
            assert torch.equal(v, res[name][1][k]), (name, k)


def test_lane_range_refusals(device):
    from unscene3d_amd import program
    from unscene3d_amd._lib import lib
    assert lib.usc_program_run_lane(None, 0, 0, None, 0, None) != 0
    with pytest.raises(RuntimeError, match="not possible"):
        program.early_backward(None, torch.zeros(1, 96, device=device))


# ------------------------------------------------------------------------------------------- 3. the whole step
def _module(device, n_scenes, overrides=()):
    import test_gpu_step_parity as sp
    cfg, batch, collate, module = sp._setup(device, 5, overrides)
    module.model.randperm = sp.PermSource()
    return module, collate(batch[:n_scenes])


def _three_steps(device, monkeypatch, n_scenes, switch):
    from unscene3d_amd import program
    from unscene3d_amd.ddp import flatten_grads
    from unscene3d_amd.models import mask3d
    from unscene3d_amd.optim import FlatAdamW

    monkeypatch.setattr(program, "EARLY_STAGE", bool(switch))
    module, batch = _module(device, n_scenes)
    params = [p for n, p in module.named_parameters() if ".backbone.final." not in n]
    flat = flatten_grads(params)
    opt = FlatAdamW(params, lr=1e-4, flat_grad=flat)
    opt.enable_early(module.model._side_stream(device))
    seen, n0 = [], mask3d.EARLY_STAGE_STEPS
    try:
        for _ in range(3):
            opt.zero_grad(set_to_none=False)
            total, _ = module.training_step(batch)
            total.backward()
            torch.cuda.synchronize()
            grads = flat.clone()
            opt.step()
            torch.cuda.synchronize()
            seen.append((total.detach().clone(), grads, [p.detach().clone() for p in params],
                         [b.clone() for b in module.buffers()]))
    finally:
        opt.disable_early()
    return seen, mask3d.EARLY_STAGE_STEPS - n0


@pytest.mark.parametrize("n_scenes", [1, 2])
def test_three_training_steps_keep_their_bits(device, monkeypatch, n_scenes):
    on, ran_on = _three_steps(device, monkeypatch, n_scenes, 1)
    off, ran_off = _three_steps(device, monkeypatch, n_scenes, 0)
    assert ran_on == 3 and ran_off == 0, (ran_on, ran_off)
    for step, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a[0], b[0]), (step, float(a[0]), float(b[0]))
        assert float(a[1].abs().sum()) > 0 and torch.equal(a[1], b[1]), step
        for k, (pa, pb) in enumerate(zip(a[2], b[2])):
            assert torch.equal(pa, pb), (step, "parameter", k)
        for k, (ba, bb) in enumerate(zip(a[3], b[3])):
            assert torch.equal(ba, bb), (step, "buffer", k)


def _one_pass(module, batch):
    for p in module.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        else:
            p.grad.zero_()
    total, _ = module.training_step(batch)
    total.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["np-features", "eval", "program-off"])
def test_configurations_that_keep_the_old_path(device, monkeypatch, case):
    from unscene3d_amd import program
    from unscene3d_amd.models import mask3d
    monkeypatch.setattr(program, "EARLY_STAGE", True)
    module, batch = _module(device, 1, ["model.use_np_features=true"] if case == "np-features" else ())
    if case == "eval":
        module.eval()
    if case == "program-off":
        monkeypatch.setattr(program, "ENABLED", False)
    n0, r0 = mask3d.EARLY_STAGE_STEPS, program.EARLY_RUNS
    _one_pass(module, batch)
    assert (mask3d.EARLY_STAGE_STEPS, program.EARLY_RUNS) == (n0, r0)
    assert float(module.model.backbone.block8[0].conv1.kernel.grad.abs().sum()) > 0


# ------------------------------------------------------------------------------------------- 4. a failed backward
def test_a_backward_that_raises_behind_the_early_part(device, monkeypatch):
    """The exception comes out of a decoder node that runs after the gate has issued the early part (the layer norm in
    front of a mask_module call was created before the gate).  Nothing stays noted or open, and the next pass gives the
    gradients of an undisturbed one."""
    import test_gpu_step_parity as sp
    from unscene3d_amd import ops, program
    from unscene3d_amd._lib import lib
    from unscene3d_amd.models import mask3d

    monkeypatch.setattr(program, "EARLY_STAGE", True)
    module, batch = _module(device, 1)
    state = {k: v.clone() for k, v in module.state_dict().items()}
    _one_pass(module, batch)
    names = [n for n, _ in module.named_parameters() if ".backbone.final." not in n]
    want = {n: p.grad.clone() for n, p in module.named_parameters() if n in names}

    module.load_state_dict(state)
    module.model.randperm = sp.PermSource()
    real = ops._LayerNorm.backward
    seen = []

    def poisoned(ctx, *grads):
        seen.append(program.EARLY_RUNS)
        raise RuntimeError("poisoned decoder node")
    monkeypatch.setattr(ops._LayerNorm, "backward", staticmethod(poisoned))
    r0, n0 = program.EARLY_RUNS, mask3d.EARLY_STAGE_STEPS
    with pytest.raises(RuntimeError, match="poisoned"):
        _one_pass(module, batch)
    monkeypatch.setattr(ops._LayerNorm, "backward", real)
    assert seen == [r0 + 1] and mask3d.EARLY_STAGE_STEPS == n0 + 1          # the early part had been issued
    assert program._EARLY_OPEN                                              # ... and nobody continued from it
    assert program.settle_abandoned(device)
    assert not program._EARLY_OPEN and lib.usc_wgrad_lane_holding() == 0

    module.load_state_dict(state)
    module.model.randperm = sp.PermSource()
    _one_pass(module, batch)
    assert mask3d.EARLY_STAGE_STEPS == n0 + 2 and not program._EARLY_OPEN
    for n, p in module.named_parameters():
        if n in want:
            assert torch.equal(p.grad, want[n]), n
