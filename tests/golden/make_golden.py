#!/usr/bin/env python
"""Golden-vector generator — runs ONLY in the build container, where /root/reference exists.

Imports the importable parts of the reference in place (stub modules for the dependencies that are
not installed: SURVEY.md Appendix A), feeds them seeded inputs and stores inputs + outputs as small
.npz fixtures next to this script.  Nothing from /root/reference is copied; the fixtures are data.

    python tests/golden/make_golden.py            # criterion / posenc / decoder_layers fixtures
    python tests/golden/make_golden.py decoder_pass   # one decoder pass, head-shared mask, forward + backward
    python tests/golden/make_golden.py aggregate  # N1 aggregate_features (mean / max, zero-segment fill)
    python tests/golden/make_golden.py felz       # Felzenszwalb over-segmentation (reference module built by oracle/Makefile)
    python tests/golden/make_golden.py felz_build # the reference module's labels on the meshes of test_oracle_equals_reference_build
    python tests/golden/make_golden.py ncut       # NCut fixtures (separate interpreter: different stubs)
    python tests/golden/make_golden.py export     # eval/export post-processing fixtures (trainer.eval_instance_step)
    python tests/golden/make_golden.py dataset    # self-train mask merge + validation-mode scene reader fixtures
    python tests/golden/make_golden.py elastic    # elastic distortion fixtures (datasets.semseg.elastic_distortion)
    python tests/golden/make_golden.py state_dict # parameter names + shapes of the reference's Res16UNet34C / Mask3D module trees
"""
import importlib
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return MagicMock()


def stub(*names):
    for n in names:
        try:
            __import__(n)
        except Exception:
            sys.modules[n] = _Stub(n)


def import_reference_models():
    stub("MinkowskiEngine", "MinkowskiEngine.MinkowskiOps", "MinkowskiEngine.MinkowskiPooling", "custom_cuda_utils",
         "detectron2", "detectron2.utils", "detectron2.utils.comm", "detectron2.projects",
         "detectron2.projects.point_rend", "detectron2.projects.point_rend.point_features", "hydra", "torch_scatter",
         "pointnet2", "pointnet2._ext", "torchvision")

    class MinkowskiNetwork(nn.Module):
        def __init__(self, D):
            super().__init__()
            self.D = D

    sys.modules["MinkowskiEngine"].MinkowskiNetwork = MinkowskiNetwork
    sys.modules["detectron2.utils.comm"].get_world_size = lambda: 1
    os.chdir(REF)
    sys.path.insert(0, REF)
    mods = {n: importlib.import_module(f"models.{n}") for n in ("matcher", "criterion", "position_embedding", "mask3d")}
    mods["helpers"] = importlib.import_module("models.modules.helpers_3detr")
    return mods


def t2n(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


def make_criterion(mods):
    g = torch.Generator().manual_seed(11)
    B, Q, C = 2, 100, 3
    S = [310, 270]
    T = [7, 9]
    n_aux = 2
    logits = [torch.randn(B, Q, C, generator=g) for _ in range(n_aux + 1)]
    masks = [[torch.randn(S[b], Q, generator=g) * 2 for b in range(B)] for _ in range(n_aux + 1)]
    targets = []
    for b in range(B):
        seg = torch.rand(T[b], S[b], generator=g) < 0.15
        seg[:, :3] = True
        targets.append({"labels": torch.ones(T[b], dtype=torch.int64), "segment_mask": seg})
    for l in logits:
        l.requires_grad_()
    for lv in masks:
        for m in lv:
            m.requires_grad_()
    matcher = mods["matcher"].HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=2.0, cost_noise_robust=0.0,
                                               num_points=-1)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0, "loss_noise_robust": 0.0}
    wd.update({f"{k}_{i}": v for i in range(n_aux) for k, v in list(wd.items())})
    crit = mods["criterion"].SetCriterion(num_classes=3, matcher=matcher, weight_dict=wd, eos_coef=0.1,
                                          losses=["labels", "masks"], num_points=-1, oversample_ratio=3.0,
                                          importance_sample_ratio=0.75, class_weights=-1)
    outputs = {"pred_logits": logits[-1], "pred_masks": masks[-1],
               "aux_outputs": [{"pred_logits": logits[i], "pred_masks": masks[i]} for i in range(n_aux)]}
    losses = crit(outputs, targets, mask_type="segment_mask")
    total = sum(losses[k] * wd[k] for k in losses if k in wd)
    total.backward()
    idx_final = matcher(outputs, targets, "segment_mask")
    out = {"n_aux": np.int64(n_aux), "total": total.detach().numpy()}
    for i in range(n_aux + 1):
        out[f"logits_{i}"] = logits[i].detach().numpy()
        out[f"logits_grad_{i}"] = logits[i].grad.numpy()
        for b in range(B):
            out[f"masks_{i}_{b}"] = masks[i][b].detach().numpy()
            out[f"masks_grad_{i}_{b}"] = masks[i][b].grad.numpy()
    for b in range(B):
        out[f"tgt_mask_{b}"] = np.packbits(targets[b]["segment_mask"].numpy(), axis=1)
        out[f"tgt_shape_{b}"] = np.array(targets[b]["segment_mask"].shape)
        out[f"match_q_{b}"], out[f"match_t_{b}"] = idx_final[b][0].numpy(), idx_final[b][1].numpy()
    for k, v in losses.items():
        out["loss/" + k] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "criterion.npz"), **out)
    print("criterion: total", float(total), "keys", len(losses))


def make_posenc(mods):
    torch.manual_seed(5)
    pe = mods["position_embedding"].PositionEmbeddingCoordsSine(pos_type="fourier", d_pos=128, gauss_scale=1.0,
                                                                 normalize=True)
    g = torch.Generator().manual_seed(6)
    xyz = torch.rand(2, 300, 3, generator=g) * torch.tensor([6.0, 4.0, 2.8]) - 1.0
    mins, maxs = xyz.min(1)[0], xyz.max(1)[0]
    out = pe(xyz.clone(), input_range=[mins, maxs])
    np.savez_compressed(os.path.join(HERE, "posenc.npz"), gauss_B=pe.gauss_B.numpy(), xyz=xyz.numpy(),
                        mins=mins.numpy(), maxs=maxs.numpy(), out=out.numpy())
    print("posenc", tuple(out.shape))


def make_decoder_layers(mods):
    m3 = mods["mask3d"]
    torch.manual_seed(9)
    g = torch.Generator().manual_seed(10)
    d, H, Q, K, B = 128, 8, 40, 48, 2
    ca, sa, ffn = m3.CrossAttentionLayer(d, H), m3.SelfAttentionLayer(d, H), m3.FFNLayer(d, 256)
    mlp = mods["helpers"].GenericMLP(input_dim=d, hidden_dims=[d], output_dim=d, use_conv=True,
                                     output_use_activation=True, hidden_use_bias=True)
    tgt = torch.randn(Q, B, d, generator=g)
    mem = torch.randn(K, B, d, generator=g)
    pos = torch.randn(K, B, d, generator=g)
    qpos = torch.randn(Q, B, d, generator=g)
    mask = torch.rand(B * H, Q, K, generator=g) < 0.3
    mask[:, :, 0] = False
    o1 = ca(tgt, mem, memory_mask=mask, memory_key_padding_mask=None, pos=pos, query_pos=qpos)
    o2 = sa(o1, tgt_mask=None, tgt_key_padding_mask=None, query_pos=qpos)
    o3 = ffn(o2)
    qp = torch.randn(B, d, Q, generator=g)
    o4 = mlp(qp)
    out = {"tgt": tgt, "mem": mem, "pos": pos, "qpos": qpos, "o1": o1, "o2": o2, "o3": o3, "qp": qp, "o4": o4}
    out = t2n(out)
    out["mask"] = np.packbits(mask.numpy(), axis=2)
    for name, mod in (("ca", ca), ("sa", sa), ("ffn", ffn), ("mlp", mlp)):
        for k, v in mod.state_dict().items():
            out[f"{name}/{k}"] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "decoder_layers.npz"), **out)
    print("decoder layers ok")


def make_decoder_pass(mods):
    """One decoder pass of the reference (CrossAttentionLayer -> SelfAttentionLayer -> FFNLayer, models/mask3d.py:491-651)
    in the PRODUCT shape of the mask: one bool[B, K, Q] mask shared by all heads, repeated per head exactly like
    mask3d.py:349 (`repeat_interleave(num_heads, dim=0).permute((0, 2, 1))`), forward AND backward.  Weights are the
    ones already stored in decoder_layers.npz; inputs are fp16-representable so that they store compactly."""
    m3 = mods["mask3d"]
    z = np.load(os.path.join(HERE, "decoder_layers.npz"))
    d, H, Q, K, B = 128, 8, 40, 160, 2
    ca, sa, ffn = m3.CrossAttentionLayer(d, H), m3.SelfAttentionLayer(d, H), m3.FFNLayer(d, 256)
    for name, mod in (("ca", ca), ("sa", sa), ("ffn", ffn)):
        mod.load_state_dict({k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/")})
    g = torch.Generator().manual_seed(21)
    h16 = lambda *shape: torch.randn(*shape, generator=g).half().float()
    tgt, mem, pos, qpos, w = h16(Q, B, d), h16(K, B, d), h16(K, B, d), h16(Q, B, d), h16(Q, B, d)
    bsl = torch.rand(B, K, Q, generator=g) < 0.4
    bsl[:, 0, :] = False                       # every query keeps one key
    bsl[0, :, 3] = True                        # ... except these two, which the decoder then un-masks (mask3d.py:346)
    bsl[1, :, 17] = True
    bsl.permute(0, 2, 1)[bsl.sum(1) == K] = False
    bsl[1, 100:, :] = True                     # scene 1 shorter than the sample size: padded keys masked (:316-323)
    leaves = {"tgt": tgt, "mem": mem, "pos": pos, "qpos": qpos}
    for v in leaves.values():
        v.requires_grad_()
    mask = bsl.repeat_interleave(H, dim=0).permute(0, 2, 1)
    o1 = ca(tgt, mem, memory_mask=mask, memory_key_padding_mask=None, pos=pos, query_pos=qpos)
    o2 = sa(o1, tgt_mask=None, tgt_key_padding_mask=None, query_pos=qpos)
    o3 = ffn(o2)
    (o3 * w).sum().backward()
    out = {k: v.detach().numpy().astype(np.float16) for k, v in leaves.items()}
    out["w"] = w.numpy().astype(np.float16)
    out["mask_bsl"] = np.packbits(bsl.numpy(), axis=2)
    out["shape"] = np.array([Q, K, B, H, d])
    out.update(t2n({"o1": o1, "o3": o3, "g_tgt": tgt.grad, "g_mem": mem.grad, "g_qpos": qpos.grad}))
    for name, mod, keys in (("ca", ca, ("multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias",
                                        "multihead_attn.out_proj.bias", "norm.weight", "norm.bias")),
                            ("sa", sa, ("self_attn.in_proj_bias", "norm.weight")),
                            ("ffn", ffn, ("linear1.bias", "linear2.bias", "norm.bias"))):
        params = dict(mod.named_parameters())
        for k in keys:
            out[f"grad/{name}/{k}"] = params[k].grad.numpy()
    np.savez_compressed(os.path.join(HERE, "decoder_pass.npz"), **out)
    print("decoder pass ok", {k: v.shape for k, v in out.items() if k.startswith("g")})


def import_reference_ncut():
    """pseudo_masks/unscene3d_pseudo_main.py with stubs (recipe 2). Run in a fresh
    interpreter state: its `models`/`datasets`/`utils.*` imports are stubbed, unlike recipe 1."""
    stub("hydra", "omegaconf", "pyviz3d", "pyviz3d.visualizer", "MinkowskiEngine", "open3d", "hdbscan", "datasets",
         "datasets.dataset", "models", "models.encoders_2d", "utils.utils", "utils.cuda_utils",
         "utils.cuda_utils.raycast_image")
    sys.modules["hydra"].main = lambda **kw: (lambda f: f)
    os.chdir(os.path.join(REF, "pseudo_masks"))
    sys.path.insert(0, os.path.join(REF, "pseudo_masks"))
    sys.path.insert(0, REF)
    return importlib.import_module("unscene3d_pseudo_main")


def planted_scene(seed, side, dims, n_objects, pts_per_seg=6, noise=None):
    """Config-5 inputs: a side x side grid of segments; `n_objects` compact rectangular
    objects of DISTINCT sizes (distinct sizes keep the small eigenvalues of the weakly coupled blocks
    simple) scattered over a background cluster that separates them spatially, like furniture on a floor."""
    rng = np.random.default_rng(seed)
    S = side * side
    label = np.zeros((side, side), np.int64)            # 0 = background
    sizes = [(2 + (k % 4), 3 + (k // 3)) for k in range(n_objects)]
    placed = 0
    for k, (h, w) in enumerate(sizes):
        for _ in range(200):
            r, c = int(rng.integers(1, side - h - 1)), int(rng.integers(1, side - w - 1))
            if not label[r - 1:r + h + 1, c - 1:c + w + 1].any():
                label[r:r + h, c:c + w] = k + 1
                placed += 1
                break
    label = label.reshape(-1)
    gx, gy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    # noise=None: every segment 0.25 sigma (clean, block-constant affinities -> highly degenerate spectra);
    # noise=(lo, hi): per-segment sigma ~ U(lo, hi) -> irregular thresholded graphs like real DINO/CSC features
    sig = 0.25 if noise is None else rng.uniform(noise[0], noise[1], size=(S, 1))
    feats = []
    for d in dims:
        cent = rng.normal(size=(n_objects + 1, d))
        feats.append((cent[label] + sig * rng.normal(size=(S, d))).astype(np.float32))
    conn = []
    for i in range(S):
        for da, db in ((1, 0), (0, 1)):
            a, b = gx[i] + da, gy[i] + db
            if a < side and b < side:
                j = a * side + b
                conn += [(i, j), (j, i)]
    conn = np.asarray(conn, np.int64)
    seg_ids = np.repeat(np.arange(S), pts_per_seg)
    coords = np.stack([gx[seg_ids] + rng.random(len(seg_ids)), gy[seg_ids] + rng.random(len(seg_ids)),
                       rng.random(len(seg_ids))], 1).astype(np.float32)
    return feats, conn, seg_ids, coords, label, placed


def make_ncut(ref):
    out = {}
    cases = {"single": (15, (96,), 8, 0.6, None), "dual": (25, (384, 96), 16, 0.6, None),
             "irregular": (25, (384, 96), 16, 0.6, (0.3, 1.2))}
    for name, (side, dims, k, tau, noise) in cases.items():
        feats, conn, seg_ids, coords, label, placed = planted_scene(50 + side, side, dims, k, noise=noise)
        S = side * side
        tf = [torch.from_numpy(f) for f in feats]
        mk = lambda: tf[0].clone() if len(tf) == 1 else (tf[0].clone(), tf[1].clone())
        uniq = torch.arange(S)
        # per-iteration internals straight from the reference's own functions (logged by wrapping them)
        trace = []
        orig = ref.second_smallest_eigenvector

        def logged(A, D, _orig=orig, _trace=trace):
            res = _orig(A, D)
            w = __import__("scipy.linalg").linalg.eigh(D - A, D, subset_by_index=[1, 2], eigvals_only=True)
            _trace.append((A > 0.5, np.diag(D).copy(), res[1].copy(), w))
            return res

        ref.second_smallest_eigenvector = logged
        masks = ref.unscene3d(mk(), uniq, torch.from_numpy(conn), torch.from_numpy(seg_ids), torch.from_numpy(coords),
                              torch.from_numpy(coords), affinity_tau=tau, max_number_of_instances=20,
                              similarity_metric="cos", min_segment_size=4, separation_mode="max",
                              max_extent_ratio=0.8)
        ref.second_smallest_eigenvector = orig
        for j, f in enumerate(feats):
            out[f"{name}/feat{j}"] = f
        out[f"{name}/conn"], out[f"{name}/label"] = conn, label
        out[f"{name}/tau"] = np.float64(tau)
        out[f"{name}/n_iter"] = np.int64(len(trace))
        for it, (A, d, vec, w) in enumerate(trace):
            out[f"{name}/it{it}/A"] = np.packbits(A, axis=1)
            out[f"{name}/it{it}/deg"], out[f"{name}/it{it}/vec"], out[f"{name}/it{it}/evals"] = d, vec, w
        out[f"{name}/masks"] = np.packbits(masks.astype(bool), axis=1)
        out[f"{name}/n_masks"] = np.int64(masks.shape[0])
        gaps = [float((w[1] - w[0]) / max(w[1], 1e-300)) for (_, _, _, w) in trace]
        print("ncut", name, "S", S, "objects placed", placed, "masks", masks.shape, "rel gaps", np.round(gaps, 4))
    np.savez_compressed(os.path.join(HERE, "ncut.npz"), **out)


def make_ncut_l2(ref):
    """get_affinity_matrix(similarity_metric='l2') of the reference (unscene3d_pseudo_main.py:89-119 -> l2_sim,
    utils/freemask_utils.py:20-36) on clustered single-modality features: thresholded affinity bits + degrees."""
    rng = np.random.default_rng(123)
    S, d, k = 150, 24, 7
    centres = rng.normal(0, 1, (k, d))
    lab = rng.integers(0, k, S)
    feats = (centres[lab] + rng.normal(0, 0.35, (S, d))).astype(np.float32)
    out = {"feats": feats}
    for tau in (0.5, 0.7):
        A, D = ref.get_affinity_matrix(torch.from_numpy(feats.copy()), tau=tau, similarity_metric="l2")
        out[f"tau{tau}/A"] = np.packbits(A > 0.5, axis=1)
        out[f"tau{tau}/deg"] = np.diag(D).copy()
        print("ncut_l2 tau", tau, "ones", int((A > 0.5).sum()), "of", S * S)
    np.savez_compressed(os.path.join(HERE, "ncut_l2.npz"), **out)


def make_aggregate(ref):
    """N1: `aggregate_features` (pseudo_masks/unscene3d_pseudo_main.py:350-402) on seeded point features: segment ids
    with gaps, ~20 % all-zero (invalid) rows, segments whose rows are ALL zero — filled from the connected segments of
    `zero_segments[0]` for every zero segment (the :387 quirk), or from the global mean when that one has no valid
    neighbour — in both aggregation modes."""
    from types import SimpleNamespace as NS
    out = {}
    for case, first_zero_connected in (("neigh", True), ("global", False)):
        rng = np.random.default_rng(77 if first_zero_connected else 78)
        S, N, d = 48, 3000, 24
        ids = np.sort(rng.choice(np.arange(5, 400), S, replace=False)).astype(np.int64)   # ids with gaps
        seg = ids[rng.integers(0, S, N)]
        feats = rng.standard_normal((N, d)).astype(np.float32)
        feats[rng.random(N) < 0.2] = 0.0                                                  # invalid rows
        zero_segs = ids[[4, 17, 30]]                                                      # every row invalid
        feats[np.isin(seg, zero_segs)] = 0.0
        pairs = set()
        for a in range(S):                                                                # ring + a few chords
            for b in (a + 1, a + 5):
                pairs.add((ids[a], ids[b % S])); pairs.add((ids[b % S], ids[a]))
        if not first_zero_connected:                                                      # isolate zero_segments[0]
            pairs = {(a, b) for (a, b) in pairs if a != zero_segs[0] and b != zero_segs[0]}
        conn = np.array(sorted(pairs), dtype=np.int64)
        out[f"{case}/feats"], out[f"{case}/seg"], out[f"{case}/conn"] = feats, seg, conn
        for mode in ("mean", "max"):
            cfg = NS(freemask=NS(aggregation_mode=mode))
            agg, uniq = ref.aggregate_features(torch.from_numpy(feats), torch.from_numpy(seg), torch.from_numpy(conn), cfg)
            assert np.array_equal(uniq.numpy(), ids)
            out[f"{case}/{mode}"] = agg.numpy()
        out[f"{case}/uniq"] = ids
        print("aggregate", case, "zero segments", zero_segs, "conn", conn.shape)
    np.savez_compressed(os.path.join(HERE, "aggregate.npz"), **out)


def make_felz():
    """§8f-2: the reference's own felzenszwalb_cpp module (built from /root/reference/utils/cpp_utils/segmentator.cpp by
    `make -C oracle ref` into oracle/_ref/) on two seeded meshes: `distinct` (continuous colours: weights equal only
    between the two copies of one mesh edge) and `ties` (colours quantised to 1/16: thousands of equal weights, incl.
    exact zeros).  Inputs are stored with the outputs; normals / weights come from the restatement that this same
    script first checks against the reference's labels and connectivity."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import felz_ref as FR
    from unscene3d_amd.synthetic import make_mesh
    ref = FR.reference_module()
    assert ref is not None, "run `make -C oracle ref` first"
    out = {}
    for name, seed, q in (("distinct", 1, False), ("ties", 2, True)):
        v, f, c = make_mesh(seed, side=60, quantise_colours=q)
        labels, conn = ref.segment_mesh(v, f, c, 0.005, 20)
        ol, oc, det = FR.segment_mesh(v, f, c, 0.005, 20, stable=False, details=True)
        assert np.array_equal(labels, ol) and np.array_equal(conn, oc), "restatement differs from the reference build"
        out.update({f"{name}/vertices": v, f"{name}/faces": f, f"{name}/colors": c, f"{name}/labels": labels.astype(np.int32),
                    f"{name}/connectivity": np.asarray(conn, np.int32), f"{name}/normals": det["normals"],
                    f"{name}/weights": det["weights"]})
        print("felz", name, "segments", int(labels.max()) + 1, "pairs", conn.shape, "distinct weights",
              len(np.unique(det["weights"])), "of", det["weights"].shape[0])
    np.savez_compressed(os.path.join(HERE, "felz.npz"), **out)


FELZ_BUILD_CASES = ((11, 40, False), (12, 40, True), (13, 120, False), (14, 120, True))


def make_felz_build():
    """The reference's own felzenszwalb_cpp module (oracle/_ref/, see make_felz) on the seeded meshes of
    tests/test_felzenszwalb.py::test_oracle_equals_reference_build — labels and connectivity for min_vertices 20 and 50.
    Only the outputs are stored: the meshes are unscene3d_amd.synthetic.make_mesh(seed, side, quantise_colours)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import felz_ref as FR
    from unscene3d_amd.synthetic import make_mesh
    ref = FR.reference_module()
    assert ref is not None, "run `make -C oracle ref` first"
    out = {}
    for seed, side, q in FELZ_BUILD_CASES:
        v, f, c = make_mesh(seed, side=side, quantise_colours=q)
        for min_verts in (20, 50):
            labels, conn = ref.segment_mesh(v, f, c, 0.005, min_verts)
            out[f"{seed}/{min_verts}/labels"] = np.asarray(labels, np.int32)
            out[f"{seed}/{min_verts}/connectivity"] = np.asarray(conn, np.int32).reshape(-1, 2)
            print("felz_build", seed, min_verts, "segments", int(np.max(labels)) + 1, "pairs", len(conn))
    np.savez_compressed(os.path.join(HERE, "felz_build.npz"), **out)


def make_ncut_b(ref):
    """A second config-5 scene for the hook-free product path (tests/golden/ncut_b.npz): 24 x 25 = 600 segments, ONE
    modality (CSC-like 96-d), per-segment noise levels, other seed.  Records the reference's masks and the sign-carrying
    eigenvector of every iteration (not the affinity matrices: the file stays small)."""
    rng_seed, rows, cols, d, k = 91, 24, 25, 96, 14
    feats, conn, seg_ids, coords, label, placed = planted_scene(rng_seed, 25, (d,), k, noise=(0.3, 1.2))
    keep = np.arange(rows * cols)                                 # drop the last grid row: 600 segments
    f = feats[0][keep]
    conn = conn[(conn[:, 0] < rows * cols) & (conn[:, 1] < rows * cols)]
    pts = np.isin(seg_ids, keep)
    seg_ids, coords = seg_ids[pts], coords[pts]
    S = rows * cols
    trace = []
    orig = ref.second_smallest_eigenvector

    def logged(A, D, _orig=orig, _trace=trace):
        res = _orig(A, D)
        w = __import__("scipy.linalg").linalg.eigh(D - A, D, subset_by_index=[1, 2], eigvals_only=True)
        _trace.append((np.diag(D).copy(), res[1].copy(), w, int((~(A > 0.5).any(1)).sum())))
        return res

    ref.second_smallest_eigenvector = logged
    masks = ref.unscene3d(torch.from_numpy(f).clone(), torch.arange(S), torch.from_numpy(conn), torch.from_numpy(seg_ids),
                          torch.from_numpy(coords), torch.from_numpy(coords), affinity_tau=0.6,
                          max_number_of_instances=20, similarity_metric="cos", min_segment_size=4,
                          separation_mode="max", max_extent_ratio=0.8)
    ref.second_smallest_eigenvector = orig
    out = {"feat0": f, "conn": conn, "tau": np.float64(0.6), "n_iter": np.int64(len(trace)),
           "masks": np.packbits(masks.astype(bool), axis=1), "n_masks": np.int64(masks.shape[0])}
    for it, (deg, vec, w, painted) in enumerate(trace):
        out[f"it{it}/deg"], out[f"it{it}/vec"], out[f"it{it}/evals"], out[f"it{it}/painted"] = deg, vec, w, np.int64(painted)
    gaps = [float((w[1] - w[0]) / max(w[1], 1e-300)) for (_, _, w, _) in trace]
    print("ncut_b S", S, "masks", masks.shape, "rel gaps", np.round(gaps, 4))
    np.savez_compressed(os.path.join(HERE, "ncut_b.npz"), **out)


def import_reference_trainer():
    stub("imageio", "pyviz3d", "pyviz3d.visualizer", "torch_scatter", "matplotlib", "matplotlib.cm", "hydra",
         "MinkowskiEngine", "MinkowskiEngine.MinkowskiOps", "MinkowskiEngine.MinkowskiPooling", "custom_cuda_utils",
         "detectron2", "detectron2.utils", "detectron2.utils.comm", "detectron2.projects",
         "detectron2.projects.point_rend", "detectron2.projects.point_rend.point_features", "pointnet2",
         "pointnet2._ext", "torchvision", "pytorch_lightning", "open3d", "benchmark",
         "benchmark.evaluate_semantic_instance", "utils.votenet_utils", "utils.votenet_utils.eval_det",
         "albumentations", "volumentations", "plyfile", "natsort", "loguru", "fire")

    class MinkowskiNetwork(nn.Module):
        def __init__(self, D):
            super().__init__()
            self.D = D

    def scatter_mean(src, index, dim=0):
        # torch_scatter 2.x (not installed, not part of /root/reference): out[i] = sum(src[index == i]) / max(count, 1)
        assert dim == 0
        n = int(index.max()) + 1
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype)
        out.index_add_(0, index, src)
        cnt = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
        return out / cnt.clamp(min=1).view(-1, *([1] * (src.dim() - 1)))

    sys.modules["MinkowskiEngine"].MinkowskiNetwork = MinkowskiNetwork
    sys.modules["pytorch_lightning"].LightningModule = nn.Module
    sys.modules["pytorch_lightning"].Callback = object
    sys.modules["torch_scatter"].scatter_mean = scatter_mean
    os.chdir(REF)
    sys.path.insert(0, REF)
    return importlib.import_module("trainer.trainer")


def export_scene(seed, n_obj=6, q=100):
    """A small voxel scene of box-shaped objects over a floor, an over-segmentation of it, and decoder outputs
    that (a) cover objects, (b) duplicate some of them, (c) merge two disconnected objects in one query."""
    rng = np.random.default_rng(seed)
    pts, seg, obj = [], [], []
    sid = 0
    fx, fy = np.meshgrid(np.arange(40), np.arange(36), indexing="ij")
    floor = np.stack([fx.ravel(), fy.ravel(), np.zeros(fx.size, int)], 1)
    pts.append(floor)
    seg.append(sid + (floor[:, 0] // 10) * 4 + floor[:, 1] // 9)
    obj.append(np.zeros(len(floor), int))
    sid += 16
    for o in range(n_obj):
        lo = np.array([3 + 6 * o, rng.integers(2, 24), 2 + (o % 2)])
        sz = rng.integers(3, 6, 3)
        g = np.stack(np.meshgrid(*[np.arange(l, l + s) for l, s in zip(lo, sz)], indexing="ij"), -1).reshape(-1, 3)
        pts.append(g)
        seg.append(sid + (g[:, 2] - lo[2]) // 2)
        sid += int(((g[:, 2] - lo[2]) // 2).max()) + 1
        obj.append(np.full(len(g), o + 1))
    pts, seg, obj = np.concatenate(pts), np.concatenate(seg), np.concatenate(obj)
    perm = rng.permutation(len(pts))
    pts, seg, obj = pts[perm], seg[perm], obj[perm]
    S = sid
    seg_obj = np.zeros(S, int)
    seg_obj[seg] = obj
    masks = rng.normal(-4.0, 1.0, (S, q)).astype(np.float32)
    for j in range(n_obj):                                   # one query per object
        masks[:, j] = np.where(seg_obj == j + 1, 4.0, -4.0) + rng.normal(0, 0.5, S)
    masks[:, n_obj] = np.where(seg_obj == 1, 3.0, -4.0) + rng.normal(0, 0.5, S)        # duplicate of object 1
    masks[:, n_obj + 1] = np.where((seg_obj == 2) | (seg_obj == 5), 3.5, -4.0)          # two objects, disconnected
    masks[:, n_obj + 2] = np.where(seg_obj == 0, 2.0, -5.0)                             # the floor
    logits = rng.normal(0, 1, (q, 3)).astype(np.float32)
    logits[:n_obj + 3, 1] += 4.0
    logits[n_obj + 3:, 2] += 3.0
    n_low = len(pts)
    inverse = np.concatenate([np.arange(n_low), rng.integers(0, n_low, 2 * n_low)])
    inverse = inverse[rng.permutation(len(inverse))]
    seg_full = seg[inverse].copy()
    flip = rng.random(len(seg_full)) < 0.04
    seg_full[flip] = rng.integers(0, S, int(flip.sum()))
    full_coords = (pts[inverse] + rng.uniform(0, 1, (len(inverse), 3))) * 0.02
    t_masks = np.stack([obj[inverse] == j + 1 for j in range(n_obj)])
    return dict(raw_coords=pts.astype(np.float64) * 0.3, point2segment=seg.astype(np.int64), pred_masks=masks,
                pred_logits=logits, inverse_map=inverse.astype(np.int64), point2segment_full=seg_full.astype(np.int64),
                full_res_coords=full_coords.astype(np.float32), target_masks=t_masks,
                target_labels=np.ones(n_obj, np.int64))


def make_export(tr):
    import tempfile
    from types import SimpleNamespace as NS

    out = {}
    cases = {"freemask": dict(use_dbscan=False, topk_per_image=100, filter_out_instances=True),
             "dbscan": dict(use_dbscan=True, topk_per_image=-1, filter_out_instances=True),
             "plain": dict(use_dbscan=False, topk_per_image=-1, filter_out_instances=False)}
    for name, opt in cases.items():
        scenes = [export_scene(100 + i) for i in range(2)]
        save_dir = tempfile.mkdtemp()

        class Cfg(dict):
            __getattr__ = dict.__getitem__

        general = Cfg(use_dbscan=opt["use_dbscan"], dbscan_eps=0.95, dbscan_min_points=1,
                      topk_per_image=opt["topk_per_image"], filter_out_instances=opt["filter_out_instances"],
                      scores_threshold=0.1, iou_threshold=0.66, separate_instances=False, eval_inner_core=-1,
                      save_visualizations=False, save_for_freemask=True, export=False, save_dir=save_dir)
        cfg = Cfg(general=general, data=Cfg(test_mode="validation"))
        me = NS(config=cfg, decoder_id=-1, eval_on_segments=True, device="cpu",
                model=NS(train_on_segments=True, num_classes=3),
                validation_dataset=NS(label_offset=2, dataset_name="scannet", _remap_model_output=lambda o: np.asarray(o)),
                preds={}, bbox_preds={}, bbox_gt={})
        me.get_mask_and_scores = lambda *a, **k: tr.InstanceSegmentation.get_mask_and_scores(me, *a, **k)
        me.get_full_res_mask = lambda *a, **k: tr.InstanceSegmentation.get_full_res_mask(me, *a, **k)
        output = {"aux_outputs": [],
                  "pred_logits": torch.from_numpy(np.stack([s["pred_logits"] for s in scenes])),
                  "pred_masks": [torch.from_numpy(s["pred_masks"]) for s in scenes]}
        target_low = [{"point2segment": torch.from_numpy(s["point2segment"])} for s in scenes]
        target_full = [{"point2segment": torch.from_numpy(s["point2segment_full"]),
                        "labels": torch.from_numpy(s["target_labels"].copy()),
                        "masks": torch.from_numpy(s["target_masks"])} for s in scenes]
        names = [f"scene{i:04d}_00" for i in range(2)]
        tr.InstanceSegmentation.eval_instance_step(
            me, output, target_low, target_full, [s["inverse_map"] for s in scenes], names,
            [s["full_res_coords"] for s in scenes], [None, None], [None, None],
            np.concatenate([s["raw_coords"] for s in scenes]), [0, 1])
        for i, (s, nm) in enumerate(zip(scenes, names)):
            for k, v in s.items():
                out[f"{name}/{i}/{k}"] = np.packbits(v, axis=1) if v.dtype == bool else v
            p = me.preds[nm]
            pm = np.asarray(p["pred_masks"]).astype(bool)
            out[f"{name}/{i}/out_masks"] = np.packbits(pm, axis=0)
            out[f"{name}/{i}/out_n"] = np.array(pm.shape)
            out[f"{name}/{i}/out_scores"] = np.asarray(p["pred_scores"], np.float32)
            out[f"{name}/{i}/out_classes"] = np.asarray(p["pred_classes"], np.int64)
            saved = np.load(f"{save_dir}/freemasks/{nm}_masks.npy")
            cloud = np.load(f"{save_dir}/freemasks/{nm}_cloud.npy")
            assert saved.dtype == bool and np.array_equal(saved, pm) and np.array_equal(cloud, s["full_res_coords"])
            out[f"{name}/{i}/out_boxes"] = np.array([np.concatenate([[c], b, [sc]]) for c, b, sc in me.bbox_preds[nm]],
                                                    np.float64).reshape(-1, 8)
            print(name, i, "masks", pm.shape, "scores", out[f"{name}/{i}/out_scores"][:6])
        for k, v in opt.items():
            out[f"{name}/{k}"] = np.array(v)
    np.savez_compressed(os.path.join(HERE, "export.npz"), **out)


def import_reference_dataset():
    stub("open3d", "felzenszwalb_cpp", "albumentations", "volumentations", "imageio", "MinkowskiEngine", "plyfile",
         "natsort", "loguru", "fire", "torch_scatter", "hydra")
    os.chdir(REF)
    sys.path.insert(0, REF)
    return importlib.import_module("datasets.freemask_semseg")


def make_dataset(ds):
    import tempfile
    from types import SimpleNamespace as NS

    rng = np.random.default_rng(7)
    out = {}
    tmp = tempfile.mkdtemp()
    os.makedirs(f"{tmp}/freemasks")
    os.makedirs(f"{tmp}/scans/scene0001_00")
    n = 4000
    xyz = rng.uniform(0, [6, 5, 2.5], (n, 3))
    pts = np.concatenate([xyz, rng.integers(0, 256, (n, 3)), rng.normal(0, 1, (n, 3)), rng.integers(0, 60, (n, 1)),
                          np.zeros((n, 2))], 1).astype(np.float32)
    obj = (xyz[:, 0] // 1.0).astype(int) + 6 * (xyz[:, 1] // 2.5).astype(int)            # 12 spatial cells
    free = np.stack([(obj == j) * rng.uniform(0.3, 1.0, n) for j in (0, 3, 7)], 1).astype(np.float32)
    free = np.concatenate([free, (rng.random((n, 1)) < 0.25) * 0.9], 1).astype(np.float32)   # one scene-sized mask
    # the previous round's export: a different (denser) cloud with its own masks, most confident first
    m = 6000
    cloud = np.concatenate([xyz + rng.normal(0, 0.004, (n, 3)), rng.uniform(0, [6, 5, 2.5], (m - n, 3))]).astype(np.float32)
    cobj = (cloud[:, 0] // 1.0).astype(int) + 6 * (cloud[:, 1] // 2.5).astype(int)
    st = np.stack([cobj == 1, (cobj == 0) | (cobj == 2), cobj == 3, cobj == 5, (cobj == 5) | (cobj == 8), cobj == 9,
                   cobj == 10, cobj == 11], 1)
    np.save(f"{tmp}/scans/scene0001_00/0001_00.npy", pts)
    np.save(f"{tmp}/scans/scene0001_00/0001_00_freemasks.npy", free)
    np.save(f"{tmp}/freemasks/scene0001_00_cloud.npy", cloud)
    np.save(f"{tmp}/freemasks/scene0001_00_masks.npy", st)
    out.update(points=pts, freemasks=free, st_cloud=cloud, st_masks=np.packbits(st, axis=1))

    mean, std = (0.47793125906962, 0.4303257521323044, 0.3749598901421883), (0.2834475483823543, 0.27566157565723015, 0.27018971370874995)

    def normalize(image):
        # albumentations.Normalize(mean, std, max_pixel_value=255) — third-party, not installed, not in /root/reference:
        # img = (img - mean * 255) * (1 / (std * 255)) in float32
        mu = np.array(mean, np.float32) * 255.0
        den = np.reciprocal(np.array(std, np.float32) * 255.0)
        return {"image": (image.astype(np.float32) - mu) * den}

    me = NS(data=[{"filepath": f"{tmp}/scans/scene0001_00/0001_00.npy",
                   "raw_filepath": f"{tmp}/raw/scene0001_00/scene0001_00_vh_clean_2.ply"}],
            self_train_data_dir=tmp, load_self_train_data=True, num_self_train_data=5, cache_data=False, on_crops=False,
            max_num_gt_instances=-1, resegment_mesh=False, freemask_extent_max_ratio=0.8, freemask_hard_threshold=0.5,
            add_colors=True, add_normals=True, add_raw_coordinates=True, mode="validation",
            volume_augmentations=NS(), normalize_color=normalize)
    me.load_self_train_masks = lambda *a, **k: ds.SemanticSegmentationFreeDataset.load_self_train_masks(me, *a, **k)
    me.__len__ = lambda: 1
    cls = ds.SemanticSegmentationFreeDataset
    # (a) the exported cloud differs from the scene's points: 1-NN transfer.  The reference queries its 3-D tree with
    # the [N,12] point table, which scipy rejects — the branch only works for a caller that passes xyz, so that is what
    # the fixture records.
    for nsd, drop in ((5, False), (2, False), (8, True)):
        me.num_self_train_data = nsd
        merged = cls.load_self_train_masks(me, 0, pts[:, :3], free, drop_original=drop)
        out[f"merge/{nsd}_{int(drop)}"] = merged.astype(np.float32)
        print("merge", nsd, drop, merged.shape)
    me.num_self_train_data = 5
    # (b) the usual case: the export was made on this very cloud (trainer.py:749 saves full_res_coords)
    same = np.stack([obj == 1, (obj == 0) | (obj == 2), obj == 3, obj == 5, (obj == 5) | (obj == 8), obj == 9], 1)
    np.save(f"{tmp}/freemasks/scene0001_00_cloud.npy", pts[:, :3])
    np.save(f"{tmp}/freemasks/scene0001_00_masks.npy", same)
    out["st_masks_same"] = np.packbits(same, axis=1)

    class Fake(NS):
        def __len__(self):
            return 1
    fake = Fake(**vars(me))
    item = cls.__getitem__(fake, 0)
    names = ("coordinates", "features", "freemasks", "scene_name", "raw_color", "raw_normals", "raw_coordinates", "idx")
    for k, v in zip(names, item):
        if k not in ("scene_name", "idx"):
            out[f"item/{k}"] = np.asarray(v)
    assert item[3] == "scene0001_00" and item[7] == 0 and item[8] == []
    print("item", [np.asarray(v).shape for v in item[:3]])

    # (c) TRAIN mode (freemask_semseg.py:334-406): centring + random shift (numpy's global generator), axis flips and
    # the elastic-distortion gate (python's `random`), two elastic distortions, colour drop, normalisation.  The
    # volumentations / albumentations pipelines are third-party packages that are not installed: identity stand-ins, so
    # the fixture pins the reference's OWN steps and their random-number consumption.
    import random as pyrandom

    class IdVolume:
        transforms = [None]

        def __call__(self, points, normals, features, labels):
            return {"points": points, "normals": normals, "features": features, "labels": labels}

    for seed in (3, 4, 11):
        tr = Fake(**vars(me))
        tr.mode, tr.volume_augmentations = "train", IdVolume()
        tr.image_augmentations = lambda image: {"image": image}
        tr.flip_in_center, tr.is_elastic_distortion, tr.point_per_cut = False, True, 0
        tr.resample_points, tr.noise_rate, tr.color_drop, tr.max_cut_region = 0, 0, 0.3, 0
        np.random.seed(seed)
        pyrandom.seed(seed)
        item = cls.__getitem__(tr, 0)
        for k, v in zip(names, item):
            if k in ("coordinates", "features", "freemasks"):
                out[f"train{seed}/{k}"] = np.asarray(v)
        out[f"train{seed}/rng_after"] = np.array([np.random.random(), pyrandom.random()])
        print("train item", seed, np.asarray(item[0]).dtype, np.asarray(item[0])[:2], np.asarray(item[1])[0, :3])
    np.savez_compressed(os.path.join(HERE, "dataset.npz"), **out)


def make_elastic():
    stub("open3d", "felzenszwalb_cpp", "albumentations", "volumentations", "imageio", "MinkowskiEngine", "plyfile",
         "natsort", "loguru", "fire", "torch_scatter", "hydra")
    os.chdir(REF)
    sys.path.insert(0, REF)
    semseg = importlib.import_module("datasets.semseg")
    rng = np.random.default_rng(5)
    out = {}
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        pts = np.concatenate([rng.uniform(-3.1, 4.3, (5000, 1)), rng.uniform(0.2, 5.7, (5000, 1)),
                              rng.uniform(-0.1, 2.6, (5000, 1)), rng.uniform(0, 1, (5000, 3))], 1).astype(dtype)
        out[f"{name}/points"] = pts.copy()
        np.random.seed(1234)
        res = pts.copy()
        drawn = []
        orig = np.random.randn
        np.random.randn = lambda *a: drawn.append(orig(*a)) or drawn[-1]
        try:
            for granularity, magnitude in ((0.2, 0.4), (0.8, 1.6)):       # freemask_semseg.py:356-361
                res = semseg.elastic_distortion(res, granularity, magnitude)
        finally:
            np.random.randn = orig
        out[f"{name}/result"] = res
        for j, d in enumerate(drawn):
            out[f"{name}/noise{j}"] = d.astype(np.float32)
        print(name, res.dtype, [d.shape for d in drawn], float(np.abs(res[:, :3] - pts[:, :3]).max()))
    np.savez_compressed(os.path.join(HERE, "elastic.npz"), **out)


def make_state_dict():
    """The parameter / buffer names and shapes of the reference's OWN module tree — models/res16unet.py:Res16UNet34C and
    models/mask3d.py:Mask3D with conf/model/mask3d.yaml's values — as the contract "published checkpoints load by key".
    The reference's classes are instantiated in place; MinkowskiEngine (not in the reference tree) is replaced by
    parameter-only stand-ins that follow ME 0.5.4's published layer definitions: MinkowskiConvolution[Transpose] owns
    `kernel` f32[K, Cin, Cout] (f32[Cin, Cout] for a kernel volume of 1) and `bias` f32[1, Cout]; MinkowskiBatchNorm
    wraps `bn = nn.BatchNorm1d`.  The module NAMES (conv0p1s1, block1.0.conv1, cross_attention.0.2.multihead_attn ...)
    and channel widths are the reference's."""
    import json
    from enum import Enum
    from types import SimpleNamespace
    import math

    me = types.ModuleType("MinkowskiEngine")

    class RegionType(Enum):
        HYPER_CUBE = 0
        HYPER_CROSS = 1
        CUSTOM = 2

    def _vol(ks, D):
        ks = [ks] * D if isinstance(ks, int) else list(ks)
        return int(math.prod(ks))

    class KernelGenerator:
        def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False, region_type=RegionType.HYPER_CUBE,
                     region_offsets=None, expand_coordinates=False, axis_types=None, dimension=-1):
            assert region_type == RegionType.HYPER_CUBE
            self.kernel_volume = _vol(kernel_size, dimension)

    class _ConvBase(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                     kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=-1):
            super().__init__()
            K = kernel_generator.kernel_volume if kernel_generator is not None else _vol(kernel_size, dimension)
            self.kernel = nn.Parameter(torch.zeros(K, in_channels, out_channels) if K > 1
                                       else torch.zeros(in_channels, out_channels))
            if bias:
                self.bias = nn.Parameter(torch.zeros(1, out_channels))

    class MinkowskiConvolution(_ConvBase):
        pass

    class MinkowskiConvolutionTranspose(_ConvBase):
        pass

    class MinkowskiBatchNorm(nn.Module):
        def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__()
            self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                     track_running_stats=track_running_stats)

    class _NoParams(nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    class MinkowskiNetwork(nn.Module):
        def __init__(self, D):
            super().__init__()
            self.D = D

    for name, obj in dict(RegionType=RegionType, KernelGenerator=KernelGenerator, MinkowskiConvolution=MinkowskiConvolution,
                          MinkowskiConvolutionTranspose=MinkowskiConvolutionTranspose, MinkowskiBatchNorm=MinkowskiBatchNorm,
                          MinkowskiNetwork=MinkowskiNetwork).items():
        setattr(me, name, obj)
    for name in ("MinkowskiReLU", "MinkowskiAvgPooling", "MinkowskiSumPooling", "MinkowskiInstanceNorm",
                 "MinkowskiGlobalPooling", "MinkowskiDropout", "MinkowskiLeakyReLU", "MinkowskiELU", "MinkowskiSigmoid",
                 "MinkowskiBroadcastMultiplication", "MinkowskiGlobalSumPooling", "MinkowskiLinear"):
        setattr(me, name, type(name, (_NoParams,), {}))
    ops_mod = types.ModuleType("MinkowskiEngine.MinkowskiOps")
    ops_mod.cat = lambda *a, **k: None
    pool_mod = types.ModuleType("MinkowskiEngine.MinkowskiPooling")
    pool_mod.MinkowskiAvgPooling = me.MinkowskiAvgPooling
    me.MinkowskiOps, me.MinkowskiPooling = ops_mod, pool_mod
    sys.modules["MinkowskiEngine"] = me
    sys.modules["MinkowskiEngine.MinkowskiOps"] = ops_mod
    sys.modules["MinkowskiEngine.MinkowskiPooling"] = pool_mod
    stub("custom_cuda_utils", "detectron2", "detectron2.utils", "detectron2.utils.comm", "detectron2.projects",
         "detectron2.projects.point_rend", "detectron2.projects.point_rend.point_features", "hydra", "torch_scatter",
         "pointnet2", "pointnet2._ext", "torchvision", "third_party", "third_party.pointnet2",
         "third_party.pointnet2.pointnet2_utils")
    os.chdir(REF)
    sys.path.insert(0, REF)
    res16unet = importlib.import_module("models.res16unet")
    mask3d = importlib.import_module("models.mask3d")
    out = {}
    # conf/model/mask3d.yaml: config.backbone = Res16UNet34C(in_channels = data.in_channels (3), out_channels = data.num_labels,
    # config = {dialations, conv1_kernel_size 3, bn_momentum 0.02}, out_fpn = true)
    cfg = SimpleNamespace(dialations=[1, 1, 1, 1], dilations=[1, 1, 1, 1], conv1_kernel_size=3, bn_momentum=0.02)
    for name in ("Res16UNet34C", "Res16UNet14"):
        bb = getattr(res16unet, name)(in_channels=3, out_channels=20, config=cfg, out_fpn=True)
        out[name] = sorted([k, list(v.shape)] for k, v in bb.state_dict().items())
    bb = res16unet.Res16UNet34C(in_channels=3, out_channels=20, config=cfg, out_fpn=True)
    m = mask3d.Mask3D(config=SimpleNamespace(backbone=bb), hidden_dim=128, num_queries=100, num_heads=8, dim_feedforward=1024,
                      sample_sizes=[200, 800, 3200, 12800, 51200], shared_decoder=True, num_classes=3, num_decoders=3,
                      dropout=0.0, pre_norm=False, positional_encoding_type="fourier", non_parametric_queries=True,
                      train_on_segments=True, normalize_pos_enc=True, use_level_embed=False, scatter_type="mean",
                      hlevels=[0, 1, 2, 3], use_np_features=False, voxel_size=0.02, max_sample_size=False,
                      random_queries=False, gauss_scale=1.0, random_query_both=False, random_normal=False)
    out["Mask3D"] = sorted([k, list(v.shape)] for k, v in m.state_dict().items())
    with open(os.path.join(HERE, "state_dict_keys.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
    for k, v in out.items():
        print(k, len(v), "entries", sum(int(np.prod(sh)) for _, sh in v), "elements")


if __name__ == "__main__":
    cwd = os.getcwd()
    if len(sys.argv) > 1 and sys.argv[1] == "state_dict":
        make_state_dict()
    elif len(sys.argv) > 1 and sys.argv[1] == "ncut":
        make_ncut(import_reference_ncut())
    elif len(sys.argv) > 1 and sys.argv[1] == "ncut_l2":
        make_ncut_l2(import_reference_ncut())
    elif len(sys.argv) > 1 and sys.argv[1] == "ncut_b":
        make_ncut_b(import_reference_ncut())
    elif len(sys.argv) > 1 and sys.argv[1] == "elastic":
        make_elastic()
    elif len(sys.argv) > 1 and sys.argv[1] == "dataset":
        make_dataset(import_reference_dataset())
    elif len(sys.argv) > 1 and sys.argv[1] == "export":
        make_export(import_reference_trainer())
    elif len(sys.argv) > 1 and sys.argv[1] == "felz":
        make_felz()
    elif len(sys.argv) > 1 and sys.argv[1] == "felz_build":
        make_felz_build()
    elif len(sys.argv) > 1 and sys.argv[1] == "decoder_pass":
        make_decoder_pass(import_reference_models())
    elif len(sys.argv) > 1 and sys.argv[1] == "aggregate":
        make_aggregate(import_reference_ncut())
    else:
        mods = import_reference_models()
        make_criterion(mods)
        make_posenc(mods)
        make_decoder_layers(mods)
    os.chdir(cwd)
