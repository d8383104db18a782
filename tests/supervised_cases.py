"""Readers of tests/golden/instance_targets.npz (written by tests/golden/make_golden_supervised.py from the reference's
own get_instance_masks / voxelize) shared by the CPU and GPU tests of the supervised collate."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_targets.npz")
MODES = ("train", "validation", "test")


def unpack(z, key):
    shape = tuple(int(v) for v in z[key + "/shape"])
    return np.unpackbits(z[key + "/bits"])[:int(np.prod(shape))].reshape(shape).astype(bool)


def stored_targets(z, key):
    out = []
    for b in range(int(z[key + "/count"])):
        entry = {}
        for name in ("labels", "point2segment"):
            if f"{key}/{b}/{name}" in z:
                entry[name] = z[f"{key}/{b}/{name}"]
        for name in ("masks", "segment_mask"):
            if f"{key}/{b}/{name}/bits" in z:
                entry[name] = unpack(z, f"{key}/{b}/{name}")
        out.append(entry)
    return out


def stored_case(z, name):
    n = int(z[f"case/{name}/n_tables"])
    tables = [z[f"case/{name}/table{b}"] for b in range(n)]
    n_seg = [int(z[f"case/{name}/n_segments{b}"]) for b in range(n)]
    return (tables, None if n_seg[0] < 0 else n_seg, [int(c) for c in z[f"case/{name}/filter"]],
            int(z[f"case/{name}/offset"]), int(z[f"case/{name}/threshold"]), stored_targets(z, f"case/{name}/target"))


def assert_targets_equal(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} targets, expected {len(want)}"
    for b, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            a = g[k]
            a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
            assert a.shape == v.shape and a.dtype == v.dtype, f"{what} scene {b} {k}: {a.shape} {a.dtype} vs {v.shape} {v.dtype}"
            assert np.array_equal(a, v), f"{what} scene {b} {k} differs"


def voxel_batch(z):
    return [(z[f"vox/scene{b}/xyz"], z[f"vox/scene{b}/feats"], z[f"vox/scene{b}/labels"], f"scene{b}", None, None,
             z[f"vox/scene{b}/xyz"].astype(np.float32), b) for b in range(2)]
