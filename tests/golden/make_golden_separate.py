"""Golden generator for `general.separate_instances` — runs only where the reference tree exists (see make_golden.py).

    python tests/golden/make_golden_separate.py

Drives the reference's own `separate_segments` (utils/point_cloud_utils.py:82-121, imported in place with the stub
modules of make_golden.py) on one planted scene, once per instance as the export step does (trainer/trainer.py:624-639),
and writes tests/golden/separate_instances.npz.  The function is imported and called in place; its two inputs (the
mutual-neighbour sets and the per-instance mask over the sorted unique ids) are built here from their meaning.  Nothing
of the reference is copied; the fixture is data.

Where the export step (:629) indexes the S-long mask with the raw segment ids, which is only meaningful for ids
0 .. S-1, the ids are looked up in the sorted unique ids here: the planted ids are not contiguous.

The scene (1 200 points, 80 segments of 15 points, ids 7, 10, 13, ... with gaps):
  A = segments 0..9 and B = 10..19, two paths of mutual pairs; (9 -> 10) is listed in ONE direction only
  C = 20..30, a path; segment 25 is its bridge
  D = 31..45 and 46..60, two paths, joined only by the mutual pair (31, 60): the scan meets 60 last and has to merge
      two blobs
  61..79: isolated, plus pairs naming unknown ids and a self pair
Instances: 0 = A + B (two groups that the one-directional pair must not join); 1 = C without segment 25 (the bridge is
outside the mask: two parts); 2 = segment 40 alone; 3 = HALF the points of segment 50 and all of 51 (the part holds all
of 50); 4 = all of D (one part through the late bridge); 5 = a seeded random subset of D's segments (several
intervals).  The script asserts that on this scene the reference's scan gives the true connected components."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF, stub  # noqa: E402


def planted_scene():
    rng = np.random.default_rng(20260)
    S, per = 80, 15
    ids = 7 + 3 * np.arange(S, dtype=np.int64) + (np.arange(S) // 9) * 11      # sorted, gaps of different widths
    seg = np.repeat(ids, per)[rng.permutation(S * per)]
    pairs = []

    def path(lo, hi):
        for s in range(lo, hi):
            pairs.extend([(ids[s], ids[s + 1]), (ids[s + 1], ids[s])])

    path(0, 9)
    path(10, 19)
    pairs.append((ids[9], ids[10]))                         # one direction only: must not connect
    path(20, 30)
    path(31, 45)
    path(46, 60)
    pairs.extend([(ids[31], ids[60]), (ids[60], ids[31])])
    pairs.extend([(ids[61], ids[61]), (ids[62], 5), (5, ids[62]), (9999, ids[63]), (ids[63], 9999)])
    pairs.append((ids[70], ids[64]))                        # one direction, descending
    conn = np.array(pairs, np.int64)[rng.permutation(len(pairs))]

    def points_of(segments):
        return np.isin(seg, ids[np.asarray(segments)])

    K = 6
    masks = np.zeros((len(seg), K), bool)
    masks[:, 0] = points_of(range(0, 20))
    masks[:, 1] = points_of([s for s in range(20, 31) if s != 25])
    masks[:, 2] = points_of([40])
    half = np.nonzero(seg == ids[50])[0][::2]
    masks[half, 3] = True
    masks[:, 3] |= points_of([51])
    masks[:, 4] = points_of(range(31, 61))
    masks[:, 5] = points_of(np.nonzero(rng.random(30) < 0.6)[0] + 31)
    return seg, conn, masks


def reference_parts(seg, conn, masks):
    stub("open3d", "plyfile")
    sys.path.insert(0, REF)
    from utils.point_cloud_utils import separate_segments

    # the function's two inputs, built here from their meaning: per id the ids it is listed with in BOTH directions,
    # and per instance the ids (as a mask over the sorted unique ids) that any of its points carries
    uniq = np.unique(seg)
    listed = {(int(a), int(b)) for a, b in conn}
    mutual = {s: {b for a, b in listed if a == s and (b, a) in listed} for s in uniq.tolist()}
    neighbours = {s: mutual[int(s)] for s in uniq}          # keyed like the ids the function iterates over
    cols, src, part_ids, part_off = [], [], [], [0]
    for j in range(masks.shape[1]):
        touched = np.isin(uniq, seg[masks[:, j]])           # see the docstring: ids looked up, not used as indices
        for part in separate_segments(touched, uniq, neighbours):
            cols.append(np.isin(seg, part))
            src.append(j)
            part_ids.extend(sorted(int(p) for p in part))
            part_off.append(len(part_ids))
    return (np.stack(cols, axis=1), np.array(src, np.int64), np.array(part_ids, np.int64), np.array(part_off, np.int64))


def main():
    import separate_ref as R

    seg, conn, masks = planted_scene()
    cols, src, part_ids, part_off = reference_parts(seg, conn, masks)
    # on this scene the reference's scan equals the true components (as sets per instance)
    want_cols, want_src, want_parts, uniq = R.separate_ref(masks, seg, conn)
    for j in range(masks.shape[1]):
        got = {tuple(part_ids[part_off[r]:part_off[r + 1]]) for r in np.nonzero(src == j)[0]}
        want = {tuple(uniq[p]) for p, s in zip(want_parts, want_src) if s == j}
        assert got == want, f"instance {j}: the reference's scan differs from the true components"
    assert np.bincount(src, minlength=6).tolist() == [2, 2, 1, 1, 1, np.bincount(want_src, minlength=6)[5]]
    np.savez_compressed(os.path.join(HERE, "separate_instances.npz"), seg=seg, conn=conn, masks=masks, ref_masks=cols,
                        ref_src=src, ref_part_ids=part_ids, ref_part_off=part_off)
    print(f"separate_instances.npz: {len(seg)} points, {len(np.unique(seg))} segments, {masks.shape[1]} instances -> "
          f"{cols.shape[1]} parts {np.bincount(src).tolist()}")


if __name__ == "__main__":
    main()
