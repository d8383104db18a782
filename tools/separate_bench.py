"""Cost of `general.separate_instances` (trainer/separate.py) at scene size: one 240 k-point scene, 100 kept instances,
about 3 000 segments (the LDS components kernel) and about 10 000 (the wide one) — the device path against the
per-instance numpy loop of the restatement tests/separate_ref.py (what the reference's Python loop does: a set scan per
instance, one np.isin over all points per part).

    python tools/separate_bench.py [--calls 20] [--out profiles/separate_instances.txt]

Segments are the cells of a square grid, adjacent (both directions listed) to their four neighbours; an instance is
one, two or three separate rectangles of cells, one of them only partly covered.  Per size: median (min ... max) of
`--calls` calls between HIP events after 2 warm-ups, for the whole call (ids -> indices, CSR, adjacency, the three
kernels) and for each kernel stage alone, called as `separate_instances` calls them (`check_range=False`: it built the
CSR and the indices itself), the peak device memory above the inputs, and the numpy loop's wall time."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import separate_ref as R  # noqa: E402
from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.pseudo_masks import freemask as fm  # noqa: E402
from unscene3d_amd.trainer.separate import separate_columns, separate_instances  # noqa: E402


def scene(side, n_points=240_000, n_inst=100, seed=0):
    rng = np.random.default_rng(seed)
    S = side * side
    ids = np.arange(S, dtype=np.int64) * 3 + 11                    # not contiguous
    seg_index = np.concatenate([np.arange(S), rng.integers(0, S, n_points - S)])[rng.permutation(n_points)]
    cell = np.arange(S).reshape(side, side)
    right = np.stack([cell[:, :-1].ravel(), cell[:, 1:].ravel()], 1)
    down = np.stack([cell[:-1].ravel(), cell[1:].ravel()], 1)
    pairs = np.concatenate([right, down])
    conn = ids[np.concatenate([pairs, pairs[:, ::-1]])]
    masks = np.zeros((n_points, n_inst), bool)
    for j in range(n_inst):
        chosen = np.zeros(S, bool)
        for _ in range(1 + j % 3):
            h, w = rng.integers(2, 7, 2)
            r, c = rng.integers(0, side - h), rng.integers(0, side - w)
            chosen[cell[r:r + h, c:c + w].ravel()] = True
        masks[:, j] = chosen[seg_index]
        partial = np.nonzero(masks[:, j] & (seg_index == np.nonzero(chosen)[0][0]))[0]
        masks[partial[1::2], j] = False                            # a partly covered segment
    return ids[seg_index], conn, masks


def timed(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return f"{np.median(ms):8.3f} ms ({min(ms):.3f} ... {max(ms):.3f})"


def bench(side, calls, dev):
    seg, conn, masks = scene(side)
    N, K = masks.shape
    t_masks, t_seg = torch.from_numpy(masks).to(dev), torch.from_numpy(seg).to(dev)
    t_conn = torch.from_numpy(conn).to(dev)
    out, src = separate_instances(t_masks, t_seg, t_conn)
    uniq, idx = torch.unique(t_seg, return_inverse=True)
    S = uniq.numel()
    csr = ops.segment_csr(idx.contiguous(), S)
    idx32 = idx.to(torch.int32)
    adj_off, adj = fm.segment_adjacency(t_conn, uniq, mutual=True)
    rows = torch.arange(K, dtype=torch.int32, device=dev)
    bits = ops.mask_columns_to_segment_bits(t_masks, csr)
    label, _ = fm.mask_components(bits, rows, adj_off, adj, n_segments=S, kernel="auto")
    parts = torch.nonzero(label == torch.arange(S, dtype=torch.int32, device=dev))
    p_src, p_root = parts[:, 0].to(torch.int32).contiguous(), parts[:, 1].to(torch.int32).contiguous()
    lines = [f"N = {N} points, K = {K} instances, S = {S} segments, {conn.shape[0]} pairs -> R = {out.shape[1]} parts; "
             f"components kernel: {'wide (global memory)' if S > fm.lib.usc_mask_bits_max_segments() else 'LDS'}"]
    lines.append(f"  separate_instances (whole call)      {timed(lambda: separate_instances(t_masks, t_seg, t_conn), calls)}")
    lines.append(f"  separate_columns (the three kernels) {timed(lambda: separate_columns(t_masks, csr, idx32, adj_off, adj, check_range=False), calls)}")
    lines.append(f"    columns -> segment bits            {timed(lambda: ops.mask_columns_to_segment_bits(t_masks, csr, check_range=False), calls)}")
    lines.append("    components (with its host checks)  "
                 f"{timed(lambda: fm.mask_components(bits, rows, adj_off, adj, n_segments=S, kernel='auto'), calls)}")
    lines.append("    parts -> columns                   "
                 f"{timed(lambda: ops.segment_parts_to_columns(label, p_src, p_root, idx32, check_range=False), calls)}")
    del out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, src = separate_columns(t_masks, csr, idx32, adj_off, adj)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = bits.numel() * 8 + label.numel() * 4 + out.numel()
    lines.append(f"  peak above the inputs {peak} bytes (bits {bits.numel() * 8} + labels {label.numel() * 4} + result "
                 f"{out.numel()} = {bound}); one [N, K] byte table is {N * K}")
    t0 = time.perf_counter()
    want, want_src, _, _ = R.separate_ref(masks, seg, conn)
    host = time.perf_counter() - t0
    same = np.array_equal(out.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), want_src)
    lines.append(f"  numpy loop of the restatement        {host * 1e3:8.1f} ms (one call); results equal: {same}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from unscene3d_amd import _lib
    lines = [f"tools/separate_bench.py --calls {a.calls}; {torch.cuda.get_device_name(0)}; "
             f"library: {_lib.lib.usc_build_info().decode()}"]
    for side in (55, 100):
        lines += bench(side, a.calls, dev)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
