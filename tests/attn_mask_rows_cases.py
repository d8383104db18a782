"""Inputs shared by tests/test_gpu_attn_mask_rows.py and tests/test_attn_mask_rows_host.py: the hand-built two-level tree
whose logits make the summation order of the pooling chain visible, and the chain's arithmetic in numpy f32."""
import numpy as np

F32 = np.float32
BIG = F32(1e8)          # ulp(1e8) = 8 in f32: an O(1) term added to it is lost, added after it cancelled it survives


def emulate_chain(logits, tables, reverse=()):
    """The bytes of the pooling chain in numpy f32: per node acc = 0, acc += child for the present slots k = 0..7 in order
    (levels listed in `reverse`: k = 7..0), mean = acc * (1 / cnt) rounded to f32 at every level, and after the last
    level sigmoid(mean) < 0.5.  logits f32[rows, q]; tables: i32[8, n_j], the first one holding rows of `logits`."""
    cur = np.asarray(logits, dtype=F32)
    for level, tab in enumerate(tables):
        n = tab.shape[1]
        out = np.zeros((n, cur.shape[1]), dtype=F32)
        for p in range(n):
            acc = np.zeros(cur.shape[1], dtype=F32)
            cnt = 0
            for k in (range(7, -1, -1) if level in reverse else range(8)):
                ch = int(tab[k, p])
                if ch >= 0:
                    cnt += 1
                    acc = (acc + cur[ch]).astype(F32)
            inv = F32(1.0) / F32(max(cnt, 1))
            out[p] = (acc * inv).astype(F32)
        cur = out
    return (F32(1.0) / (F32(1.0) + np.exp(-cur, dtype=F32))) < F32(0.5)


def order_tree(q=16, seed=3):
    """-> (logits f32[65, q], [tab0 i32[8, 9], tab1 i32[8, 2]]): coarse voxel 0 has all 8 children, each with all 8
    leaves (rows 0..63); coarse voxel 1 has one child (slot 5) with one leaf (slot 2, row 64).
    Per column: the leaves of a "mixed" child are 4 multiples of 0.25 and two cancelling pairs +-1e8 at random slots (the
    small terms that are added while a 1e8 is in the accumulator are lost: another slot order loses other terms); the 8
    leaves of a "big" child are all +1e8 or all -1e8 (its mean is exactly +-1e8) and big children come in cancelling
    pairs, which does to the coarse voxel's sum what the pairs do to a mixed child's.  Every nonzero mean of the tree is
    a multiple of 2^-8 in magnitude: sigmoid(mean) < 0.5 does not hang on the last bit of expf."""
    rng = np.random.default_rng(seed)
    logits = np.zeros((65, q), dtype=F32)
    for col in range(q):
        big_children = rng.permutation(8)[:4]              # two cancelling pairs of big children
        for j, child in enumerate(big_children):
            logits[child * 8:child * 8 + 8, col] = BIG if j % 2 == 0 else -BIG
        for child in sorted(set(range(8)) - set(big_children.tolist())):
            slots = rng.permutation(8)
            vals = np.empty(8, dtype=F32)
            vals[slots[:4]] = [BIG, -BIG, BIG, -BIG]
            vals[slots[4:]] = rng.integers(-12, 13, 4).astype(F32) * F32(0.25)
            logits[child * 8:child * 8 + 8, col] = vals
        logits[64, col] = F32(rng.integers(-8, 9)) * F32(0.5)
    tab0 = np.full((8, 9), -1, dtype=np.int32)
    tab0[:, :8] = np.arange(64, dtype=np.int32).reshape(8, 8).T      # child c, slot k -> leaf row 8 c + k
    tab0[2, 8] = 64
    tab1 = np.full((8, 2), -1, dtype=np.int32)
    tab1[:, 0] = np.arange(8, dtype=np.int32)
    tab1[5, 1] = 8
    return logits, [tab0, tab1]
