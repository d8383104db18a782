"""Shared by test_selftrain_host.py and test_gpu_selftrain.py: numpy restatements of the bit-row layout and of the
self-training merge, and merge cases in which every branch of the rule is planted.

Bit rows: mask j of an [n, k] table is row j of u64[k, ceil(n / 64)]; point r is bit r % 64 of word r / 64; the bits
past n are zero.

The merge, in this project's words: the exported instances are visited in file order.  An instance is taken when it
is not empty and strictly more than half of its points are not covered yet; what is taken is only its uncovered
part, and that part is covered from then on.  After `max_add` instances the walk ends."""
import functools

import numpy as np

BRANCHES = ("added", "empty", "tie", "less", "cap")
MAX_ADD = (0, 1, 5)
KP = (0, 1, 100)


def numpy_pack(masks):
    """[n, k] (non-zero = set) -> u64[k, ceil(n / 64)]."""
    m = np.asarray(masks) != 0
    n, k = m.shape
    W = (n + 63) // 64
    pad = np.zeros((k, W * 64), bool)
    pad[:, :n] = m.T
    return np.packbits(pad.reshape(k, W, 64), axis=2, bitorder="little").reshape(k, W * 8).view("<u8").reshape(k, W)


def numpy_unpack(bits, n):
    """u64[k, W] -> bool[n, k]; the bits past n are dropped."""
    b = np.ascontiguousarray(np.asarray(bits, dtype="<u8"))
    k = b.shape[0]
    flat = np.unpackbits(b.view(np.uint8).reshape(k, -1), axis=1, bitorder="little")
    return flat[:, :n].T.astype(bool)


def numpy_popcount(bits):
    b = np.ascontiguousarray(np.asarray(bits, dtype="<u8"))
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[0], -1), axis=1).sum(1).astype(np.int32)


def numpy_merge(st, covered, max_add):
    """st bool[n, kp], covered bool[n] -> {"picked": [j...], "fresh": bool[n, len(picked)], "covered": bool[n] at the
    end, "census": how often each branch was taken}.  "cap" counts the instances that were still waiting when the
    walk ended at `max_add` and that the rule would have taken against the final cover."""
    st = np.asarray(st, bool)
    covered = np.asarray(covered, bool).copy()
    census = dict.fromkeys(BRANCHES, 0)
    picked, fresh = [], []
    j = 0
    while j < st.shape[1] and len(picked) < max_add:
        size = int(st[:, j].sum())
        new = st[:, j] & ~covered
        gain = int(new.sum())
        if size == 0:
            census["empty"] += 1
        elif 2 * gain == size:
            census["tie"] += 1
        elif 2 * gain < size:
            census["less"] += 1
        else:
            census["added"] += 1
            picked.append(j)
            fresh.append(new)
            covered |= new
        j += 1
    for jj in range(j, st.shape[1]):
        size = int(st[:, jj].sum())
        if size > 0 and 2 * int((st[:, jj] & ~covered).sum()) > size:
            census["cap"] += 1
    out = np.stack(fresh, 1) if fresh else np.zeros((st.shape[0], 0), bool)
    return {"picked": picked, "fresh": out, "covered": covered, "census": census}


def _planted(n, seed, kp=100):
    """n >= 256.  Points [0, n/4) start covered.  The first columns hold, in this order: an instance that is taken, an
    empty one, a tie against the initial cover, one with less than half new, a tie that exists only because column 0
    was taken (half of it lies in column 0's new part), one with exactly one point more than a tie (taken), then six
    disjoint instances that are all eligible (more than any `max_add` here leaves room for); the rest is random."""
    rng = np.random.default_rng(seed)
    q = n // 4
    covered = np.zeros(n, bool)
    covered[:q] = True
    st = np.zeros((n, kp), bool)
    free = np.arange(q, n)
    blocks = np.array_split(free, 16)                       # disjoint uncovered regions, each >= 12 points
    g = min(10, len(blocks[0]) // 2)
    st[blocks[0][:g], 0] = True                             # taken: g new, 2 covered
    st[:2, 0] = True
    #   column 1 stays empty
    st[blocks[1][:g], 2] = True                             # tie: g new, g covered
    st[2:2 + g, 2] = True
    st[blocks[2][:3], 3] = True                             # less: 3 new, 8 covered
    st[10:18, 3] = True
    st[blocks[0][:g // 2], 4] = True                        # tie only after column 0 was taken
    st[blocks[3][:g // 2], 4] = True
    st[blocks[4][:g + 1], 5] = True                         # one more than a tie: taken
    st[20:20 + g, 5] = True
    for c in range(6):
        st[blocks[5 + c], 6 + c] = True                     # eligible, disjoint
    st[n - 1, 11] = True                                    # the last point, in the tail word
    dens = rng.uniform(0.0, 0.2, kp - 12)
    st[:, 12:] = rng.random((n, kp - 12)) < dens
    st[:, 20] = False                                       # one more empty instance, further on
    return st, covered


def _random(n, seed, kp=100):
    rng = np.random.default_rng(seed)
    return rng.random((n, kp)) < rng.uniform(0.0, 0.6, kp), rng.random(n) < 0.3


@functools.lru_cache(maxsize=None)
def merge_cases():
    """[(name, st bool[n, 100], covered bool[n])]: tiny and tile-edge sizes at random, planted branches at sizes of
    several words, and one case with more words (1094) than the merge workgroup has threads."""
    cases = [(f"random{n}", *_random(n, 100 + n)) for n in (1, 63, 64, 65, 130)]
    cases += [(f"planted{n}", *_planted(n, n)) for n in (256, 1000, 4099, 70000)]
    return cases


@functools.lru_cache(maxsize=None)
def merge_expectations():
    """{(name, max_add, kp): numpy_merge(...)} for every case and every `max_add` x `kp` of the tests."""
    return {(name, a, kp): numpy_merge(st[:, :kp], cov, a)
            for name, st, cov in merge_cases() for a in MAX_ADD for kp in KP}
