"""Inputs of the FreeMask kernel tests (tests/test_gpu_freemask.py) and the rule for the entries whose bit an f32
evaluation may legitimately get differently from float64 (checked on the f64 values alone by
tests/test_freemask_host.py).

Shapes (Q, K, C): the smallest possible; odd sizes below one tile; exactly one 64-query / 64-key tile with a wide C;
more than one tile both ways with tails (257 keys = 4 words + 1 bit, 9 32-key tiles: an odd number, so the last u32
of every row is a padding tile); more than one workgroup and more than one key split.  Every case has all-zero keys
(K = 1: its only key), (130, 257, 96) has an all-zero query row.
"""
import numpy as np

SHAPES = [(1, 1, 1), (37, 70, 5), (64, 64, 384), (130, 257, 96), (300, 4100, 96)]
# the widest C (the largest LDS tile) and a C that is no multiple of 8 and more than one wave wide (the scalar key loads)
EXTRA_SHAPES = [(33, 65, 512), (70, 33, 100)]
ZERO_QUERY = {(130, 257, 96): 7}
THRESHOLD = 0.35
SKIP_SHARE_MAX = 1e-3


def dot_bound(C):
    """f32 bound on |q^ . k^ - exact|: C products and sums plus the two normalisations, 8x headroom."""
    return 8.0 * (C + 4) * 2.0 ** -24


def make_case(Q, K, C, seed=0):
    """Clustered features (six centres, noise 0.3 per channel, random magnitudes), ~5 % all-zero keys, coordinates."""
    rng = np.random.default_rng(1000 + seed + Q * 7 + K * 13 + C)
    centres = rng.standard_normal((6, C))
    fk = centres[rng.integers(0, 6, K)] + 0.3 * rng.standard_normal((K, C))
    fq = centres[rng.integers(0, 6, Q)] + 0.3 * rng.standard_normal((Q, C))
    fk *= rng.uniform(0.25, 4.0, (K, 1))
    fq *= rng.uniform(0.25, 4.0, (Q, 1))
    zero = rng.permutation(K)[:max(1, round(0.05 * K))]
    fk[zero] = 0.0
    if (Q, K, C) in ZERO_QUERY:
        fq[ZERO_QUERY[(Q, K, C)]] = 0.0
    coords = rng.integers(-40, 200, (K, 3)).astype(np.int32)
    return fk.astype(np.float32), fq.astype(np.float32), coords


def skip_mask(a64, lo64, hi64, fq, C, thr=THRESHOLD):
    """bool[Q,K]: entries whose bit is not compared.  delta_row = dot_bound / (rowmax - rowmin): the dot-product bound
    carried through the min-max.  Rows whose normalised values are exactly 0 in ANY arithmetic get delta 0 (nothing
    skipped) instead of the formula's 1/0: an all-zero query (every product is 0) and K = 1 (min = max = the value
    itself, so a - min is 0) — stricter than the formula, which would skip those rows whole."""
    rng = hi64 - lo64
    exact = np.all(np.asarray(fq) == 0, axis=1) | (a64.shape[1] == 1)
    with np.errstate(divide="ignore"):
        delta = np.where(exact, 0.0, dot_bound(C) / rng)
    return (np.abs(a64 - thr) <= delta[:, None]) & ~exact[:, None]
