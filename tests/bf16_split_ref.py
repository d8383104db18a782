"""Split-bf16 oracle of the training-precision tests (csrc/spconv_bf16.hip): the planes of an f32 value, the kept plane
products, and a float64 convolution that sums exactly those products.  Every product of two planes is exact in f32
(and in float64), so the kernel differs from this oracle only by its f32 accumulation."""
import numpy as np

from bf16_ref import bf16_bits, bf16_round


def split_planes(a, P) -> np.ndarray:
    """float32 values -> float32[P, ...] planes, each exactly a bf16 value: x0 = bf16(x), x1 = bf16(x - x0),
    x2 = bf16(x - x0 - x1); round to nearest even, subtractions in f32.  A value whose x0 is not finite keeps x0 and
    gets zero in the other planes."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    planes = np.zeros((P,) + a.shape, np.float32)
    planes[0] = bf16_round(a)
    ok = np.isfinite(planes[0])
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(ok, a - planes[0], np.float32(0)).astype(np.float32)
        for p in range(1, P):
            planes[p] = bf16_round(r)
            r = (r - planes[p]).astype(np.float32)
    return planes


def split_bits(a, P) -> np.ndarray:
    """The uint16 bit patterns of split_planes(a, P), uint16[P, ...]."""
    return np.stack([bf16_bits(pl) for pl in split_planes(a, P)])


def kept_pairs(P):
    """(activation plane i, weight plane j) of the products the kernel keeps: i + j < P, in its summation order."""
    return [(0, 0), (0, 1), (1, 0)] if P == 2 else [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]


def split_conv_ref(x, W, nbr, n_out, P, bias=None, acc=None, pairs=None):
    """-> (y float64[n_out, cout], mag float64[n_out, cout]):
    y[o] = sum_k sum_{(i, j) in pairs} x_i[nbr[k][o]] @ W_j[k] (+ bias) (+ acc), mag = sum |x||w| (+ |bias|) (+ |acc|) of
    the unsplit operands.  pairs: kept_pairs(P) unless given.  nbr int[K, n_out] (-1: no neighbour) or None (identity)."""
    xp = split_planes(x, P).astype(np.float64)
    Wp = split_planes(W, P).astype(np.float64)
    pairs = kept_pairs(P) if pairs is None else pairs
    K, cin, cout = W.shape
    y = np.zeros((n_out, cout), np.float64)
    mag = np.zeros((n_out, cout), np.float64)
    xa, Wa = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64))
    for k in range(K):
        rows = np.arange(n_out) if nbr is None else np.asarray(nbr[k], np.int64)
        m = rows >= 0
        if not m.any():
            continue
        for i in sorted({i for i, _ in pairs}):
            Wsum = sum(Wp[j][k] for ii, j in pairs if ii == i)          # exact in float64: parts of one f32 value
            y[m] += xp[i][rows[m]] @ Wsum
        mag[m] += xa[rows[m]] @ Wa[k]
    if bias is not None:
        y += np.asarray(bias, np.float64)
        mag += np.abs(np.asarray(bias, np.float64))
    if acc is not None:
        y += np.asarray(acc, np.float64)
        mag += np.abs(np.asarray(acc, np.float64))
    return y, mag


def split_conv_vjp_ref(dy, W, nbr, n_in, P):
    """The float64 vector-Jacobian product of split_conv_ref with respect to its input, with dy and W as planes:
    dx[nbr[k][o]] += sum_{(i, j) kept} dy_i[o] @ W_j[k]^T;  -> (dx float64[n_in, cin], mag = the same with |dy|, |W|)."""
    dp = split_planes(dy, P).astype(np.float64)
    Wp = split_planes(W, P).astype(np.float64)
    K, cin, cout = W.shape
    dx = np.zeros((n_in, cin), np.float64)
    mag = np.zeros((n_in, cin), np.float64)
    da, Wa = np.abs(np.asarray(dy, np.float64)), np.abs(np.asarray(W, np.float64))
    for k in range(K):
        rows = np.arange(dy.shape[0]) if nbr is None else np.asarray(nbr[k], np.int64)
        m = rows >= 0
        if not m.any():
            continue
        g = np.zeros((int(m.sum()), cin), np.float64)
        for i in range(P):
            Wsum = sum(Wp[j][k] for ii, j in kept_pairs(P) if ii == i)
            g += dp[i][m] @ Wsum.T
        np.add.at(dx, rows[m], g)
        np.add.at(mag, rows[m], da[m] @ Wa[k].T)
    return dx, mag
