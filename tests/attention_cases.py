"""Cases, float64 references and comparators for the decoder's attention kernels (csrc/attention.hip: usc_attn_fwd /
usc_attn_bwd with their mask pack, combine and dq reduce passes, usc_self_attn_fwd / usc_self_attn_bwd), shared by
tests/test_attention_cases_host.py (CPU: the table holds every size the kernels and the split planner branch on, the
recipes are what they claim, the comparators accept an f32 evaluation in the kernels' partition and reject planted
errors) and tests/test_gpu_attention_f64.py (every entry point, element-wise).  Nothing here touches a device at import
time and the references call nothing from the library: plain torch in float64, on whatever device the inputs are on.

Inputs, per (batch, head) (bh = b H + h, seed = the case's):
  k[..., 0] = 4 (a handle for a common offset), k[..., 1] = 8 (2 j / (S - 1) - 1) (a ramp over the key index, 0 at
  S = 1), k[..., 2:] standard normal; v and dO standard normal.  The keys of key_list() (0, 31, 32, S - 1, the first key
  of the last non-empty split, the last key of split 0) have |k[2:]| = SELECT_NORM.
  Query row i takes score recipe (i + seed + bh) % 7:
    0 normal      q[0:2] = 0, rest randn                      today's regime
    1 sharp       as 0, times 8                               peaked softmax, large alpha steps
    2 flat        0                                           uniform p = 1 / n
    3 selector    k[pi] SELECT_SCORE * 4 / |k[pi, 2:]|^2, q[0:2] = 0: key pi scores SELECT_SCORE = 35, every other
                  key N(0, (35 / 9)^2) (10 k[pi] on keys of standard norm would leave the largest of 3 200 other scores
                  above the selected one); pi cycles over key_list()
    4 offset +    as 0, q[0] = +50                            every score ~ +50
    5 offset -    as 0, q[0] = -50                            every score ~ -50
    6 ramp        q[1] = +20 | -20 alternating, q[0] = 0, rest RAMP_NOISE randn: the running maximum rises in every
                  chunk and split, or is set by the first chunk
  Cross attention: query row i of batch b also takes mask recipe (3 i + seed + b) % 7:
    0 all keys open | 1 random half | 2 exactly one key open (cycling over key_list()) | 3 the first chunk (keys 0..31)
    masked | 4 one whole non-empty key split masked (the split index cycles) | 5 everything masked | 6 random 90 % masked
  Recipes 3 and 4 need keys outside what they mask (S > 32, two used splits); where there are none the row takes recipe
  1, and `mrec` records that.  Key 5, where it exists, is masked for every query.  The mask is bool[B, S, L], True =
  masked, shared by the heads, as ops.masked_cross_attention takes it.

References (f64 from the f32 inputs; self attention: the same without a mask):
  forward   s = (q / 4) k^T, masked entries -inf; lse = logsumexp(s), p = exp(s - lse), o = p v.  A row with every key
            masked is p = 0, o = +0.0, lse = +inf (what the kernels return; softmax alone would give NaN).
  backward  inputs q, k, v, mask, dO and the F32 o and lse as a forward saved them: D = sum_d dO o, p = exp(s - lse),
            dp = dO v^T, ds = p (dp - D), dq = ds k / 4, dk = ds^T q / 4, dv = p^T dO.
Magnitudes, every factor by its absolute value: mag_s[i, j] = sum_d |q_id| |k_jd| / 4; the conditioning of a row is
amp_i = 1 + max_{j open} mag_s[i, j] + |lse_i| (1 for a fully masked row): an f32 score carries an absolute error of about
2^-24 mag_s, the fast exponential a relative one of about 2^-24 |x| from rounding its argument, and both pass straight
into p.
  lse  amp_i                                 o   amp_i sum_j p_ij |v_jd|
  dv   sum_i amp_i p_ij |dO_id|              dq  sum_j amp_i mds_ij |k_jd| / 4      dk  sum_i amp_i mds_ij |q_id| / 4
  with mds_ij = p_ij (sum_d |dO_id| |v_jd| + sum_d |dO_id| |o_id|)
Bound: |y - ref| <= BOUND mag + 1e-30 per element, BOUND = conv_cases.BOUND = 2**-20; where mag is 0 (o and dq of a
fully masked row, dk and dv of a key masked for every query) the kernel must give exactly 0; where lse is +inf the
kernel must give +inf.

Count mode (the forward's counterpart of the integer mode of the other suites): q = 0, v integers in [-3, 3], a mask
under which every query's number of open keys n is a power of two from 1 up to the largest that fits S.  Every
exponential is exp(0) = 1, l = n exactly and every partial sum of v is an integer, so |o - (sum_open v) / n| <=
2**-22 |ref| (one rounding for a reciprocal, one for its product), o = 0 exactly where the sum is 0, lse = log n within
the bound above.  One dropped, doubled or misplaced key or one wrong mask bit moves the sum by at least 1 / n >= 2**-12.

The split planner, restated (planned()): about 1024 waves, at most one split per chunk of 32 keys, at most 64;
keys_per_split = ceil(S / nsplit) rounded up to 32; the trailing splits that start at or behind S are empty, and their
partials are written all the same (zeros and m = -inf) because the combine and dq-reduce kernels read them.
"""
import functools
import math
import zlib
from dataclasses import dataclass

import torch

from conv_cases import BOUND, EXACT_LIMIT, PATTERN, WS_BYTE, GuardedF32, GuardedWs, accepts, bounded_ratios  # noqa: F401
from rows_cases import _gen, same_bits, to_device  # noqa: F401

HD = 16
CHUNK = 32
N_RECIPES = 7
SCORE = ("normal", "sharp", "flat", "selector", "offset+", "offset-", "ramp")
MASK = ("open", "half", "one key", "first chunk", "split", "all", "ninety")
SELECT_NORM = 9.0
SELECT_SCORE = 35.0
RAMP_NOISE = 0.05
COUNT_BOUND = 2.0 ** -22
CROSS_L = (1, 31, 32, 33, 100, 128, 129, 150, 160, 161, 255, 256)
CROSS_S = (1, 3, 31, 32, 33, 77, 200, 999, 1024, 1100, 2100)
SELF_L = (1, 2, 31, 32, 33, 64, 100, 128, 129, 160, 161, 255, 256)


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- the planner
def planned(S, B, H):
    """(nsplit, keys_per_split, empty trailing splits) of usc_attn_fwd / usc_attn_bwd."""
    bh = B * H
    nsplit = max(1, min(-(-1024 // (4 * bh)), -(-S // CHUNK), 64))
    kps = -(-(-(-S // nsplit)) // CHUNK) * CHUNK
    return nsplit, kps, nsplit - -(-S // kps)


def plan_string(nsplit, kps, empty):
    return f"{nsplit}x{kps} empty {empty}"


def lse_stride(L):
    return 128 if L <= 128 else 256


def ws_layout(L, S, B, H, nsplit):
    """The documented workspace: packed mask bits, the partials (o or dq), (m, l), 256 spare bytes."""
    LP = lse_stride(L)
    bits = -(-(B * S * (LP // 32) * 4) // 256) * 256
    return bits, B * H * nsplit * 4 * LP * HD * 4, B * H * nsplit * 2 * LP * 4, 256


def nsplit_from_ws_bytes(nbytes, L, S, B, H):
    bits, part, ml, spare = ws_layout(L, S, B, H, 1)
    n, rest = divmod(nbytes - bits - spare, part + ml)
    return n if rest == 0 else None


# ------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class CrossCase:
    L: int
    S: int
    B: int
    H: int
    plan: str                   # nsplit x keys_per_split, empty trailing splits: what the library must plan
    why: str
    repeat: bool = False

    @property
    def name(self):
        return f"l{self.L}-s{self.S}-b{self.B}-h{self.H}"

    @property
    def E(self):
        return HD * self.H

    @property
    def seed(self):
        return _seed("cross", self.name)

    @property
    def masked(self):
        return True


@dataclass(frozen=True)
class SelfCase:
    L: int
    B: int
    H: int
    repeat: bool = False

    @property
    def name(self):
        return f"l{self.L}-b{self.B}-h{self.H}"

    @property
    def S(self):
        return self.L

    @property
    def E(self):
        return HD * self.H

    @property
    def seed(self):
        return _seed("self", self.name)

    @property
    def masked(self):
        return False

    @property
    def count_mode(self):
        return self.L & (self.L - 1) == 0


PLANNER_ROWS = ((100, 1100, 1, 8), (100, 1024, 1, 8), (150, 999, 2, 8), (161, 77, 3, 8), (5, 200, 33, 8), (33, 2100, 1, 1),
                (129, 2100, 1, 1), (37, 33, 1, 3), (1, 1, 1, 8), (256, 3200, 1, 8))

_CROSS = (
    (100, 1100, 1, 8, "32x64 empty 14", "32 splits of 64 keys, 18 used, the last with 12 keys, 14 empty"),
    (100, 1024, 1, 8, "32x32 empty 0", "32 full splits of one chunk"),
    (150, 999, 2, 8, "16x64 empty 0", "16 splits, ragged tail, two batches, NG = 2"),
    (161, 77, 3, 8, "3x32 empty 0", "fewer chunks than wanted splits; a sixth query tile with one row"),
    (5, 200, 33, 8, "1x224 empty 0", "264 heads: one split of 224 keys"),
    (33, 2100, 1, 1, "64x64 empty 31", "the 64-split cap, 33 used, 31 empty"),
    (129, 2100, 1, 1, "64x64 empty 31", "the same under NG = 2"),
    (37, 33, 1, 3, "2x32 empty 0", "H = 3, one chunk plus one key"),
    (1, 1, 1, 8, "1x32 empty 0", "one key: p = 1, dq = dk = 0"),
    (256, 3200, 1, 8, "32x128 empty 7", "the widest case, the only one above 2 100 keys; four chunks per split"),
    (1, 3, 2, 8, "1x32 empty 0", "one query, three keys, two batches"),
    (31, 31, 1, 8, "1x32 empty 0", "one short query tile, one short chunk"),
    (32, 32, 2, 3, "1x32 empty 0", "exactly one tile and one chunk, H = 3"),
    (33, 33, 1, 8, "2x32 empty 0", "one row into the second tile, one key into the second split"),
    (100, 1, 1, 8, "1x32 empty 0", "the training query count on a single key"),
    (128, 77, 1, 8, "3x32 empty 0", "the last query count of NG = 1"),
    (129, 31, 1, 8, "1x32 empty 0", "the first query count of NG = 2, one short chunk"),
    (150, 200, 1, 8, "7x32 empty 0", "the export query count; seven one-chunk splits, the last with 8 keys"),
    (160, 32, 1, 3, "1x32 empty 0", "five full query tiles, H = 3"),
    (161, 999, 1, 8, "32x32 empty 0", "32 one-chunk splits, the last with 7 keys"),
    (255, 1024, 1, 8, "32x32 empty 0", "one row short of the width limit"),
    (256, 1100, 1, 1, "35x32 empty 0", "one head: a split per chunk, below the cap"),
    (128, 2100, 1, 8, "32x96 empty 10", "three chunks per split, 22 used, the last with 84 keys, 10 empty"),
    (31, 3, 1, 1, "1x32 empty 0", "H = 1, three keys"),
    (32, 1024, 2, 8, "16x64 empty 0", "16 heads: two full chunks per split"),
    (33, 1100, 3, 8, "11x128 empty 2", "24 heads: 11 splits of four chunks, 9 used, 2 empty"),
    (100, 200, 2, 8, "7x32 empty 0", "the decoder's coarsest level at batch 2"),
    (129, 77, 2, 3, "3x32 empty 0", "NG = 2 with H = 3 and two batches"),
    (255, 33, 1, 8, "2x32 empty 0", "NG = 2, a second split of one key"),
    (256, 1, 1, 8, "1x32 empty 0", "the width limit on a single key"),
    (160, 2100, 1, 3, "64x64 empty 31", "the cap from B H = 3, NG = 2"),
    (1, 999, 1, 8, "32x32 empty 0", "one query over 32 splits"),
    (7, 32, 1, 8, "1x32 empty 0", "one row of each recipe on one full chunk"),
    (100, 999, 4, 8, "8x128 empty 0", "32 heads: 8 splits of four chunks, a last split of 103 keys"),
    (128, 200, 1, 1, "7x32 empty 0", "H = 1 at four full query tiles"),
    (150, 1100, 1, 3, "35x32 empty 0", "H = 3 under NG = 2, a split per chunk"),
    (161, 3, 1, 8, "1x32 empty 0", "NG = 2 on three keys"),
    (31, 2100, 2, 8, "16x160 empty 2", "five chunks per split, 14 used, the last with 20 keys, 2 empty"),
    (33, 200, 32, 8, "1x224 empty 0", "256 heads: the first head count with one split"),
    (5, 77, 85, 3, "2x64 empty 0", "255 heads: the last head count with two splits"),
)
CROSS_CASES = [CrossCase(*row, repeat=i % 4 == 0) for i, row in enumerate(_CROSS)]

_SELF = ((1, 1, 8), (2, 2, 3), (31, 1, 8), (32, 3, 1), (33, 1, 8), (64, 2, 8), (100, 1, 8), (100, 3, 3), (128, 1, 8),
         (128, 2, 1), (129, 1, 8), (129, 2, 3), (160, 1, 8), (161, 3, 1), (161, 1, 8), (255, 1, 8), (255, 2, 3), (256, 1, 8),
         (256, 3, 1), (256, 2, 8))
SELF_CASES = [SelfCase(*row, repeat=i % 3 == 0) for i, row in enumerate(_SELF)]


def case_plan(c):
    """(nsplit, keys_per_split, empty) the kernels run a case with; self attention is one launch over all keys."""
    return planned(c.S, c.B, c.H) if c.masked else (1, -(-c.S // CHUNK) * CHUNK, 0)


def key_list(S, nsplit, kps):
    """The keys the selector rows and the one-key masks cycle over (key 5 is masked for every query: never one)."""
    used = -(-S // kps)
    out = []
    for j in (0, 31, 32, S - 1, (used - 1) * kps, min(kps, S) - 1):
        if 0 <= j < S and j not in out and j != 5:
            out.append(j)
    return out


# ------------------------------------------------------------------------------------------------- inputs
def heads(t, H):
    """[len, B, H * 16] -> [B, H, len, 16] (a view)."""
    n, B, E = t.shape
    return t.view(n, B, H, HD).permute(1, 2, 0, 3)


def unheads(t):
    """[B, H, len, 16] -> [len, B, H * 16], contiguous."""
    B, H, n, d = t.shape
    return t.permute(2, 0, 1, 3).reshape(n, B, H * d).contiguous()


def _mask(c, g, keys, nsplit, kps):
    L, S, B = c.L, c.S, c.B
    used = -(-S // kps)
    mask = torch.zeros((B, S, L), dtype=torch.bool)
    mrec = torch.zeros((B, L), dtype=torch.int64)
    for b in range(B):
        for i in range(L):
            r = (3 * i + c.seed + b) % N_RECIPES
            if (r == 3 and S <= CHUNK) or (r == 4 and used < 2):
                r = 1
            col = torch.zeros(S, dtype=torch.bool)
            if r == 1:
                col = torch.rand(S, generator=g) < 0.5
            elif r == 2:
                col[:] = True
                col[keys[(i // N_RECIPES + b) % len(keys)]] = False
            elif r == 3:
                col[:CHUNK] = True
            elif r == 4:
                sp = (i // N_RECIPES + b) % used
                col[sp * kps:(sp + 1) * kps] = True
            elif r == 5:
                col[:] = True
            elif r == 6:
                col = torch.rand(S, generator=g) < 0.9
            mask[b, :, i] = col
            mrec[b, i] = r
    if S > 5:
        mask[:, 5, :] = True
    return mask, mrec


@functools.lru_cache(maxsize=None)
def attn_inputs(c):
    """CPU tensors of a case (shared, never written to): q, dO [L, B, E], k, v [S, B, E] in f32, mask bool[B, S, L] (None for
    self attention), srec [B, H, L] / mrec [B, L] the recipes realised, pi [B, H, L] the selector key of every row."""
    L, S, B, H = c.L, c.S, c.B, c.H
    g = _gen(c.seed)
    nsplit, kps, _ = case_plan(c)
    keys = key_list(S, nsplit, kps)
    k = torch.randn((B, H, S, HD), generator=g, dtype=torch.float64)
    k[..., 0] = 4.0
    k[..., 1] = 8.0 * (2.0 * torch.arange(S, dtype=torch.float64) / (S - 1) - 1.0) if S > 1 else 0.0
    for j in keys:
        k[:, :, j, 2:] *= SELECT_NORM / k[:, :, j, 2:].norm(dim=-1, keepdim=True)
    v = torch.randn((B, H, S, HD), generator=g, dtype=torch.float64)
    dO = torch.randn((B, H, L, HD), generator=g, dtype=torch.float64)
    z = torch.randn((B, H, L, HD), generator=g, dtype=torch.float64)
    i = torch.arange(L)
    bh = torch.arange(B * H).view(B, H, 1)
    srec = (i + c.seed + bh) % N_RECIPES
    pi = torch.tensor(keys)[(i // N_RECIPES + bh) % len(keys)]
    base = z.clone()
    base[..., :2] = 0.0
    ksel = torch.gather(k, 2, pi[..., None].expand(B, H, L, HD)).clone()
    ksel[..., :2] = 0.0
    sel = ksel * (4.0 * SELECT_SCORE / SELECT_NORM ** 2)
    plus, minus, ramp = base.clone(), base.clone(), RAMP_NOISE * base
    plus[..., 0], minus[..., 0] = 50.0, -50.0
    ramp[..., 1] = torch.where((i // N_RECIPES) % 2 == 0, 20.0, -20.0).double()
    q = torch.zeros_like(z)
    for r, t in enumerate((base, 8.0 * base, torch.zeros_like(z), sel, plus, minus, ramp)):
        q = torch.where((srec == r)[..., None], t, q)
    out = dict(q=unheads(q).float(), k=unheads(k).float(), v=unheads(v).float(), dO=unheads(dO).float(), mask=None,
               srec=srec, mrec=None, pi=pi)
    if c.masked:
        out["mask"], out["mrec"] = _mask(c, g, keys, nsplit, kps)
    return out


@functools.lru_cache(maxsize=None)
def count_inputs(c):
    """Count mode: q = 0, v integers in [-3, 3], every query with a power-of-two number of open keys (self attention: all
    L keys, so only where L is a power of two)."""
    L, S, B, H = c.L, c.S, c.B, c.H
    g = _gen(c.seed + 1)
    t = dict(attn_inputs(c))
    t["q"] = torch.zeros_like(t["q"])
    t["v"] = torch.randint(-3, 4, (S, B, c.E), generator=g).float()
    if c.masked:
        steps = int(math.log2(S)) + 1
        mask = torch.ones((B, S, L), dtype=torch.bool)
        for b in range(B):
            for i in range(L):
                mask[b, torch.randperm(S, generator=g)[:2 ** ((i + b) % steps)], i] = False
        t["mask"] = mask
    return t


def realised_pairs(c):
    """The (score recipe, mask recipe) pairs of a cross case, as names."""
    t = attn_inputs(c)
    pairs = t["srec"] * N_RECIPES + t["mrec"][:, None, :]
    return {(SCORE[int(p) // N_RECIPES], MASK[int(p) % N_RECIPES]) for p in pairs.unique()}


# ------------------------------------------------------------------------------------------------- references
def _masked(mask, B, L, S, device):
    """bool [B, 1, L, S]: True = masked."""
    if mask is None:
        return torch.zeros((B, 1, L, S), dtype=torch.bool, device=device)
    return mask.permute(0, 2, 1)[:, None]


def _scores(q, k, mask, H):
    qh, kh = heads(q, H).double(), heads(k, H).double()
    masked = _masked(mask, q.shape[1], q.shape[0], k.shape[0], q.device)
    s = ((qh / 4) @ kh.transpose(-1, -2)).masked_fill(masked, float("-inf"))
    mag_s = ((qh.abs() / 4) @ kh.abs().transpose(-1, -2)).masked_fill(masked, 0.0)
    return s, mag_s, qh, kh


def _amp(mag_s, lse):
    """[B, H, L]: 1 + the largest open mag_s + |lse|; 1 for a fully masked row (lse = +inf)."""
    dead = torch.isinf(lse)
    return torch.where(dead, torch.ones_like(lse), 1.0 + mag_s.amax(-1) + torch.where(dead, torch.zeros_like(lse), lse).abs())


def ref_forward(q, k, v, mask, H):
    """dict(o, o_mag [B, H, L, 16], lse, amp [B, H, L], p [B, H, L, S]) in f64."""
    s, mag_s, _, _ = _scores(q, k, mask, H)
    vh = heads(v, H).double()
    lse = torch.logsumexp(s, -1)
    lse = torch.where(torch.isinf(lse) & (lse < 0), torch.full_like(lse, float("inf")), lse)
    p = torch.exp(s - lse[..., None])
    amp = _amp(mag_s, lse)
    return dict(o=p @ vh, o_mag=amp[..., None] * (p @ vh.abs()), lse=lse, amp=amp, p=p)


def saved_forward(fw, stride):
    """The f32 o [L, B, E] and lse [B * H, stride] a forward would have saved for this reference (columns L .. stride - 1
    hold NaN: the backward must not look at them)."""
    B, H, L = fw["lse"].shape
    lse = torch.full((B * H, stride), float("nan"), dtype=torch.float32, device=fw["lse"].device)
    lse[:, :L] = fw["lse"].reshape(B * H, L).float()
    return unheads(fw["o"]).float(), lse


def ref_backward(q, k, v, mask, dO, o32, lse32, H):
    """name -> (ref, mag) for dq, dk, dv in head layout [B, H, len, 16]; o32 [L, B, E] and lse32 [B * H, >= L] in f32."""
    L, B = q.shape[0], q.shape[1]
    s, mag_s, qh, kh = _scores(q, k, mask, H)
    vh, dOh, oh = heads(v, H).double(), heads(dO, H).double(), heads(o32, H).double()
    lse = lse32[:, :L].reshape(B, H, L).double()
    amp = _amp(mag_s, lse)[..., None]
    p = torch.exp(s - lse[..., None])
    D = (dOh * oh).sum(-1, keepdim=True)
    ds = p * (dOh @ vh.transpose(-1, -2) - D)
    mds = amp * p * (dOh.abs() @ vh.abs().transpose(-1, -2) + (dOh.abs() * oh.abs()).sum(-1, keepdim=True))
    ap = amp * p
    return dict(dq=(ds @ kh / 4, mds @ kh.abs() / 4),
                dk=(ds.transpose(-1, -2) @ qh / 4, mds.transpose(-1, -2) @ qh.abs() / 4),
                dv=(p.transpose(-1, -2) @ dOh, ap.transpose(-1, -2) @ dOh.abs()))


def ref_count(v, mask, H, L):
    """Count mode: (sums [B, H, L, 16] the integer sum of v over the open keys, n [B, 1, L, 1] their number) in f64."""
    vh = heads(v, H).double()
    B, _, S, _ = vh.shape
    opened = (~_masked(mask, B, L, S, v.device)).double()
    return opened @ vh, opened.sum(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------- comparators
def fraction(y, ref, mag):
    """The largest |y - ref| / (BOUND mag + 1e-30); inf where ref is +inf and y is not, and where mag is 0 and y is not."""
    if y.numel() == 0:
        return 0.0
    y, ref, mag = y.double(), ref.double().expand(y.shape), mag.double().expand(y.shape)
    nan = torch.full_like(y, float("nan"))
    same_inf = torch.isinf(ref) & (y == ref)
    y = torch.where(same_inf, torch.zeros_like(y), y)
    ref0 = torch.where(torch.isinf(ref), torch.zeros_like(ref), ref)
    y = torch.where((mag == 0) & (y != ref0), nan, y)
    mag = torch.where(torch.isfinite(mag), mag, torch.ones_like(mag))
    return bounded_ratios(y, ref0, mag)[0]


def forward_fractions(o, lse, fw):
    """o [L, B, E] and lse [B * H, >= L] of a kernel against ref_forward()."""
    B, H, L = fw["lse"].shape
    return dict(o=fraction(heads(o, H), fw["o"], fw["o_mag"]), lse=fraction(lse[:, :L].reshape(B, H, L), fw["lse"], fw["amp"]))


def backward_fractions(dq, dk, dv, refs):
    H = refs["dq"][0].shape[1]
    return {n: fraction(heads(t, H), *refs[n]) for n, t in (("dq", dq), ("dk", dk), ("dv", dv))}


def dead_rows_exact(o, lse, fw):
    """Fully masked rows hold o = +0.0 and lse = +inf bit for bit."""
    B, H, L = fw["lse"].shape
    dead = torch.isinf(fw["lse"])
    oh, ls = heads(o, H)[dead], lse[:, :L].reshape(B, H, L)[dead]
    return same_bits(oh, torch.zeros_like(oh)) and same_bits(ls, torch.full_like(ls, float("inf")))


def count_fractions(o, lse, sums, n):
    """Count mode: o against sums / n within COUNT_BOUND |ref| (exactly 0 where the sum is 0), lse against log n."""
    B, H, L, _ = sums.shape
    ref = sums / n
    oh = heads(o, H).double()
    err = (oh - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    fr_o = torch.where(sums == 0, torch.where(oh == 0, 0.0, float("inf")), err / (COUNT_BOUND * ref.abs() + 1e-300))
    logn = torch.log(n[..., 0]).expand(B, H, L)
    return dict(o=float(fr_o.max()), lse=fraction(lse[:, :L].reshape(B, H, L), logn, 1.0 + logn))


def largest_count_sum(v, mask, H, L):
    """An upper limit of every partial sum of count mode: the sum of |v| over the open keys."""
    return float(ref_count(v.abs(), mask, H, L)[0].max())
