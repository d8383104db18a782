"""Cases, float64 reference and comparators for the f32 sparse convolutions (csrc/spconv.hip, csrc/spconv_sorted.hip),
shared by tests/test_conv_cases_host.py (CPU: every case is what it claims to be, the comparators catch planted errors)
and tests/test_gpu_conv_f64.py (every kernel variant, element-wise).  Nothing here touches a device at import time and
the reference calls nothing from the library: index_select, matmul and index_add_ in float64, on whatever device its
inputs are on.

Reference (all float64, `mag` = sum of the absolute values of every term of an element):
  forward    out[o] = sum_k x[nbr[k, o]] @ W[k] (+ bias) (+ out_before), nbr -1 = no term, nbr None = identity rows
             w_transposed: W is [K, cout, cin] and W'[k][c][n] = W[K-1-k][n][c] (K = 1: W[0][n][c])
  pairs      out[rows_out[p]] = x[rows_in[p]] @ W[k(p)]
  wgrad      dW[k] = sum_{p in list k} a[a_idx[p]]^T b[b_idx[p]] (+ dW_before); identity form K = 1 without lists;
             the stem's table form takes the lists of its neighbour table

Inputs are built directly (not from geometry): a neighbour table is -1 with probability 1 - d and uniform in [0, n_in)
otherwise, optionally with a block of rows without any neighbour and a block of rows that all read input row 0; pair
lists come from a table or from explicit per-offset counts.

Two comparators, both over every output element:
  exact      activations are integers in [-3, 3], weights / bias / pre-existing output integers in [-2, 2], and the
             reference asserts mag.max() < 2**24.  Every partial sum in every order is then an integer below 2**24,
             exactly representable in f32 (the matrix-core instruction is a chain of fmaf), so the kernel must equal the
             reference whatever its tile shape, split count or reduction order: one dropped, doubled or misplaced pair
             changes an integer.
  bounded    standard-normal activations, weights scaled by 1 / sqrt(K * cin); |y - ref| <= 2**-20 * mag + 1e-30 per
             element, the bound tests/test_gpu_bf16_conv.py uses for f32 accumulation.

Plans are written as strings, decoded from usc_spconv_plan (plan_string) or from a workspace size:
  row-order  al<NB>/G<G> (aligned kernel), un<NB>/G1 (bounds-checked kernel), stem, ct<NB> (tile-compacted)
  pairs      al<NB> / un<NB>
  sorted     s<NB>/G<G>          NB from the output width (sorted_nb), G = usc_spconv_sorted_ws_bytes / slice bytes
  wgrad      full<CT>x<NB>/S<S> (wgrad_full_kernel<CT, NB>), wg<NB>a/S<S>, wg<NB>u/S<S> (wgrad_kernel<NB, ALIGNED>),
             S = usc_spconv_wgrad_ws_bytes_rows / bytes of dW
"""
import zlib
from dataclasses import dataclass

import numpy as np
import torch

BOUND = 2.0 ** -20
EXACT_LIMIT = 2.0 ** 24
GUARD_ROWS = 64
WS_GUARD = 4096
PATTERN = 0x7FC5A5A5                       # a quiet NaN: a kernel that reads a guard cannot produce a finite result
WS_BYTE = 0xA5
MODES = ("exact", "bounded")


@dataclass(frozen=True)
class Case:
    family: str
    name: str
    plan: str
    cin: int
    cout: int
    K: int
    n: int                      # output rows (forward), rows of a / b (wgrad identity form), rows of dy (stem table form)
    n_in: int = 0               # 0: the same as n
    d: float = 0.5              # density of the neighbour table
    table: bool = True          # False: K = 1 identity rows (no table / no pair lists)
    wt: bool = False            # w_transposed
    bias: bool = False
    acc: bool = False           # accumulate into pre-existing output
    empty: int = 0              # a block of this many consecutive rows without any neighbour
    row0: int = 0               # a block of this many rows whose neighbours are all input row 0
    counts: tuple = ()          # per-offset pair counts (pairs form, wgrad list form)
    capacity: int = 0           # capacity of the pair lists (0: exactly the pairs)
    shift: bool = False         # dW starts one float into its buffer (4-byte aligned only)
    background: bool = False    # also run with usc_spconv_wgrad_grid_limit(8): same bits
    repeat: bool = False        # a second launch must give identical bits
    slices: bool = False        # sorted: also the slices_left form of usc_spconv_sorted_gemm_ex
    tm: int = 0                 # tile-compacted kernel: tile height the planner chooses (compact_tm)
    mirror: int = 0             # usc_weight_transpose

    @property
    def rows_in(self):
        return self.n_in or self.n

    @property
    def seed(self):
        return zlib.crc32(f"{self.family}/{self.name}".encode()) & 0x7FFFFFFF

    @property
    def id(self):
        return self.name


# ------------------------------------------------------------------------------------------------- plans
def plan_string(kind, code):
    """usc_spconv_plan's code as the plan string of the module docstring (without the S of a weight gradient)."""
    nb, aligned, compact, full, stem, hi = code & 0xFF, (code >> 8) & 1, (code >> 12) & 1, (code >> 13) & 1, \
        (code >> 14) & 1, code >> 16
    if kind == 2:
        return f"full{hi}x{nb}" if full else f"wg{nb}{'a' if aligned else 'u'}"
    if stem:
        return "stem"
    if compact:
        return f"ct{nb}"
    base = f"{'al' if aligned else 'un'}{nb}"
    return base if kind == 1 else f"{base}/G{hi}"


def variant(plan):
    """The kernel instantiation of a plan string: without the split counts."""
    return plan.split("/")[0]


def sorted_nb(cout):
    cb = cout // 32
    return 4 if cb % 4 == 0 else 3 if cb % 3 == 0 else 2 if cb % 2 == 0 else 1


def compact_tm(n_out, nb):
    """Tile height of the tile-compacted kernel (plan_table in csrc/spconv.hip): whole rounds of 256 tiles, at most 256
    rows (192 for three column blocks), rounded up to a multiple of 4.  The library does not report it; the cases carry
    it to say which step of the rule they sit on."""
    tm_max = 192 if nb == 3 else 256
    rounds = 1
    while -(-n_out // (256 * rounds)) > tm_max:
        rounds += 1
    return (-(-n_out // (256 * rounds)) + 3) & ~3


def decoded_plan(lib, c):
    """The plan the library chooses for a case, as a plan string (host-only entry points)."""
    if c.family in ("row", "stem", "compact"):
        # usc_spconv_plan takes K = 1 for identity rows: a K = 1 TABLE with <= 4 input and 32 output channels runs the
        # stem kernel all the same (usc_spconv_gather_gemm tests the table pointer), so those cases are written "stem".
        if c.family == "stem" and c.K == 1:
            return "stem"
        return plan_string(0, lib.usc_spconv_plan(0, c.n, c.cin, c.cout, c.K))
    if c.family == "pairs":
        return plan_string(1, lib.usc_spconv_plan(1, c.capacity or sum(c.counts), c.cin, c.cout, c.K))
    if c.family == "sorted":
        ws = lib.usc_spconv_sorted_ws_bytes(c.n, c.cin, c.cout, c.K)
        return f"s{sorted_nb(c.cout)}/G{max(1, ws // (c.n * c.cout * 4))}"
    if c.family in ("wgrad", "group"):
        rows = wgrad_capacity(c)
        s = lib.usc_spconv_wgrad_ws_bytes_rows(c.K, c.cin, c.cout, rows) // (c.K * c.cin * c.cout * 4)
        if c.family == "group":
            s = 1                                                          # the grouped form never splits
        return f"{plan_string(2, lib.usc_spconv_plan(2, rows, c.cin, c.cout, c.K))}/S{s}"
    if c.family == "stem_wgrad":
        return "stemtable"
    return "transpose"


def wgrad_capacity(c):
    return (c.capacity or sum(c.counts)) if c.table else c.n


# ------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _acts(mode, g, shape):
    return torch.randint(-3, 4, shape, generator=g).float() if mode == "exact" else torch.randn(shape, generator=g)


def _small(mode, g, shape, scale=1.0):
    """Weights, bias and pre-existing output: integers in [-2, 2] (exact) or normal * scale (bounded)."""
    return torch.randint(-2, 3, shape, generator=g).float() if mode == "exact" else torch.randn(shape, generator=g) * scale


def make_table(K, n_in, n_out, d, seed, empty=0, row0=0):
    """int32 [K, n_out]: -1 with probability 1 - d, else uniform in [0, n_in)."""
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, n_in, size=(K, n_out), dtype=np.int32)
    if d < 1.0:
        nbr[rng.random((K, n_out)) >= d] = -1
    if empty:
        start = max(0, min(n_out // 3, n_out - empty))
        nbr[:, start:start + empty] = -1
    if row0:
        start = max(0, min(2 * n_out // 3, n_out - row0))
        nbr[:, start:start + row0] = 0
    return torch.from_numpy(nbr)


def pairs_from_table(nbr):
    """(in rows, out rows, koff) of a table, offset-major, as usc_rulebook_compact lists them."""
    a, b, koff = [], [], [0]
    for k in range(nbr.shape[0]):
        o = torch.nonzero(nbr[k] >= 0).flatten()
        a.append(nbr[k][o].int())
        b.append(o.int())
        koff.append(koff[-1] + o.numel())
    return torch.cat(a), torch.cat(b), torch.tensor(koff, dtype=torch.int64)


def pairs_from_counts(counts, n_a, n_b, seed, capacity=0, unique_b=False):
    """Pair lists with the given per-offset counts; capacity > sum(counts) leaves valid but unused entries at the end.
    unique_b: every b row appears in at most one pair (the pairs form writes every output row once)."""
    rng = np.random.default_rng(seed)
    total = int(sum(counts))
    cap = max(capacity, total)
    a_idx = rng.integers(0, n_a, size=cap, dtype=np.int32)
    if unique_b:
        assert cap <= n_b
        b_idx = rng.permutation(n_b)[:cap].astype(np.int32)
    else:
        b_idx = rng.integers(0, n_b, size=cap, dtype=np.int32)
    koff = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    return torch.from_numpy(a_idx), torch.from_numpy(b_idx), torch.from_numpy(koff)


def forward_inputs(c, mode):
    """CPU tensors of a forward case (families row, stem, compact, sorted): x, W (as the entry point takes it), nbr or
    None, bias or None, before or None."""
    g = _gen(c.seed + (0 if mode == "exact" else 1))
    n_in = c.rows_in
    x = _acts(mode, g, (n_in, c.cin))
    wshape = (c.K, c.cout, c.cin) if c.wt else (c.K, c.cin, c.cout)
    W = _small(mode, g, wshape, (c.K * c.cin) ** -0.5)
    nbr = make_table(c.K, n_in, c.n, c.d, c.seed, c.empty, c.row0) if c.table else None
    bias = _small(mode, g, (c.cout,)) if c.bias else None
    before = _small(mode, g, (c.n, c.cout)) if c.acc else None
    return dict(x=x, W=W, nbr=nbr, bias=bias, before=before)


def pairs_inputs(c, mode):
    g = _gen(c.seed + (0 if mode == "exact" else 1))
    total = sum(c.counts)
    x = _acts(mode, g, (c.rows_in, c.cin))
    W = _small(mode, g, (c.K, c.cin, c.cout), c.cin ** -0.5)
    rows_in, rows_out, koff = pairs_from_counts(c.counts, c.rows_in, c.n, c.seed, c.capacity or total, unique_b=True)
    return dict(x=x, W=W, rows_in=rows_in, rows_out=rows_out, koff=koff)


def wgrad_inputs(c, mode):
    """a [rows, cin], b [rows, cout], pair lists (or None: identity form), dW_before or None."""
    g = _gen(c.seed + (0 if mode == "exact" else 1))
    a = _acts(mode, g, (c.rows_in, c.cin))
    b = _small(mode, g, (c.n, c.cout))
    a_idx = b_idx = koff = None
    if c.table:
        a_idx, b_idx, koff = pairs_from_counts(c.counts, c.rows_in, c.n, c.seed, c.capacity)
    before = _small(mode, g, (c.K, c.cin, c.cout)) if c.acc else None
    return dict(a=a, b=b, a_idx=a_idx, b_idx=b_idx, koff=koff, before=before)


def stem_wgrad_inputs(c, mode):
    g = _gen(c.seed + (0 if mode == "exact" else 1))
    x = _acts(mode, g, (c.rows_in, c.cin))
    dy = _small(mode, g, (c.n, c.cout))
    nbr = make_table(c.K, c.rows_in, c.n, c.d, c.seed)
    before = _small(mode, g, (c.K, c.cin, c.cout)) if c.acc else None
    return dict(x=x, dy=dy, nbr=nbr, before=before)


def to_device(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------- reference
def effective_weights(W, wt):
    """[K, cin, cout] weights a forward call uses: W itself, or W'[k][c][n] = W[K-1-k][n][c] of a [K, cout, cin] W."""
    return W.flip(0).transpose(1, 2) if wt else W


def ref_forward(x, W, nbr, n_out, bias=None, before=None, wt=False, dtype=torch.float64, exact=False):
    """(out, mag) of the forward convolution, accumulated in `dtype`."""
    We = effective_weights(W, wt).to(dtype)
    K, cin, cout = We.shape
    xz = torch.cat([x.to(dtype), torch.zeros((1, cin), dtype=dtype, device=x.device)])      # row n_in: "no neighbour"
    y = torch.zeros((n_out, cout), dtype=dtype, device=x.device)
    mag = torch.zeros_like(y)
    for k in range(K):
        if nbr is None:
            rows = torch.arange(n_out, device=x.device)
        else:
            r = nbr[k].long()
            rows = torch.where(r >= 0, r, torch.full_like(r, x.shape[0]))
        xa = xz.index_select(0, rows)
        y += xa.matmul(We[k])
        mag += xa.abs().matmul(We[k].abs())
    if bias is not None:
        y += bias.to(dtype)
        mag += bias.to(dtype).abs()
    if before is not None:
        y += before.to(dtype)
        mag += before.to(dtype).abs()
    if exact:
        assert float(mag.max()) < EXACT_LIMIT, "not an exact case: a partial sum may leave the integers f32 holds"
    return y, mag


def ref_pairs(x, W, rows_in, rows_out, koff, n_out, dtype=torch.float64, exact=False):
    """(out, mag, written) of the pairs form; rows no pair names stay zero in out and False in written."""
    K, cin, cout = W.shape
    y = torch.zeros((n_out, cout), dtype=dtype, device=x.device)
    mag = torch.zeros_like(y)
    written = torch.zeros(n_out, dtype=torch.bool, device=x.device)
    ko = [int(v) for v in koff.tolist()]
    for k in range(K):
        s, e = ko[k], ko[k + 1]
        if e == s:
            continue
        xa = x.to(dtype).index_select(0, rows_in[s:e].long())
        o = rows_out[s:e].long()
        y.index_add_(0, o, xa.matmul(W[k].to(dtype)))
        mag.index_add_(0, o, xa.abs().matmul(W[k].to(dtype).abs()))
        written[o] = True
    if exact:
        assert float(mag.max()) < EXACT_LIMIT
    return y, mag, written


def ref_wgrad(a, b, K, a_idx=None, b_idx=None, koff=None, before=None, dtype=torch.float64, exact=False):
    """(dW, mag) of the weight gradient; a_idx None = the identity form (K = 1, every row one pair)."""
    cin, cout = a.shape[1], b.shape[1]
    dW = torch.zeros((K, cin, cout), dtype=dtype, device=a.device)
    mag = torch.zeros_like(dW)
    ad, bd = a.to(dtype), b.to(dtype)
    if a_idx is None:
        assert K == 1 and a.shape[0] == b.shape[0]
        dW[0] = ad.t().matmul(bd)
        mag[0] = ad.abs().t().matmul(bd.abs())
    else:
        ko = [int(v) for v in koff.tolist()]
        for k in range(K):
            s, e = ko[k], ko[k + 1]
            if e == s:
                continue
            ar = ad.index_select(0, a_idx[s:e].long())
            br = bd.index_select(0, b_idx[s:e].long())
            dW[k] = ar.t().matmul(br)
            mag[k] = ar.abs().t().matmul(br.abs())
    if before is not None:
        dW += before.to(dtype)
        mag += before.to(dtype).abs()
    if exact:
        assert float(mag.max()) < EXACT_LIMIT
    return dW, mag


def ref_wgrad_table(x, dy, nbr, before=None, dtype=torch.float64, exact=False):
    """The stem's table form: dW[k][c][n] = sum_o x[nbr[k][o]][c] dy[o][n]."""
    a_idx, b_idx, koff = pairs_from_table(nbr.cpu())
    return ref_wgrad(x, dy, nbr.shape[0], a_idx.to(x.device), b_idx.to(x.device), koff, before, dtype, exact)


def ref_transpose(W, mirror):
    """out[k][co][ci] = W[mirror ? K-1-k : k][ci][co], as an indexed copy."""
    K = W.shape[0]
    order = torch.arange(K - 1, -1, -1, device=W.device) if mirror else torch.arange(K, device=W.device)
    return W.index_select(0, order).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------- comparators
def exact_mismatches(y, ref):
    """Number of elements of y (f32) that differ from the float64 reference, NaN included."""
    return int((y.double() != ref.double()).sum())


def bounded_ratios(y, ref, mag):
    """(largest |err| / (BOUND * mag + 1e-30), largest |err| / (2**-24 * mag + 1e-30)) over every element."""
    err = (y.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / (BOUND * mag + 1e-30)).max()), float((err / (2.0 ** -24 * mag + 1e-30)).max())


def accepts(mode, y, ref, mag):
    """Whether the comparator of `mode` accepts y."""
    if y.numel() == 0:
        return True
    return exact_mismatches(y, ref) == 0 if mode == "exact" else bounded_ratios(y, ref, mag)[0] <= 1.0


# ------------------------------------------------------------------------------------------------- guarded buffers
class GuardedF32:
    """f32 [rows, cols] as an interior slice of a larger buffer: at least GUARD_ROWS rows of PATTERN before and after;
    shift = 1 starts the slice one float later (4-byte aligned only).  The interior starts as PATTERN too (rows a kernel
    must not write keep it) unless `init` is given."""

    def __init__(self, rows, cols, device, init=None, shift=0):
        self.g = max(GUARD_ROWS * cols, 1024) + shift
        self.n = rows * cols
        self.buf = torch.full((self.g + self.n + self.g,), PATTERN, dtype=torch.int32, device=device)
        self.raw = self.buf[self.g:self.g + self.n]
        self.t = self.raw.view(torch.float32).view(rows, cols)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.g] == PATTERN).all()) and bool((self.buf[self.g + self.n:] == PATTERN).all())

    def pattern_rows(self):
        """bool [rows]: the rows that still hold PATTERN in every element."""
        return (self.raw.view(self.t.shape) == PATTERN).all(1)


class GuardedWs:
    """A workspace of exactly nbytes with WS_GUARD bytes of WS_BYTE before and after (0 bytes: a NULL pointer)."""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        self.buf = torch.full((WS_GUARD + self.nbytes + WS_GUARD,), WS_BYTE, dtype=torch.uint8, device=device)

    def ptr(self):
        return self.buf.data_ptr() + WS_GUARD if self.nbytes else None

    def interior(self):
        return self.buf[WS_GUARD:WS_GUARD + self.nbytes]

    def guards_intact(self):
        return bool((self.buf[:WS_GUARD] == WS_BYTE).all()) and bool((self.buf[WS_GUARD + self.nbytes:] == WS_BYTE).all())


# ------------------------------------------------------------------------------------------------- case table
def _c(family, name, plan, cin, cout, K, n, **kw):
    return Case(family, name, plan, cin, cout, K, n, **kw)


def _row_cases():
    out = []
    # aligned NB 1: the K offsets split over G groups (G = K on the smallest maps), reduced by group_reduce_kernel
    for n, G in ((1, 27), (33, 27), (129, 27), (700, 27), (2500, 20)):
        out.append(_c("row", f"64x64-K27-n{n}", f"al1/G{G}", 64, 64, 27, n, n_in=max(n // 2, 5), repeat=n == 700))
    out.append(_c("row", "128x128-K8-n24575", "al1/G1", 128, 128, 8, 24575, n_in=9000))
    # aligned NB 2 / 3 / 4: wide outputs on tens of thousands of rows, with a table and on identity rows
    for cout, n, nb in ((320, 19680, 2), (288, 32768, 3), (384, 32768, 4)):
        out.append(_c("row", f"32x{cout}-K8-n{n}", f"al{nb}/G1", 32, cout, 8, n, n_in=5000, d=0.3))
        out.append(_c("row", f"32x{cout}-K1id-n{n}", f"al{nb}/G1", 32, cout, 1, n, table=False))
        out.append(_c("row", f"32x{cout}-K1wt-n{n}", f"al{nb}/G1", 32, cout, 1, n, table=False, wt=True))
    # WT form: K = 1, identity rows, [cout][cin] weights
    for cin, cout in ((64, 96), (96, 128)):
        for n in (129, 700):
            out.append(_c("row", f"{cin}x{cout}-K1wt-n{n}", "al1/G1", cin, cout, 1, n, table=False, wt=True))
    # bounds-checked kernel: NB from the output width, float4 loads when cin % 8 == 0, scalar loads otherwise
    for cin, cout, nb in ((96, 20, 1), (3, 64, 2), (20, 96, 3), (40, 100, 4), (20, 100, 4)):
        for n in (1, 127, 129):
            out.append(_c("row", f"{cin}x{cout}-K27-n{n}", f"un{nb}/G1", cin, cout, 27, n, n_in=77))
    # bias / accumulate: aligned without a split, aligned with the split (bias added by the reduction, cout = 96 is no
    # power of two: the (j * 4) % cout path), bounds-checked
    for bias, acc in ((True, False), (False, True), (True, True)):
        tag = ("b" if bias else "") + ("a" if acc else "")
        out.append(_c("row", f"64x96-K1tab-n700-{tag}", "al1/G1", 64, 96, 1, 700, n_in=300, bias=bias, acc=acc))
        out.append(_c("row", f"64x96-K27-n700-{tag}", "al1/G27", 64, 96, 27, 700, n_in=300, bias=bias, acc=acc))
        out.append(_c("row", f"20x50-K8-n129-{tag}", "un2/G1", 20, 50, 8, 129, n_in=60, bias=bias, acc=acc))
    return out


def _stem_cases():
    out = []
    for cin in (1, 2, 3, 4):
        for K in (1, 8, 27, 32):
            for n in (1, 255, 257):
                for bias in (False, True):
                    out.append(_c("stem", f"{cin}x32-K{K}-n{n}{'-b' if bias else ''}", "stem", cin, 32, K, n, n_in=100,
                                  bias=bias, repeat=(cin, K, n, bias) == (3, 27, 257, True)))
    # accumulate = 1 is not the stem kernel's: the call falls through to the bounds-checked kernel and must still be right
    out.append(_c("stem", "3x32-K27-n257-ba", "stem", 3, 32, 27, 257, n_in=100, bias=True, acc=True))
    out.append(_c("stem", "4x32-K8-n255-a", "stem", 4, 32, 8, 255, n_in=100, acc=True))
    return out


def _compact_cases():
    def c(cin, cout, nb, n, K=27, **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items() if k not in ("repeat",))
        return _c("compact", f"{cin}x{cout}-K{K}-n{n}{tag}", f"ct{nb}", cin, cout, K, n, n_in=max(n // 3, 7),
                  tm=compact_tm(n, nb), **kw)
    return [
        c(64, 32, 1, 24576), c(64, 32, 1, 24577, repeat=True), c(64, 32, 1, 49153),
        c(64, 64, 2, 65536), c(64, 64, 2, 65537),
        c(96, 96, 3, 24577), c(96, 96, 3, 49153),
        c(64, 64, 2, 24577, d=1.0), c(64, 64, 2, 24577, K=8, d=1.0),         # every offset of every tile full
        c(64, 64, 2, 24577, d=0.02, empty=256, row0=300),                      # tiles without any neighbour
        c(96, 96, 3, 24577, wt=True),
        c(64, 32, 1, 24577, bias=True, acc=True),
    ]


def _sorted_cases():
    # a covering selection: every K, every n_out, every cout at least once; both cin; G = 1 and G > 1
    rows = [  # K, n, cin, cout, G, extras
        (2, 1, 32, 32, 2, {}), (2, 33, 32, 64, 2, {"slices": True}), (2, 4096, 96, 128, 2, {}),
        (2, 33, 4096, 32, 2, {"d": 0.7}),
        (8, 31, 32, 96, 8, {}), (8, 257, 32, 128, 8, {"slices": True}), (8, 700, 96, 160, 8, {}),
        (8, 4095, 32, 64, 8, {}), (8, 4096, 96, 32, 8, {}),
        (27, 1, 32, 160, 27, {}), (27, 33, 96, 96, 27, {"slices": True}), (27, 255, 32, 64, 27, {}),
        (27, 700, 96, 128, 27, {"repeat": True, "slices": True}), (27, 4095, 96, 96, 14, {}),
        (27, 4096, 96, 96, 14, {"slices": True}), (27, 4096, 32, 160, 5, {}),
        (32, 1, 32, 32, 32, {}), (32, 31, 96, 64, 32, {}), (32, 257, 32, 96, 32, {"slices": True}),
        (32, 700, 32, 64, 32, {}), (32, 4095, 96, 128, 16, {"d": 0.1}), (32, 4096, 32, 32, 16, {}),
        (27, 700, 96, 96, 27, {"wt": True}), (32, 255, 32, 64, 32, {"wt": True}), (2, 257, 96, 128, 2, {"wt": True}),
        (27, 700, 32, 64, 27, {"bias": True, "acc": True}), (8, 4095, 96, 96, 8, {"bias": True}),
        (27, 700, 32, 64, 27, {"acc": True}),
    ]
    out = []
    for K, n, cin, cout, G, kw in rows:
        tag = "".join(f"-{k}" for k in kw if k not in ("repeat", "slices", "d"))
        out.append(_c("sorted", f"{cin}x{cout}-K{K}-n{n}{tag}", f"s{sorted_nb(cout)}/G{G}", cin, cout, K, n,
                      n_in=max(n // 2, 3), **kw))
    # G = 1: enough row tiles that no split is planned (bias and accumulate applied by the kernel itself)
    out.append(_c("sorted", "32x160-K8-n19680", "s1/G1", 32, 160, 8, 19680, n_in=9000))
    out.append(_c("sorted", "32x160-K8-n19680-bias-acc", "s1/G1", 32, 160, 8, 19680, n_in=9000, bias=True, acc=True))
    out.append(_c("sorted", "32x64-K2-n98305-wt", "s2/G1", 32, 64, 2, 98305, n_in=9000, wt=True))
    return out


_TAILS8 = (0, 1, 31, 32, 33, 0, 64, 5)
_TAILS27 = (0, 3, 33, 1, 0, 16, 31, 17, 2, 8, 9, 40, 1, 1, 7, 15, 64, 0, 0, 5, 32, 33, 6, 12, 1, 20, 0)


def _pairs_cases():
    out = []
    for cin, cout, plan in ((64, 64, "al1"), (32, 96, "al1"), (32, 128, "al1"), (20, 50, "un2")):
        out.append(_c("pairs", f"{cin}x{cout}-K8", plan, cin, cout, 8, sum(_TAILS8) + 37, n_in=50, counts=_TAILS8,
                      repeat=cin == 64))
    out.append(_c("pairs", "64x64-K27-empty-ends", "al1", 64, 64, 27, sum(_TAILS27) + 80, n_in=50, counts=_TAILS27,
                  capacity=sum(_TAILS27) + 40))
    # wide tiles of the list form need >= 3 072 tiles of 32 pairs
    big = (14100, 14101, 0, 14131, 14089, 14100, 14079, 14100)
    for cout, nb in ((64, 2), (96, 3), (128, 4)):
        out.append(_c("pairs", f"32x{cout}-K8-98k", f"al{nb}", 32, cout, 8, sum(big) + 37, n_in=4000, counts=big))
    return out


_WG8 = (0, 1, 7, 8, 9, 15, 16, 17)
_WG8_LONG = (0, 1, 4095, 3000, 9, 2047, 3119, 17)            # 12 288 pairs: four slices (full kernel), seven (wgrad_kernel)
_WG27 = (0, 31, 33, 1, 0, 16, 7, 17, 2, 8, 9, 40, 1, 1, 7, 15, 64, 0, 0, 5, 32, 33, 6, 12, 1, 20, 0)


def _wgrad_cases():
    out = []
    full = ((32, 32, "1x1"), (32, 64, "1x2"), (32, 128, "1x4"), (64, 32, "2x1"), (64, 64, "2x2"), (64, 128, "2x4"),
            (96, 32, "3x1"), (96, 64, "3x2"), (96, 96, "3x3"), (128, 32, "4x1"), (128, 64, "4x2"), (128, 96, "4x3"))
    part = ((32, 96, "wg3a"), (32, 384, "wg4a"), (3, 32, "wg1u"), (20, 50, "wg2u"), (20, 96, "wg3u"), (20, 100, "wg4u"))
    for cin, cout, v in full:
        out.append(_c("wgrad", f"{cin}x{cout}-K8-tails", f"full{v}/S1", cin, cout, 8, 90, n_in=70, counts=_WG8,
                      capacity=sum(_WG8) + 50))
    for cin, cout, v in part:
        out.append(_c("wgrad", f"{cin}x{cout}-K8-tails", f"{v}/S1", cin, cout, 8, 90, n_in=70, counts=_WG8,
                      capacity=sum(_WG8) + 50))
    for cin, cout, v in ((32, 32, "1x1"), (96, 96, "3x3"), (64, 128, "2x4")):
        p = f"{cin}x{cout}"
        out += [
            _c("wgrad", f"{p}-K8-tails-acc", f"full{v}/S1", cin, cout, 8, 90, n_in=70, counts=_WG8, acc=True),
            _c("wgrad", f"{p}-K8-tails-shift", f"full{v}/S1", cin, cout, 8, 90, n_in=70, counts=_WG8, shift=True),
            _c("wgrad", f"{p}-K8-tails-acc-shift", f"full{v}/S1", cin, cout, 8, 90, n_in=70, counts=_WG8, acc=True,
               shift=True),
            _c("wgrad", f"{p}-K27-tails", f"full{v}/S1", cin, cout, 27, 120, n_in=70, counts=_WG27, background=True,
               repeat=cin == 96),
            _c("wgrad", f"{p}-K8-long", f"full{v}/S4", cin, cout, 8, 3000, n_in=2000, counts=_WG8_LONG, background=True),
            _c("wgrad", f"{p}-K8-long-acc", f"full{v}/S4", cin, cout, 8, 3000, n_in=2000, counts=_WG8_LONG, acc=True),
            _c("wgrad", f"{p}-K8-long-acc-shift", f"full{v}/S4", cin, cout, 8, 3000, n_in=2000, counts=_WG8_LONG,
               acc=True, shift=True, background=True),
        ]
        for n, S in ((1, 1), (255, 1), (256, 2), (257, 2), (5000, 20)):
            out.append(_c("wgrad", f"{p}-K1id-n{n}", f"full{v}/S{S}", cin, cout, 1, n, table=False))
        out.append(_c("wgrad", f"{p}-K1id-n255-acc-shift", f"full{v}/S1", cin, cout, 1, 255, table=False, acc=True,
                      shift=True))
        out.append(_c("wgrad", f"{p}-K1id-n5000-acc", f"full{v}/S20", cin, cout, 1, 5000, table=False, acc=True,
                      background=True))
    # the per-input-tile kernel always writes slices and reduces them: with more than one slice, into an unaligned dW
    out.append(_c("wgrad", "32x96-K8-long-acc", "wg3a/S7", 32, 96, 8, 3000, n_in=2000, counts=_WG8_LONG, acc=True))
    out.append(_c("wgrad", "20x50-K8-long-shift", "wg2u/S7", 20, 50, 8, 3000, n_in=2000, counts=_WG8_LONG, shift=True))
    out.append(_c("wgrad", "3x32-K1id-n5000", "wg1u/S3", 3, 32, 1, 5000, table=False))
    return out


def _stem_wgrad_cases():
    out = []
    for cin in (1, 2, 3, 4):
        for K in (8, 27, 32):
            for n in (1, 63, 5000):
                for acc in (False, True):
                    out.append(_c("stem_wgrad", f"{cin}x32-K{K}-n{n}{'-acc' if acc else ''}", "stemtable", cin, 32, K, n,
                                  n_in=max(n // 2, 9), acc=acc, repeat=(cin, K, n, acc) == (3, 27, 5000, False)))
    return out


def _group_cases():
    # n = the number of problems R; each problem has 90 rows of a / b
    return [_c("group", f"64x64-K8-R{R}{'-acc' if acc else ''}", "full2x2/S1", 64, 64, 8, R, n_in=70, counts=_WG8, acc=acc)
            for R in (2, 16) for acc in (True, False)] + \
           [_c("group", "96x96-K27-R2-acc", "full3x3/S1", 96, 96, 27, 2, n_in=70, counts=_WG27, acc=True)]


def _transpose_cases():
    return [_c("transpose", f"{cin}x{cout}-K{K}-m{m}", "transpose", cin, cout, K, 0, mirror=m)
            for cin, cout in ((64, 96), (3, 32), (20, 50)) for K in (1, 27) for m in (0, 1)]


CASES = {
    "row": _row_cases(), "stem": _stem_cases(), "compact": _compact_cases(), "sorted": _sorted_cases(),
    "pairs": _pairs_cases(), "wgrad": _wgrad_cases(), "stem_wgrad": _stem_wgrad_cases(), "group": _group_cases(),
    "transpose": _transpose_cases(),
}
GROUP_ROWS = 90                                  # rows of a / b of every problem of a "group" case


def all_cases():
    return [c for cs in CASES.values() for c in cs]


def exactness_bound(c):
    """An upper bound of mag over every element of an exact case, from the shape alone."""
    if c.family in ("row", "stem", "compact", "sorted"):
        return c.K * c.cin * 6 + 4                                   # K * cin products of at most 3 * 2, bias, before
    if c.family == "pairs":
        return c.cin * 6
    if c.family in ("wgrad", "group"):
        return (max(c.counts) if c.table else c.n) * 6 + 2          # one product per pair of an offset, before
    if c.family == "stem_wgrad":
        return c.n * 6 + 2
    return 0


def forward_cost(c):
    """Multiply-adds of a forward case's reference (to choose what a CPU test can afford)."""
    return c.n * c.K * c.cin * c.cout
