"""Cases, float64 references and comparators for the row kernels (csrc/rows.hip: batch norm in its three forms, ReLU,
pooling, gather / scatter, segment CSR and mean) and the batch-norm dispatch of csrc/units.hip, shared by
tests/test_rows_cases_host.py (CPU: every case reaches the form written next to it, the comparators accept an f32
evaluation and reject planted errors) and tests/test_gpu_rows_f64.py (every form, element-wise).  Nothing here touches a
device at import time and the references call nothing from the library: plain torch in float64, on whatever device the
inputs are on.

Batch-norm columns.  Column j of a case takes recipe (j + seed) % 8 of
  standard normal | 3 randn + 1 | mean 100, std 0.05 | mean -30, std 0.5 | a constant (var = 0) | std 1e-3 around 0
  (var << eps) | mean 1000, std 4 | integers in [-3, 3]
so that every kernel form sees the regime in which the design of these kernels shows: sums in f64 and
var = E[x^2] - mean^2.  That one-pass variance is accurate while E[x^2] / (var + eps) <= 2**24 (CONDITION_CAP; the host
test asserts it for every case).  To keep the cap at every row count, the three shifted recipes standardise their noise
per column (sample mean 0, sample variance 1 from two rows on: var is std^2 whatever the rows drawn), and on a one-row
map, where var = 0, their means are scaled into [-12, 12] (x^2 / eps <= 2**24 needs |x| <= 12.9).

References (f64 from the f32 inputs; `mag` = the sum of the absolute values of every term):
  statistics  m = mean(x), var = mean((x - m)^2) (two passes), invstd = 1 / sqrt(var + eps), scale = gamma invstd,
              shift = beta - m scale, running statistics by torch's rule (unbiased var n / (n - 1), factor 1 at n = 1)
  apply       out = [relu](x scale + shift [+ res]), mag = (|x| + |m|) |scale| + |beta| + |res|
  backward    inputs x, dy, y_out (the mask is y_out > 0 ON THOSE BITS) and f32 mean / invstd as a forward saved them:
              g = dy (y_out > 0), xhat = (x - mean) invstd, dbeta = sum g (+ before), dgamma = sum g xhat (+ before),
              dx = gamma invstd (g - mean_g - xhat mean_gx), dres = g bit for bit; training = 0: mean_g = mean_gx = 0;
              mag: every factor by its absolute value, x - mean by |x| + |mean|
  tile form   y = the G slices summed in slice order in f32 (bit-exact), then as above
Bounds: per element |y - ref| <= 2**-20 mag + 1e-30 (conv_cases.BOUND); the f64-summed statistics mean, dbeta, mean_g:
|err| <= 2**-23 |ref| + 2**-40 sum|terms| (/ n for a mean); invstd: <= 2**-22 ref.  Where dbeta is added into a
pre-existing f32 value, the f32 addition rounds sum g and the result once each: 2**-23 (|ref| + |before|) takes the
place of 2**-23 |ref|.

Plans are strings decoded from usc_bn_plan:
  statistics  refused | small/x0, small/x1 (one launch, XCD remap off / on) | two4/B<blocks>, two1/B<blocks>
  tile form   t<rows per tile>x<tiles>, "/u" appended where the unit calls take the tile form on that map
"""
import zlib
from dataclasses import dataclass

import torch

from conv_cases import BOUND, GuardedF32, GuardedWs, accepts, bounded_ratios  # noqa: F401  (re-exported)

EPS = 1e-5
MOMENTUM = 0.02
CONDITION_CAP = 2.0 ** 24
STAT_REL, STAT_ABS, INVSTD_REL = 2.0 ** -23, 2.0 ** -40, 2.0 ** -22
N_RECIPES = 8


# ------------------------------------------------------------------------------------------------- plans
def decode_plan(code):
    return dict(form=code & 3, remap=(code >> 2) & 1, vec=(code >> 3) & 7, blocks=(code >> 8) & 0xFFF,
                tile_ok=(code >> 20) & 1, units=(code >> 21) & 1, ntiles=(code >> 24) & 0xFF, tr=code >> 32)


def stat_plan_string(code):
    p = decode_plan(code)
    if p["form"] == 0:
        return "refused"
    return f"small/x{p['remap']}" if p["form"] == 1 else f"two{p['vec']}/B{p['blocks']}"


def tile_plan_string(code):
    p = decode_plan(code)
    if not p["tile_ok"]:
        return "none"
    return f"t{p['tr']}x{p['ntiles']}" + ("/u" if p["units"] else "")


def stat_form(plan):
    """The kernel form of a statistics plan string: without the block count."""
    return plan.split("/B")[0]


# ------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class BnCase:
    family: str                 # fwd (statistics + apply), bwd (reduce + dx), tile (both directions)
    name: str
    plan: str
    n: int
    c: int
    res: bool = False
    relu: bool = False
    dres: bool = False
    acc: bool = False           # dgamma / dbeta added into pre-existing values
    training: int = 1           # backward
    G: int = 0                  # tile: slices
    slice_acc: bool = False     # tile backward: dout' = dout + slices
    shift: bool = False         # parameters and their gradients one float into their buffers (4-byte aligned only)
    repeat: bool = False

    @property
    def seed(self):
        return zlib.crc32(f"{self.family}/{self.name}".encode()) & 0x7FFFFFFF

    @property
    def backward(self):
        return self.family == "bwd"


def decoded_plan(lib, c):
    code = lib.usc_bn_plan(c.n, c.c, int(c.backward))
    return tile_plan_string(code) if c.family == "tile" else stat_plan_string(code)


def _flags(i, **names):
    """Rotating flags: name -> bit of i."""
    return {k: bool((i >> b) & 1) for k, b in names.items()}


def _fwd_cases():
    out = []
    small = ((1, 4), (1, 256), (2, 36), (2, 1024), (255, 32), (255, 100), (256, 96), (256, 4), (257, 36), (257, 256),
             (1023, 100), (1023, 1024), (1024, 32), (1024, 36), (1025, 96), (1025, 100), (4096, 256), (4096, 4), (4096, 36))
    for i, (n, c) in enumerate(small):
        out.append(BnCase("fwd", f"n{n}-c{c}", f"small/x{int((c // 4) % 8 == 0)}", n, c, shift=i % 4 == 0,
                          repeat=i % 5 == 0, **_flags(i, res=0, relu=1)))
    two4 = ((4097, 4, 2), (4097, 100, 26), (4097, 1024, 257), (12000, 516, 750), (12000, 96, 75), (70001, 256, 1024),
            (16401, 1024, 1024))
    for i, (n, c, b) in enumerate(two4):
        out.append(BnCase("fwd", f"n{n}-c{c}", f"two4/B{b}", n, c, shift=i % 3 == 0, repeat=i == 1,
                          **_flags(i + 1, res=0, relu=1)))
    i = 0
    for c in (1, 3, 19, 255):
        for n in (1, 33, 5000):
            rp = 256 // c
            b = min(1024, -(-n // (rp * 16)))
            out.append(BnCase("fwd", f"n{n}-c{c}", f"two1/B{b}", n, c, shift=i % 3 == 1, repeat=i == 5,
                              **_flags(i, res=1, relu=0)))
            i += 1
    out.append(BnCase("fwd", "n5000-c258", "refused", 5000, 258))
    out.append(BnCase("fwd", "n100-c1025", "refused", 100, 1025))
    return out


def _bwd_cases():
    out = []
    rows = ((1, 36, "small/x0"), (1, 32, "small/x1"), (255, 100, "small/x0"), (255, 256, "small/x1"),
            (1024, 96, "small/x1"), (1024, 4, "small/x0"), (1024, 1024, "small/x1"),
            (1025, 32, "two4/B3"), (1025, 100, "two4/B7"), (1025, 516, "two4/B65"), (12000, 256, "two4/B188"),
            (16401, 1024, "two4/B1024"), (4097, 4, "two4/B2"),
            (5000, 19, "two1/B25"), (33, 3, "two1/B1"), (1, 255, "two1/B1"), (5000, 1, "two1/B2"), (5000, 255, "two1/B313"),
            (33, 19, "two1/B1"))
    for i, (n, c, plan) in enumerate(rows):
        out.append(BnCase("bwd", f"n{n}-c{c}", plan, n, c, shift=i % 3 == 0, repeat=i % 4 == 1, training=int(i % 4 != 2),
                          **_flags(i, relu=0, dres=1, acc=2)))
    out.append(BnCase("bwd", "n5000-c258", "refused", 5000, 258))
    out.append(BnCase("bwd", "n100-c1025", "refused", 100, 1025))
    return out


def _tile_cases():
    rows = ((1, 32, 0, "t32x1/u"), (31, 64, 1, "t32x1/u"), (32, 96, 7, "t32x1/u"), (33, 256, 8, "t32x2/u"),
            (2047, 32, 9, "t32x64/u"), (2048, 64, 16, "t32x64/u"), (2049, 96, 27, "t64x33/u"), (4096, 256, 0, "t64x64/u"),
            (4097, 32, 1, "t96x43"), (12000, 64, 7, "t192x63"), (33, 1024, 9, "t32x2/u"), (2048, 1024, 0, "t32x64/u"),
            (2049, 256, 8, "t64x33/u"), (4096, 96, 16, "t64x64/u"), (31, 32, 27, "t32x1/u"), (4097, 64, 0, "t96x43"))
    out = []
    for i, (n, c, G, plan) in enumerate(rows):
        out.append(BnCase("tile", f"n{n}-c{c}-G{G}", plan, n, c, G=G, shift=i % 3 == 0, repeat=i % 5 == 2,
                          training=int(i % 3 != 1), **_flags(i, res=0, relu=1, acc=2, slice_acc=3)))
    return [BnCase(**{**c.__dict__, "dres": c.res}) for c in out]


BN_CASES = {"fwd": _fwd_cases(), "bwd": _bwd_cases(), "tile": _tile_cases()}


def all_bn_cases():
    return [c for cs in BN_CASES.values() for c in cs]


# ------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def recipe_table(n, c, seed):
    """f32 [n, c]: column j by recipe (j + seed) % 8 (module docstring)."""
    g = _gen(seed)
    z = torch.randn((n, c), generator=g, dtype=torch.float64)
    ints = torch.randint(-3, 4, (n, c), generator=g).double()
    zs = z
    if n >= 2:
        zs = (z - z.mean(0)) / z.var(0, unbiased=False).sqrt()
    far, near = (1.0, 1.0) if n >= 2 else (0.011, 0.05)   # one row: var = 0, |x| <= 12.9 keeps x^2 / eps under the cap
    col = (torch.arange(c) + seed) % N_RECIPES
    cols = [z, 3 * z + 1, 100 * far + 0.05 * zs, -30 * min(1.0, far * 30) + 0.5 * near * zs, torch.full_like(z, 2.5),
            1e-3 * z, 1000 * far + 4 * near * zs, ints]
    x = torch.zeros((n, c), dtype=torch.float64)
    for r, t in enumerate(cols):
        x = torch.where(col == r, t, x)
    return x.float()


def condition(x, eps=EPS):
    """Largest E[x^2] / (var + eps) over the columns of x (f64, two-pass variance)."""
    xd = x.double()
    var = ((xd - xd.mean(0)) ** 2).mean(0)
    return float(((xd * xd).mean(0) / (var + eps)).max())


def params(c, seed):
    """gamma (with a negative and an exact 0), beta, running statistics that start at random values (one
    running_var = 0), pre-existing dgamma / dbeta."""
    g = _gen(seed + 7)
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[c // 2] = 0.0
    if c > 1:
        gamma[c - 1] = -gamma[c - 1]
    rv = torch.rand(c, generator=g) + 0.25
    rv[c // 3] = 0.0
    return dict(gamma=gamma, beta=torch.randn(c, generator=g), rm=torch.randn(c, generator=g), rv=rv,
                dgamma0=torch.randn(c, generator=g), dbeta0=torch.randn(c, generator=g))


def mask_input(n, c, seed):
    """y_out of a backward case: about half +0.0, the rest positive; a sprinkling of -0.0, of the smallest normal and of
    a denormal.  An input: the reference masks by y_out > 0 on these bits."""
    g = _gen(seed + 11)
    y = torch.randn((n, c), generator=g).clamp_min(0.0)
    pick = torch.randint(0, 16, (n, c), generator=g)
    y = torch.where(pick == 0, torch.full_like(y, -0.0), y)
    y = torch.where(pick == 1, torch.full_like(y, 1.17549435e-38), y)
    y = torch.where(pick == 2, torch.full_like(y, 1e-42), y)
    return y


def sum_slices_f32(slices, first=None):
    """first (or 0) + the slices in slice order, in f32: what the slice reductions of the library compute."""
    total = torch.zeros_like(slices[0]) if first is None else first.clone()
    for s in range(slices.shape[0]):
        total = total + slices[s]
    return total


def split_into_slices(y, G, seed):
    """G f32 slices whose f32 sum in slice order is close to y (the last slice is y minus the others)."""
    g = _gen(seed + 13)
    parts = torch.randn((G,) + tuple(y.shape), generator=g) * 0.5
    parts[G - 1] = y - sum_slices_f32(parts[:G - 1]) if G > 1 else y
    return parts


def bn_inputs(c):
    """CPU tensors of a batch-norm case."""
    t = params(c.c, c.seed)
    g = _gen(c.seed + 3)
    x = recipe_table(c.n, c.c, c.seed)
    if c.family == "tile" and c.G > 0:
        t["slices"] = split_into_slices(x, c.G, c.seed)
        x = sum_slices_f32(t["slices"])
    t["x"] = x
    t["res"] = torch.randn((c.n, c.c), generator=g) if c.res else None
    if c.family in ("bwd", "tile"):
        dy = torch.randn((c.n, c.c), generator=g)
        if c.family == "tile" and c.G > 0:
            t["dslices"] = split_into_slices(dy, c.G, c.seed + 1)
            t["dout0"] = torch.randn((c.n, c.c), generator=g)             # what dout holds before the call
            dy = sum_slices_f32(t["dslices"], t["dout0"] if c.slice_acc else None)
        t["dy"] = dy
        t["y_out"] = mask_input(c.n, c.c, c.seed) if c.relu else None
        st = ref_stats(x, t["gamma"], t["beta"], t["rm"], t["rv"])
        t["mean32"], t["invstd32"] = st["mean"].float(), st["invstd"].float()   # as a forward saved them
    return t


def to_device(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------- references
def ref_stats(x, gamma, beta, rm=None, rv=None, eps=EPS, momentum=MOMENTUM):
    xd = x.double()
    n = x.shape[0]
    m = xd.mean(0)
    var = ((xd - m) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    out = dict(mean=m, var=var, invstd=invstd, scale=scale, shift=beta.double() - m * scale,
               mean_terms=xd.abs().mean(0), scale_mag=gamma.double().abs() * invstd,
               shift_mag=beta.double().abs() + m.abs() * scale.abs())
    if rm is not None:
        unbiased = var * (n / (n - 1.0) if n > 1 else 1.0)
        out["rm"] = (1 - momentum) * rm.double() + momentum * m
        out["rv"] = (1 - momentum) * rv.double() + momentum * unbiased
        out["rm_mag"] = (1 - momentum) * rm.double().abs() + momentum * m.abs()
        out["rv_mag"] = (1 - momentum) * rv.double().abs() + momentum * unbiased
    return out


def ref_eval_stats(gamma, beta, rm, rv, eps=EPS):
    invstd = 1.0 / torch.sqrt(rv.double() + eps)
    scale = gamma.double() * invstd
    return dict(mean=rm.double(), invstd=invstd, scale=scale, shift=beta.double() - rm.double() * scale,
                scale_mag=gamma.double().abs() * invstd, shift_mag=beta.double().abs() + rm.double().abs() * scale.abs())


def ref_apply(x, st, beta, res=None, relu=False):
    """(out, mag)."""
    xd = x.double()
    out = xd * st["scale"] + st["shift"]
    mag = (xd.abs() + st["mean"].abs()) * st["scale"].abs() + beta.double().abs()
    if res is not None:
        out = out + res.double()
        mag = mag + res.double().abs()
    if relu:
        out = out.clamp_min(0.0)
    return out, mag


def ref_backward(x, dy, y_out, mean32, invstd32, gamma, training=1, dgamma0=None, dbeta0=None):
    xd, mu, is_ = x.double(), mean32.double(), invstd32.double()
    n = x.shape[0]
    g32 = dy if y_out is None else torch.where(y_out > 0, dy, torch.zeros_like(dy))     # dres: these bits
    g = g32.double()
    xhat = (xd - mu) * is_
    axhat = (xd.abs() + mu.abs()) * is_
    sg, sgx = g.sum(0), (g * xhat).sum(0)
    sg_terms, sgx_mag = g.abs().sum(0), (g.abs() * axhat).sum(0)
    mean_g = sg / n if training else torch.zeros_like(sg)
    mean_gx = sgx / n if training else torch.zeros_like(sgx)
    ga = gamma.double()
    out = dict(g32=g32, mean_g=mean_g, mean_g_terms=sg_terms / n, mean_gx=mean_gx, mean_gx_mag=sgx_mag / n,
               dbeta=sg, dbeta_terms=sg_terms, dbeta_before=torch.zeros_like(sg), dgamma=sgx, dgamma_mag=sgx_mag,
               dx=ga * is_ * (g - mean_g - xhat * mean_gx),
               dx_mag=ga.abs() * is_ * (g.abs() + mean_g.abs() + axhat * mean_gx.abs()))
    if dgamma0 is not None:
        out["dbeta"] = sg + dbeta0.double()
        out["dbeta_before"] = dbeta0.double().abs()
        out["dgamma"] = sgx + dgamma0.double()
        out["dgamma_mag"] = sgx_mag + dgamma0.double().abs()
    return out


# ------------------------------------------------------------------------------------------------- comparators
def _worst(err, bound):
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max()) if err.numel() else 0.0


def stat_ratio(y, ref, terms, before=None):
    """Largest |err| / (2**-23 (|ref| [+ |before|]) + 2**-40 terms + 1e-30)."""
    rel = ref.abs() if before is None else ref.abs() + before
    return _worst((y.double() - ref).abs(), STAT_REL * rel + STAT_ABS * terms + 1e-30)


def invstd_ratio(y, ref):
    return _worst((y.double() - ref).abs(), INVSTD_REL * ref)


def elem_ratio(y, ref, mag):
    return bounded_ratios(y, ref, mag)[0] if y.numel() else 0.0


def stats_fractions(got, st):
    """Fractions of their bounds the outputs of a statistics call use.  got: name -> f32 tensor (mean, invstd, scale,
    shift, and rm / rv when st has them)."""
    f = dict(mean=stat_ratio(got["mean"], st["mean"], st["mean_terms"]), invstd=invstd_ratio(got["invstd"], st["invstd"]),
             scale=elem_ratio(got["scale"], st["scale"], st["scale_mag"]),
             shift=elem_ratio(got["shift"], st["shift"], st["shift_mag"]))
    if "rm" in st and "rm" in got:
        f["running_mean"] = elem_ratio(got["rm"], st["rm"], st["rm_mag"])
        f["running_var"] = elem_ratio(got["rv"], st["rv"], st["rv_mag"])
    return f


def backward_fractions(got, rb):
    """got: dbeta, dgamma, dx and (two-launch forms) mean_g, mean_gx."""
    f = dict(dbeta=stat_ratio(got["dbeta"], rb["dbeta"], rb["dbeta_terms"], rb["dbeta_before"]),
             dgamma=elem_ratio(got["dgamma"], rb["dgamma"], rb["dgamma_mag"]),
             dx=elem_ratio(got["dx"], rb["dx"], rb["dx_mag"]))
    if "mean_g" in got:
        f["mean_g"] = stat_ratio(got["mean_g"], rb["mean_g"], rb["mean_g_terms"])
        f["mean_gx"] = elem_ratio(got["mean_gx"], rb["mean_gx"], rb["mean_gx_mag"])
    return f


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------- row movers
RELU_NUMELS = (0, 1, 3, 4, 5, 1027, 262147)


@dataclass(frozen=True)
class PoolCase:
    name: str
    c: int
    ld: int
    n_coarse: int = 301
    n_fine: int = 700
    row_of: bool = False

    @property
    def vec(self):
        return 4 if self.c % 4 == 0 and self.ld % 4 == 0 else 1


POOL_CASES = [PoolCase(f"c{c}-ld{ld}{'-rowof' if r else ''}", c, ld, row_of=r)
              for c, ld in ((3, 3), (4, 4), (100, 100), (128, 128), (100, 128), (4, 6), (100, 102), (3, 128))
              for r in (False, True)]


def pool_inputs(c, mode, seed=0):
    """in [rows, ld], row_of i64[n_fine] or None, nbr2 i32[8, n_coarse] whose columns have 0, 1, 2, 4 or 8 children
    (exact mode: sum / count is exact) or any count (bounded mode)."""
    g = _gen(zlib.crc32(c.name.encode()) + seed + (0 if mode == "exact" else 1))
    rows = 57 if c.row_of else c.n_fine
    src = (torch.randint(-3, 4, (rows, c.ld), generator=g).float() if mode == "exact"
           else torch.randn((rows, c.ld), generator=g))
    counts = torch.tensor([0, 1, 2, 4, 8])[torch.randint(0, 5, (c.n_coarse,), generator=g)] if mode == "exact" \
        else torch.randint(0, 9, (c.n_coarse,), generator=g)
    counts[0], counts[1] = 0, 8
    nbr2 = torch.full((8, c.n_coarse), -1, dtype=torch.int32)
    for p in range(c.n_coarse):
        slots = torch.randperm(8, generator=g)[:int(counts[p])]
        nbr2[slots, p] = torch.randint(0, c.n_fine, (int(counts[p]),), generator=g).int()
    row_of = torch.randint(0, rows, (c.n_fine,), generator=g) if c.row_of else None
    return dict(src=src, nbr2=nbr2, row_of=row_of)


def ref_pool(src, nbr2, row_of, c):
    """(mean, mag) f64 [n_coarse, c]."""
    n_coarse = nbr2.shape[1]
    total = torch.zeros((n_coarse, c), dtype=torch.float64, device=src.device)
    mag = torch.zeros_like(total)
    cnt = torch.zeros(n_coarse, dtype=torch.float64, device=src.device)
    sd = src.double()[:, :c]
    for k in range(8):
        ch = nbr2[k].long()
        ok = ch >= 0
        ch = ch.clamp_min(0)
        rows = row_of[ch] if row_of is not None else ch
        v = torch.where(ok[:, None], sd[rows], torch.zeros_like(total))
        total += v
        mag += v.abs()
        cnt += ok.double()
    d = cnt.clamp_min(1.0)[:, None]
    return total / d, mag / d


@dataclass(frozen=True)
class MoveCase:
    name: str
    c: int
    kind: str                   # perm, subset, dup
    n_src: int = 777            # rows of the table
    n: int = 777                # indices

    @property
    def seed(self):
        return zlib.crc32(self.name.encode()) & 0x7FFFFFFF


MOVE_CASES = [MoveCase(f"c{c}-{kind}", c, kind, n={"perm": 777, "subset": 300, "dup": 1500}[kind])
              for c in (1, 19, 96, 128) for kind in ("perm", "subset", "dup")]


def move_indices(c):
    g = _gen(c.seed)
    if c.kind == "dup":
        return torch.randint(0, c.n_src // 4, (c.n,), generator=g)       # every named row several times
    return torch.randperm(c.n_src, generator=g)[:c.n]


def move_values(shape, mode, seed):
    g = _gen(seed + (0 if mode == "exact" else 1))
    return torch.randint(-3, 4, shape, generator=g).float() if mode == "exact" else torch.randn(shape, generator=g)


@dataclass(frozen=True)
class SegCase:
    name: str
    n: int
    S: int
    c: int
    layout: str = "shuffle"     # shuffle | chunks (rows 0..63 one id, rows 64..127 sixty-four ids) | one (a single id)

    @property
    def seed(self):
        return zlib.crc32(self.name.encode()) & 0x7FFFFFFF

    @property
    def vec(self):
        return self.c % 4 == 0 and self.c <= 128


SEG_CASES = [SegCase(f"n{n}-S{S}-c{c}-{lay}", n, S, c, lay) for n, S, c, lay in (
    (0, 1, 4, "shuffle"), (0, 321, 3, "shuffle"), (1, 1, 128, "one"), (1, 321, 132, "shuffle"), (1023, 321, 4, "shuffle"),
    (1024, 1, 128, "one"), (1024, 321, 3, "chunks"), (1025, 321, 128, "chunks"), (1025, 5000, 384, "shuffle"),
    (5000, 5000, 4, "shuffle"), (5000, 321, 576, "chunks"), (5000, 1, 132, "one"), (5000, 321, 128, "shuffle"),
    (1023, 5000, 576, "shuffle"))]


def segment_ids(c):
    """i64[n] segment ids in [0, S) with power-of-two segment sizes wherever the rows allow and every third id empty."""
    g = _gen(c.seed)
    if c.n == 0:
        return torch.zeros(0, dtype=torch.int64)
    if c.layout == "one":
        return torch.full((c.n,), c.S - 1, dtype=torch.int64)
    sizes, rem, s = [], c.n, 0
    if c.layout == "chunks":
        sizes, rem = [64] + [1] * 64, c.n - 128
    pattern = (1, 2, 0, 4, 8, 0, 16, 64, 0, 32, 1, 0)
    while rem > 0 and len(sizes) < c.S:
        want = pattern[s % len(pattern)]
        s += 1
        take = min(want, rem)
        take = 1 << (take.bit_length() - 1) if take else 0
        sizes.append(take)
        rem -= take
    ids = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if rem > 0:                          # more rows than the pattern places: the rest into the segments it gave 64 rows
        big = torch.tensor([i for i, v in enumerate(sizes) if v == 64 and i > 0])
        ids = torch.cat([ids, big[torch.randint(0, big.shape[0], (rem,), generator=g)]])
    if c.layout == "shuffle":
        ids = ids[torch.randperm(c.n, generator=g)]
    return ids.long()


def segment_values(c, mode):
    """f32 [n, c] with about a fifth of the rows all zero, and every row of the segments 4, 16, 28, ... zero."""
    g = _gen(c.seed + (5 if mode == "exact" else 6))
    v = torch.randint(-3, 4, (c.n, c.c), generator=g).float() if mode == "exact" else torch.randn((c.n, c.c), generator=g)
    zero = torch.rand(c.n, generator=g) < 0.2
    zero |= (segment_ids(c) % 12) == 4
    v[zero] = 0.0
    return v


def ref_segment(src, seg, S, mode):
    """(out, mag, cnt) f64 [S, c] of mode 'mean', 'mean_nonzero' or 'max_nonzero'; cnt i64[S] the rows used."""
    sd = src.double()
    use = torch.ones(src.shape[0], dtype=torch.bool, device=src.device) if mode == "mean" else (src != 0).any(1)
    cnt = torch.zeros(S, dtype=torch.int64, device=src.device).index_add_(0, seg[use], torch.ones_like(seg[use]))
    c = src.shape[1]
    if mode == "max_nonzero":
        out = torch.full((S, c), float("-inf"), dtype=torch.float64, device=src.device)
        out = out.scatter_reduce(0, seg[use][:, None].expand(-1, c), sd[use], "amax", include_self=True)
        out = torch.where(cnt[:, None] > 0, out, torch.zeros_like(out))
        return out, out.abs(), cnt
    total = torch.zeros((S, c), dtype=torch.float64, device=src.device).index_add_(0, seg[use], sd[use])
    mag = torch.zeros_like(total).index_add_(0, seg[use], sd[use].abs())
    d = cnt.clamp_min(1).double()[:, None]
    return total / d, mag / d, cnt


def is_pow2(cnt):
    return (cnt > 0) & ((cnt & (cnt - 1)) == 0)
