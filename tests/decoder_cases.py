"""Cases, float64 references and comparators for the decoder's small-row kernels (csrc/decoder.hip: LayerNorm forward
and backward, the 32x32-tile linear forward in its plain / padded / split forms, the fused dx | dW | db backward with its
extra operands, the one-launch q/k/v backward and the fixed-order column sum), shared by tests/test_decoder_cases_host.py
(CPU: the table holds every size the kernels branch on, the comparators accept an f32 evaluation in the kernels'
partition and reject planted errors) and tests/test_gpu_decoder_f64.py (every entry point, element-wise).  Nothing here
touches a device at import time and the references call nothing from the library: plain torch in float64, on whatever
device the inputs are on.

Modes (conv_cases.MODES).  exact: integers in [-3, 3] (every partial sum stays below EXACT_LIMIT, the host test asserts
it through `mag`): the kernel must equal the float64 result bit for bit.  bounded: random inputs, per element
|y - ref| <= BOUND mag + 1e-30 with mag = the sum of the absolute values of every term and BOUND = 2**-20.  The linear
families run in both modes; LayerNorm runs bounded, with sum_out = f32(x + res) bit for bit.

References (f64 from the f32 inputs):
  linear forward   ref = [relu]((x + x2) W^T + b), mag = sum_k (|x| + |x2|) |W| + |b|; x2 enters the output columns
                   < x2_cols only; split layout [N / split][M][split]; rows M .. M_pad - 1 are +0.0
  linear backward  g = dy (y_relu > 0) ON THE BITS of y_relu, dx_b = g W + dx_add, dx = dx_b + dx_add2,
                   dW = g^T (x + x2) (+ dW0), db = sum_m g (+ db0); mag: every product by absolute values, every addend
                   by its absolute value
  q/k/v backward   dy3 = dq | dk | dv, dx_b = dq Wq + dk Wk, dx = dx_b + dv Wv + dres,
                   dW_j = dy_j^T (x + [j < 2] pos) (+ dW0), db_j = sum_m dy_j (+ db0)
  LayerNorm fwd    v = x (+ res), mean / rstd by a two-pass f64 evaluation, y = (v - mean) rstd gamma + beta,
                   mag_y = (|v| + |mean|) rstd |gamma| + |beta|
  LayerNorm bwd    inputs x, dy and the F32 mean / rstd as a forward saved them: xhat = (x - mean) rstd, gy = dy gamma,
                   dx = rstd (gy - mean(gy) - xhat mean(gy xhat)) + dx_add, dgamma = sum_r dy xhat (+ before),
                   dbeta = sum_r dy (+ before); mag: every factor by its absolute value, x - mean by |x| + |mean|, the
                   two row means by the means of the absolute values
  column sum       sum_r x (+ before), mag = sum |x| + |before|

The two LayerNorm statistics are an f32 wave sum (lane l holds columns l, l + 64, ..., then the butterfly of
wave_reduce_addf) and an rsqrtf of a second such sum around the first: their bounds are BOUND mag with mag = mean|v|
for the mean and mag = rstd for rstd.  Row r of a case takes recipe (r + seed) % 8 of
  standard normal | 3 randn + 1 | mean 100, std 0.05 | mean -30, std 0.5 | the constant 2.5 (var = 0) | 1e-4 randn
  (spread << sqrt(eps)) | mean 1000, std 4 | integers in [-3, 3]
(the three shifted recipes standardise their noise per row).  tests/test_decoder_cases_host.py evaluates the kernel's
arithmetic in f32 on the CPU for every case: it uses at most half of each bound on these recipes, whose conditioning
mean(|v|)^2 / (var + eps) stays below LN_CONDITION_CAP (asserted there for every case).
"""
import zlib
from dataclasses import dataclass

import torch

from conv_cases import (BOUND, EXACT_LIMIT, MODES, GuardedF32, GuardedWs, accepts, bounded_ratios,  # noqa: F401
                        exact_mismatches)
from rows_cases import CONDITION_CAP, _flags, _gen, _worst, mask_input, move_values, same_bits, to_device  # noqa: F401

EPS = 1e-5
LN_CONDITION_CAP = 2.0 ** 22        # mean(|v|)^2 / (var + eps) of a LayerNorm row; rows_cases.CONDITION_CAP is 2**24
LN_DIMS = (64, 128, 192, 256, 384, 512)
LN_ROWS_NARROW = (1, 3, 4, 5, 100, 128, 129, 1024, 1025, 1152, 1153, 2500)         # d <= 128: prefetch up to 128 rows
LN_ROWS_WIDE = (1, 5, 64, 65, 1024, 1025, 1088, 1089)                              # d >= 192: prefetch up to 64 rows
LN_ROWS_PER_BLOCK = 1024
LN_REFUSED_DIMS = (320, 448, 32, 576)
N_RECIPES = 8

LIN_M = (1, 31, 32, 33, 100, 129)
LIN_NK = ((32, 32), (32, 96), (96, 160), (128, 128), (1024, 128), (128, 1024))
PAD_ROWS = ((100, 128), (100, 110), (1, 64), (33, 33), (32, 33))
QKV_E = (32, 96, 128)
QKV_M = (1, 100, 129)
COLSUM_C = (1, 17, 65)
COLSUM_N = (63, 64, 65, 1025)
EX_OPERANDS = ("y_relu", "x2", "dx_add", "dx_add2", "dx_b")
OUTPUTS = ("dx", "dW+db", "dW", "all")           # dx only | dW and db, no dx | dW without db, no dx | everything


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class LnCase:
    name: str
    rows: int
    d: int
    res: bool = False           # forward: y = LN(x + res), sum_out written
    dx_add: bool = False        # backward
    accumulate: bool = False    # backward: dgamma / dbeta added into pre-existing values
    repeat: bool = False
    shift: bool = False         # gamma / beta / dgamma / dbeta one float into their buffers (4-byte aligned only)

    @property
    def seed(self):
        return _seed("ln", self.name)

    @property
    def launches(self):
        return 1 if self.rows <= LN_ROWS_PER_BLOCK else 2


def _ln_cases():
    shapes = [(r, 128) for r in LN_ROWS_NARROW] + [(r, 192) for r in LN_ROWS_WIDE]
    shapes += [(100, 64), (129, 64), (1152, 64), (64, 256), (65, 256), (1089, 256), (5, 384), (65, 384), (1088, 384),
               (1, 512), (64, 512), (1025, 512)]
    out = []
    for i, (rows, d) in enumerate(shapes):
        out.append(LnCase(f"r{rows}-d{d}", rows, d, **_flags(i * 3 + 2, accumulate=0, res=1, dx_add=2, shift=3, repeat=4)))
    return out


LN_CASES = _ln_cases()


@dataclass(frozen=True)
class LinCase:
    family: str                 # fwd | pad | split | bwd_plain | bwd_ex | qkv
    name: str
    M: int
    N: int
    K: int
    x2: bool = False
    b: bool = True
    relu: bool = False
    M_pad: int = 0              # pad
    x2_cols: int = 0            # split
    split: int = 0              # split
    operands: tuple = ()        # bwd_ex: the subset of EX_OPERANDS; qkv: the subset of ("pos", "dres", "dx_b", "db")
    outputs: str = "all"        # bwd_*: one of OUTPUTS
    accumulate: bool = False
    repeat: bool = False

    @property
    def seed(self):
        return _seed(self.family, self.name)

    def has(self, operand):
        return operand in self.operands

    @property
    def want_dx(self):
        return self.outputs in ("dx", "all")

    @property
    def want_dW(self):
        return self.outputs != "dx"

    @property
    def want_db(self):
        return self.outputs in ("dW+db", "all")


def _shapes():
    return [(M, N, K) for M in LIN_M for (N, K) in LIN_NK]


def _fwd_cases():
    out = []
    for i, (M, N, K) in enumerate(_shapes()):
        f = _flags(i + i // 6 + 1, x2=0, relu=1, nob=2)
        out.append(LinCase("fwd", f"m{M}-n{N}-k{K}", M, N, K, x2=f["x2"], relu=f["relu"], b=not f["nob"], repeat=i % 6 == 1))
    return out


def _pad_cases():
    nk = ((96, 160), (32, 96), (128, 128), (32, 32), (1024, 128))
    return [LinCase("pad", f"m{M}-pad{Mp}-n{N}-k{K}", M, N, K, M_pad=Mp, **_flags(i, x2=0, relu=1), repeat=i == 1)
            for i, ((M, Mp), (N, K)) in enumerate(zip(PAD_ROWS, nk))]


def _split_cases():
    out = []
    rows = (100, 1, 33, 129, 32, 31, 100, 33, 129)
    i = 0
    for E in QKV_E:
        for cols in (0, 2 * E, 3 * E):
            out.append(LinCase("split", f"e{E}-x2cols{cols}-m{rows[i]}", rows[i], 3 * E, E, x2=True, x2_cols=cols, split=E,
                               repeat=i == 4))
            i += 1
    out.append(LinCase("split", "e96-one-piece", 100, 288, 96, x2=True, x2_cols=192, split=288))
    out.append(LinCase("split", "e128-no-bias", 33, 384, 128, x2=True, x2_cols=256, split=128, b=False))
    out.append(LinCase("split", "e96-no-x2", 33, 288, 96, x2=False, x2_cols=192, split=96))
    return out


def _bwd_cases():
    plain, ex = [], []
    patterns = [(o,) for o in EX_OPERANDS] + [EX_OPERANDS]
    for i, (M, N, K) in enumerate(_shapes()):
        acc = bool((i // 2) % 2)
        plain.append(LinCase("bwd_plain", f"m{M}-n{N}-k{K}", M, N, K, outputs=OUTPUTS[(i + i // 6) % 4], accumulate=acc,
                             repeat=i % 7 == 3))
        ops = patterns[(i + i // 6) % 6]
        outs = OUTPUTS[(i + i // 6 + 1) % 4]
        if set(ops) & {"dx_add", "dx_add2", "dx_b"} and outs in ("dW+db", "dW"):          # these operands need dx
            outs = "all" if len(ops) > 1 else ("all", "dx")[(i // 3) % 2]
        ex.append(LinCase("bwd_ex", f"m{M}-n{N}-k{K}-{ops[0] if len(ops) == 1 else 'every'}", M, N, K, x2="x2" in ops,
                          operands=tuple(ops), outputs=outs, accumulate=acc, repeat=i % 7 == 5))
    return plain, ex


def _qkv_cases():
    out = []
    names = ("pos", "dres", "dx_b", "db")
    i = 0
    for rep in range(2):
        for E in QKV_E:
            for M in QKV_M:
                f = _flags(i * 11 + 5 + rep, pos=0, dres=1, dx_b=2, db=3, accumulate=4)
                ops = tuple(n for n in names if f[n])
                out.append(LinCase("qkv", f"e{E}-m{M}-" + ("+".join(ops) or "bare") + ("-acc" if f["accumulate"] else ""), M,
                                   3 * E, E, operands=ops, accumulate=f["accumulate"], repeat=i % 5 == 2))
                i += 1
    return out


_PLAIN, _EX = _bwd_cases()
LIN_CASES = {"fwd": _fwd_cases(), "pad": _pad_cases(), "split": _split_cases(), "bwd_plain": _PLAIN, "bwd_ex": _EX,
             "qkv": _qkv_cases()}


def all_lin_cases():
    return [c for cs in LIN_CASES.values() for c in cs]


@dataclass(frozen=True)
class ColSumCase:
    name: str
    n: int
    c: int
    accumulate: bool = False

    @property
    def seed(self):
        return _seed("colsum", self.name)


COLSUM_CASES = [ColSumCase(f"n{n}-c{c}{'-acc' if (i + j) % 2 else ''}", n, c, bool((i + j) % 2))
                for i, n in enumerate(COLSUM_N) for j, c in enumerate(COLSUM_C)]
COLSUM_CASES += [ColSumCase("n0-c17", 0, 17), ColSumCase("n0-c17-acc", 0, 17, True)]


# ------------------------------------------------------------------------------------------------- inputs
def ln_rows(rows, d, seed):
    """f32 [rows, d]: row r by recipe (r + seed) % 8 (module docstring)."""
    g = _gen(seed)
    z = torch.randn((rows, d), generator=g, dtype=torch.float64)
    ints = torch.randint(-3, 4, (rows, d), generator=g).double()
    zs = (z - z.mean(1, keepdim=True)) / z.var(1, unbiased=False, keepdim=True).sqrt()
    kind = ((torch.arange(rows) + seed) % N_RECIPES)[:, None]
    recipes = [z, 3 * z + 1, 100 + 0.05 * zs, -30 + 0.5 * zs, torch.full_like(z, 2.5), 1e-4 * z, 1000 + 4 * zs, ints]
    v = torch.zeros((rows, d), dtype=torch.float64)
    for r, t in enumerate(recipes):
        v = torch.where(kind == r, t, v)
    return v.float()


def ln_condition(v, eps=EPS):
    """Largest mean(|v|)^2 / (var + eps) over the rows of v (f64, two-pass variance)."""
    vd = v.double()
    var = ((vd - vd.mean(1, keepdim=True)) ** 2).mean(1)
    return float((vd.abs().mean(1) ** 2 / (var + eps)).max()) if v.numel() else 0.0


def ln_inputs(c):
    """CPU tensors of a LayerNorm case.  With a residual, res lies on a quarter grid and x = v - res, so that the constant
    and the integer rows of v = f32(x + res) stay what their recipe says; `v` is that sum, the backward's x."""
    g = _gen(c.seed + 3)
    v0 = ln_rows(c.rows, c.d, c.seed)
    t = dict(x=v0, res=None)
    if c.res:
        t["res"] = torch.randint(-8, 9, (c.rows, c.d), generator=g).float() / 4
        t["x"] = (v0.double() - t["res"].double()).float()
    t["v"] = t["x"] + t["res"] if c.res else t["x"]
    gamma = torch.rand(c.d, generator=g) + 0.5
    gamma[c.d // 2] = 0.0
    gamma[c.d - 1] = -gamma[c.d - 1]
    t.update(gamma=gamma, beta=torch.randn(c.d, generator=g), dgamma0=torch.randn(c.d, generator=g),
             dbeta0=torch.randn(c.d, generator=g), dy=torch.randn((c.rows, c.d), generator=g),
             dx_add=torch.randn((c.rows, c.d), generator=g) if c.dx_add else None)
    st = ref_ln_stats(t["v"])
    t["mean32"], t["rstd32"] = st["mean"].float(), st["rstd"].float()           # as a forward saved them
    return t


def lin_inputs(c, mode):
    """CPU tensors of a linear case (every family): only what the case names is present, the rest is None."""
    s = c.seed
    M, N, K = c.M, c.N, c.K

    def val(shape, k, on=True):
        return move_values(shape, mode, s + k) if on else None

    t = dict(x=val((M, K), 1), W=val((N, K), 2), b=val((N,), 3, c.b), x2=val((M, K), 4, c.x2))
    if c.family in ("bwd_plain", "bwd_ex"):
        t.update(dy=val((M, N), 5), y_relu=mask_input(M, N, s) if c.has("y_relu") else None,
                 dx_add=val((M, K), 6, c.has("dx_add")), dx_add2=val((M, K), 7, c.has("dx_add2")),
                 dW0=val((N, K), 8), db0=val((N,), 9))
    if c.family == "qkv":
        E = K
        t = dict(dy3=val((3, M, E), 5), x=val((M, E), 1), W=val((3 * E, E), 2), pos=val((M, E), 4, c.has("pos")),
                 dres=val((M, E), 6, c.has("dres")), dW0=val((3 * E, E), 8), db0=val((3 * E,), 9))
    return t


def colsum_inputs(c, mode):
    return dict(x=move_values((c.n, c.c), mode, c.seed), before=move_values((c.c,), mode, c.seed + 1))


# ------------------------------------------------------------------------------------------------- references
def _d(t):
    return None if t is None else t.double()


def ref_linear_fwd(x, x2, W, b, relu=False, x2_cols=None):
    """(ref, mag) f64 [M, N]."""
    xd, Wd = x.double(), W.double()
    ref, mag = xd @ Wd.T, xd.abs() @ Wd.abs().T
    if x2 is not None:
        N = W.shape[0]
        sel = (torch.arange(N, device=x.device) < (N if x2_cols is None else x2_cols)).double()
        ref = ref + (x2.double() @ Wd.T) * sel
        mag = mag + (x2.double().abs() @ Wd.abs().T) * sel
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    return (ref.clamp_min(0.0) if relu else ref), mag


def split_layout(y, split):
    """[M, N] -> [N / split][M][split] as one [N / split * M, split] table."""
    M, N = y.shape
    return y.view(M, N // split, split).permute(1, 0, 2).reshape(-1, split)


def masked(dy, y_relu):
    return dy if y_relu is None else torch.where(y_relu > 0, dy, torch.zeros_like(dy))


def ref_linear_bwd(dy, y_relu, x, x2, W, dx_add=None, dx_add2=None, dW0=None, db0=None):
    """name -> (ref, mag) for dx_b, dx, dW, db."""
    g = masked(dy, y_relu).double()
    Wd = W.double()
    dxb, dxb_mag = g @ Wd, g.abs() @ Wd.abs()
    if dx_add is not None:
        dxb, dxb_mag = dxb + dx_add.double(), dxb_mag + dx_add.double().abs()
    dx, dx_mag = dxb, dxb_mag
    if dx_add2 is not None:
        dx, dx_mag = dxb + dx_add2.double(), dxb_mag + dx_add2.double().abs()
    xs, xs_mag = x.double(), x.double().abs()
    if x2 is not None:
        xs, xs_mag = xs + x2.double(), xs_mag + x2.double().abs()
    dW, dW_mag = g.T @ xs, g.abs().T @ xs_mag
    db, db_mag = g.sum(0), g.abs().sum(0)
    if dW0 is not None:
        dW, dW_mag = dW + dW0.double(), dW_mag + dW0.double().abs()
    if db0 is not None:
        db, db_mag = db + db0.double(), db_mag + db0.double().abs()
    return dict(dx_b=(dxb, dxb_mag), dx=(dx, dx_mag), dW=(dW, dW_mag), db=(db, db_mag))


def ref_qkv_bwd(dy3, x, pos, W, dres=None, dW0=None, db0=None):
    """name -> (ref, mag) for dx_b, dx, dW [3E, E], db [3E] (the formulas above qkv_bwd_kernel)."""
    E = x.shape[1]
    d3, Wd = dy3.double(), W.double().view(3, E, E)
    prod = [d3[j] @ Wd[j] for j in range(3)]
    pmag = [d3[j].abs() @ Wd[j].abs() for j in range(3)]
    dxb, dxb_mag = prod[0] + prod[1], pmag[0] + pmag[1]
    dx, dx_mag = dxb + prod[2], dxb_mag + pmag[2]
    if dres is not None:
        dx, dx_mag = dx + dres.double(), dx_mag + dres.double().abs()
    xs = [x.double() + (pos.double() if pos is not None and j < 2 else 0.0) for j in range(3)]
    xm = [x.double().abs() + (pos.double().abs() if pos is not None and j < 2 else 0.0) for j in range(3)]
    dW = torch.cat([d3[j].T @ xs[j] for j in range(3)])
    dW_mag = torch.cat([d3[j].abs().T @ xm[j] for j in range(3)])
    db, db_mag = d3.sum(1).reshape(-1), d3.abs().sum(1).reshape(-1)
    if dW0 is not None:
        dW, dW_mag = dW + dW0.double(), dW_mag + dW0.double().abs()
    if db0 is not None:
        db, db_mag = db + db0.double(), db_mag + db0.double().abs()
    return dict(dx_b=(dxb, dxb_mag), dx=(dx, dx_mag), dW=(dW, dW_mag), db=(db, db_mag))


def ref_ln_stats(v, eps=EPS):
    vd = v.double()
    mean = vd.mean(1)
    var = ((vd - mean[:, None]) ** 2).mean(1)
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), mean_mag=vd.abs().mean(1))


def ref_ln_fwd(v, gamma, beta, eps=EPS):
    """v = x (+ res) in f32 -> dict(mean, rstd, mean_mag, y, y_mag)."""
    st = ref_ln_stats(v, eps)
    vd, m, rs = v.double(), st["mean"][:, None], st["rstd"][:, None]
    st["y"] = (vd - m) * rs * gamma.double() + beta.double()
    st["y_mag"] = (vd.abs() + m.abs()) * rs * gamma.double().abs() + beta.double().abs()
    return st


def ref_ln_bwd(x, dy, mean32, rstd32, gamma, dx_add=None, dgamma0=None, dbeta0=None):
    """name -> (ref, mag) for dx, dgamma, dbeta."""
    xd, dyd = x.double(), dy.double()
    mu, rs = mean32.double()[:, None], rstd32.double()[:, None]
    xhat, axhat = (xd - mu) * rs, (xd.abs() + mu.abs()) * rs
    gy = dyd * gamma.double()
    m1, m2 = gy.mean(1, keepdim=True), (gy * xhat).mean(1, keepdim=True)
    a1, a2 = gy.abs().mean(1, keepdim=True), (gy.abs() * axhat).mean(1, keepdim=True)
    dx, dx_mag = rs * (gy - m1 - xhat * m2), rs * (gy.abs() + a1 + axhat * a2)
    if dx_add is not None:
        dx, dx_mag = dx + dx_add.double(), dx_mag + dx_add.double().abs()
    dg, dg_mag = (dyd * xhat).sum(0), (dyd.abs() * axhat).sum(0)
    db, db_mag = dyd.sum(0), dyd.abs().sum(0)
    if dgamma0 is not None:
        dg, dg_mag = dg + dgamma0.double(), dg_mag + dgamma0.double().abs()
        db, db_mag = db + dbeta0.double(), db_mag + dbeta0.double().abs()
    return dict(dx=(dx, dx_mag), dgamma=(dg, dg_mag), dbeta=(db, db_mag))


def ref_col_sum(x, before=None):
    s, mag = x.double().sum(0), x.double().abs().sum(0)
    if before is not None:
        s, mag = s + before.double(), mag + before.double().abs()
    return s, mag


# ------------------------------------------------------------------------------------------------- comparators
def fraction(mode, y, ref, mag):
    """exact: 0 where y equals the reference in every element, inf otherwise; bounded: the largest |err| / bound."""
    if y.numel() == 0:
        return 0.0
    if mode == "exact":
        return float("inf") if exact_mismatches(y, ref.view(y.shape)) else 0.0
    return bounded_ratios(y, ref.view(y.shape), mag.view(y.shape))[0]


def fractions(mode, got, refs):
    """got: name -> f32 tensor; refs: name -> (ref, mag).  The fraction of its bound every output of `got` uses."""
    return {k: fraction(mode, v, *refs[k]) for k, v in got.items()}


def ln_stat_fractions(mean, rstd, st):
    return dict(mean=_worst((mean.double() - st["mean"]).abs(), BOUND * st["mean_mag"] + 1e-30),
                rstd=_worst((rstd.double() - st["rstd"]).abs(), BOUND * st["rstd"]))


def largest_partial_sum(refs):
    """An upper limit of every partial sum of every output: the largest mag."""
    return max(float(mag.max()) for _, mag in refs.values() if mag.numel())
