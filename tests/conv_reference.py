"""Float64 restatement of the convolution core's formula (csrc/kernels.h, ConvArgs) on STORED values, the five storage
layouts' encoders and decoders, and the data sets and shape table of the configuration sweep
(tests/test_gpu_conv_cfgs.py, checked on the host by tests/test_conv_reference_host.py).

    out[m][co] = store(act(sum_k x[pix(m) + tap(k)] * w[co][k] + bias[m][co] + res[m][co]))

m = (n*Ho + ho)*Wo + wo, k = (kh*KW + kw)*Cin + c.  x, w and res are the values the layout holds (after rounding to
bf16 / f16, or the hi + lo a split-f16 pair stands for); a pre-conv BatchNorm x*s + t on the unpadded input is folded as
add_conv (csrc/plan.cpp) folds it -- w' = fp32(w*s), and the shift reaches an output through the taps that land inside
the image, bias[m] = fp32(b + fp32(sum_{valid taps of m} w*t)): computed here per PIXEL from the taps' validity, not
from the nine border classes the kernels use, so a wrong class shows; store is round-to-nearest-even to the storage
type (fp32 under out_f32).  Everything is plain torch on the CPU in float64."""
from dataclasses import dataclass, replace   # replace: for the tests that vary a Geom

import torch

DTYPES = ("f32", "bf16", "f16", "f16x2", "f16p")   # f16x2: interleaved (hi, lo) pairs; f16p: 8-channel units [8 hi][8 lo]
ELEM_BYTES = {"f32": 4, "bf16": 2, "f16": 2, "f16x2": 4, "f16p": 4}
CHAN_ALIGN = {"f32": 4, "bf16": 8, "f16": 8, "f16x2": 4, "f16p": 8}   # dtype_chan_align (csrc/kernels.h)
SPLIT = ("f16x2", "f16p")
ACT_NONE, ACT_RELU, ACT_PRELU = 0, 1, 2
_FMT = {"f32": (24, -126), "bf16": (8, -126), "f16": (11, -14)}   # significand bits, exponent of the smallest normal


# ------------------------------------------------------------------------------------------------ number formats
def rne(v, bits, emin):
    """float64 -> the nearest number with `bits` significand bits, ties to even, gradual underflow below 2^emin."""
    _, e = torch.frexp(v)                      # |v| = m * 2^e, m in [0.5, 1)
    q = torch.ldexp(torch.ones_like(v), torch.clamp(e, min=emin + 1) - bits)
    return torch.round(v / q) * q              # torch.round: half to even; v / q is exact


def ulp(v, bits, emin):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), torch.clamp(e, min=emin + 1) - bits)


def split_pair(v):
    """sf16(v) of csrc/split_f16.h on the fp32 value of v: hi = rne_f16(v), lo = rne_f16(v - hi)."""
    v = rne(v, *_FMT["f32"])
    hi = rne(v, *_FMT["f16"])
    return hi, rne(v - hi, *_FMT["f16"])


def stored(v, dt):
    """The value the layout holds for v (float64 in, float64 out)."""
    if dt in SPLIT:
        hi, lo = split_pair(v)
        return hi + lo
    return rne(v, *_FMT[dt])


def encode(v, dt):
    """float64 values (..., C) -> the layout's bits: int16 (..., C) for the 2-byte types, int32 (..., C) for the rest."""
    if dt == "f32":
        return rne(v, *_FMT["f32"]).float().view(torch.int32)
    if dt == "bf16":
        return rne(v, *_FMT["bf16"]).float().to(torch.bfloat16).view(torch.int16)
    if dt == "f16":
        return rne(v, *_FMT["f16"]).float().half().view(torch.int16)
    hi, lo = (t.float().half() for t in split_pair(v))
    if dt == "f16x2":   # struct sf16 {hi, lo}: hi at the lower address
        return torch.stack([hi, lo], dim=-1).contiguous().view(torch.int32).squeeze(-1)
    lead, C = v.shape[:-1], v.shape[-1]
    assert C % 8 == 0
    return torch.stack([hi.reshape(*lead, C // 8, 8), lo.reshape(*lead, C // 8, 8)], dim=-2).contiguous().view(torch.int32).reshape(*lead, C)


def decode(raw, dt):
    """The layout's bits -> the float64 values they stand for."""
    if dt == "f32":
        return raw.view(torch.float32).double()
    if dt == "bf16":
        return raw.view(torch.bfloat16).double()
    if dt == "f16":
        return raw.view(torch.float16).double()
    lead, C = raw.shape[:-1], raw.shape[-1]
    h = raw.contiguous().view(torch.float16).double()
    if dt == "f16x2":
        return h.reshape(*lead, C, 2).sum(-1)
    return h.reshape(*lead, C // 8, 2, 8).sum(-2).reshape(*lead, C)


def raw_dtype(dt):
    return torch.int16 if ELEM_BYTES[dt] == 2 else torch.int32


def store_ulp(v, dt):
    """One unit in the last place of the storage type at v; a split pair counts as 22 bits: max(2^-21 |v|, 2^-24)."""
    if dt in SPLIT:
        return torch.clamp(v.abs() * 2.0 ** -21, min=2.0 ** -24)
    return ulp(v, *_FMT[dt])


# the planar layout as tests/test_gpu_seir.py builds it from fp32 tensors (torch's own conversions)
def _split(x):
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def to_planar(x):   # (n,H,W,C) fp32 -> the encoders' 8-channel units [8 hi][8 lo], and the values the pairs stand for
    n, H, W, C = x.shape
    hi, lo = _split(x)
    p = torch.stack([hi.view(n, H, W, C // 8, 8), lo.view(n, H, W, C // 8, 8)], dim=-2).contiguous().view(torch.int32).view(x.shape)
    return p, hi.float() + lo.float()


def from_planar(p):
    n, H, W, C = p.shape
    return p.view(torch.float16).view(n, H, W, C // 8, 2, 8).float().sum(-2).reshape(n, H, W, C)


# ------------------------------------------------------------------------------------------------ geometry
@dataclass(frozen=True)
class Geom:
    name: str
    n: int
    H: int
    W: int
    Cin: int
    Cout: int
    KH: int = 1
    KW: int = 1
    sh: int = 1
    sw: int = 1
    ph: int = 0
    pw: int = 0
    x_coff: int = 0
    ldx: int = 0                      # 0: Cin
    segs: tuple = ()                  # (c0, c1, ld, coff) per output buffer; (): one dense buffer
    res: tuple = None                 # (ld, coff) or None
    act: int = ACT_RELU
    out_f32: bool = False
    pre_bn: bool = False

    def __post_init__(self):
        if not self.ldx:
            object.__setattr__(self, "ldx", self.Cin)
        if not self.segs:
            object.__setattr__(self, "segs", ((0, self.Cout, self.Cout, 0),))

    @property
    def Ho(self):
        return (self.H + 2 * self.ph - self.KH) // self.sh + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pw - self.KW) // self.sw + 1

    @property
    def M(self):
        return self.n * self.Ho * self.Wo

    @property
    def K(self):
        return self.KH * self.KW * self.Cin


# The shape table of the sweep: each the smallest that reaches the edge it is there for.
CASES = {
    # M = 105 < BM, tiles cross image boundaries, ragged last N tile (80 under 32 / 64 / 128), one K tile below and above
    # the half-tile test of the 2-byte layouts (K = 24 < 32 < 40)
    "A": [Geom("A24", 3, 5, 7, 24, 80), Geom("A40", 3, 5, 7, 40, 80)],
    # every BN admitted; patch kernels; padding taps through the zero page; odd K-tile count; sliced input, output, residual
    "B": [Geom("B", 2, 9, 11, 16, 192, KH=3, KW=3, ph=1, pw=1, x_coff=8, ldx=32, segs=((0, 192, 256, 64),), res=(224, 16), act=ACT_PRELU)],
    # stride 2, K = 72 padded to the K tile, M = 40
    "C": [Geom("C", 2, 11, 9, 8, 32, KH=3, KW=3, sh=2, sw=2)],
    # the Block17 taps; 96-wide tiles; even K-tile count
    "D": [Geom("D1x7", 2, 5, 9, 32, 96, KH=1, KW=7, pw=3), Geom("D7x1", 2, 5, 9, 32, 192, KH=7, KW=1, ph=3)],
    # border-class bias at every class, one map without interior (2x2), one 1x1 with the table but no padding
    "E": [Geom("E2x2", 2, 2, 2, 16, 64, KH=3, KW=3, ph=1, pw=1, act=ACT_PRELU, pre_bn=True),
          Geom("E5x4", 2, 5, 4, 16, 64, KH=3, KW=3, ph=1, pw=1, act=ACT_PRELU, pre_bn=True),
          Geom("E1x1", 2, 3, 3, 16, 64, act=ACT_PRELU, pre_bn=True)],
    # IR-100 downsample: 1x1 stride 2, no activation, fp32 store path
    "F": [Geom("F", 2, 7, 7, 64, 128, sh=2, sw=2, act=ACT_NONE, out_f32=True)],
    # segment boundaries that are multiples of 8 but not of BN, differently strided buffers
    "G": [Geom("G32", 2, 6, 6, 32, 96, segs=((0, 32, 40, 8), (32, 64, 64, 16), (64, 96, 32, 0))),
          Geom("G80", 2, 6, 6, 32, 80, segs=((0, 24, 24, 0), (24, 64, 56, 8), (64, 80, 48, 32))),
          Geom("G4", 2, 6, 6, 32, 96, segs=((0, 16, 16, 0), (16, 48, 40, 8), (48, 72, 56, 24), (72, 96, 24, 0)), res=(96, 0))],
    # the 3x3-pixel tail (M = 9), long K (28 tiles of 64)
    "H": [Geom("H", 1, 3, 3, 1792, 192)],
}
# pre-BN geometries add_conv refuses: the nine-class bias table would be wrong for them
REFUSED = [Geom("Rs2", 1, 6, 6, 16, 64, KH=3, KW=3, sh=2, sw=2, ph=1, pw=1, pre_bn=True),
           Geom("RHo1", 1, 1, 4, 16, 64, KH=3, KW=3, ph=1, pw=1, pre_bn=True),
           Geom("RWo1", 1, 4, 1, 16, 64, KH=3, KW=3, ph=1, pw=1, pre_bn=True),
           Geom("Rp2", 1, 6, 6, 16, 64, KH=5, KW=5, ph=2, pw=2, pre_bn=True)]


def persistent_geom(M, Cout, with_res):
    """Case P: a 1x1 over M pixels, Cin = 64, for the tile-to-tile walk of the persistent wave-specialised kernels."""
    return Geom("P%d%s" % (Cout, "res" if with_res else ""), 1, 1, M, 64, Cout, res=(Cout, 0) if with_res else None)


# ------------------------------------------------------------------------------------------------ the formula
def im2col(x, g):
    """x (n,H,W,Cin) float64 -> A (M, K), k = (kh*KW + kw)*Cin + c, zeros at padding taps; valid (M, KH*KW)."""
    xp = torch.zeros((g.n, g.H + 2 * g.ph, g.W + 2 * g.pw, g.Cin + 1), dtype=torch.float64)
    xp[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W, :g.Cin] = x
    xp[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W, g.Cin] = 1.0    # rides along: 1 where the tap is inside the image
    taps = []
    for kh in range(g.KH):
        for kw in range(g.KW):
            taps.append(xp[:, kh:kh + g.sh * (g.Ho - 1) + 1:g.sh, kw:kw + g.sw * (g.Wo - 1) + 1:g.sw, :])
    t = torch.stack(taps, dim=3)                                   # (n, Ho, Wo, taps, Cin + 1)
    return t[..., :g.Cin].reshape(g.M, g.K).contiguous(), t[..., g.Cin].reshape(g.M, g.KH * g.KW).contiguous()


def packed_weights(w, pre_s, dt):
    """w (Cout,Cin,KH,KW) float64 of fp32 values -> (Cout, K) of the values add_conv stores: fp32(w * s), then the layout."""
    if pre_s is not None:
        w = rne(w * pre_s.view(1, -1, 1, 1), *_FMT["f32"])
    return stored(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous(), dt)


def bias_rows(w, bias, pre_t, valid):
    """(M, Cout) or (1, Cout): the bias of every output pixel, fp32 values."""
    if pre_t is None:
        return bias.view(1, -1).clone()
    T = (w * pre_t.view(1, -1, 1, 1)).sum(1).reshape(w.shape[0], -1)      # (Cout, taps): sum_c w * t
    return rne(bias.view(1, -1) + rne(valid @ T.t(), *_FMT["f32"]), *_FMT["f32"])


@dataclass
class Data:
    x: torch.Tensor                   # (n,H,W,Cin) stored values
    w: torch.Tensor                   # (Cout,Cin,KH,KW) fp32 values as handed to the library
    bias: torch.Tensor
    res: torch.Tensor = None          # (M,Cout) stored values
    slope: torch.Tensor = None
    pre_s: torch.Tensor = None
    pre_t: torch.Tensor = None
    q: int = 0                        # exact class: every term is a multiple of 2^-q
    note: str = ""


def conv_pre_store(g, dt, d):
    """act(sum + bias + res) in float64, (M, Cout), and sum_k |x*w| per output."""
    A, valid = im2col(d.x, g)
    Wm = packed_weights(d.w, d.pre_s, dt)
    v = A @ Wm.t() + bias_rows(d.w, d.bias, d.pre_t, valid)
    if d.res is not None:
        v = v + d.res
    if g.act == ACT_RELU:
        v = torch.clamp(v, min=0.0)
    elif g.act == ACT_PRELU:
        v = torch.where(v > 0, v, v * d.slope.view(1, -1))
    return v, A.abs() @ Wm.abs().t()


def out_dtype(g, dt):
    return "f32" if g.out_f32 else dt


# ------------------------------------------------------------------------------------------------ data sets
def _grid(gen, shape, step, imax):
    return torch.randint(-imax, imax + 1, shape, generator=gen).double() * step


def exact_sets(dt):
    """Names of the exact data sets of a dtype: the split layouts need two, so that the lo halves of either operand are
    not all zero while lo * lo' (which the planar kernels drop) is."""
    return ("xfine", "wfine") if dt in SPLIT else ("grid",)


EXACT_MAX_K_SPLIT = 256   # 12-bit operands leave no room for more terms inside 22 bits


def exact_data(g, dt, which, seed=0):
    """Operands on small dyadic grids: each exactly representable in the storage type, every product and every partial
    sum in any order exact in fp32 with two bits to spare.  All terms are multiples of 2^-q and
    K * max|x| * max|w'| + max|bias| + max|res| < 2^(22-q)  (exact_budget checks it on the data).

    bf16 (8 bits):    x = i/8, |i| <= 15;  w = j/8, |j| <= 7          q = 6   sums need 11+ bits: the store rounds
    f16, f32:         x = i/64, |i| <= 127;  w = j/16, |j| <= 15      q = 10  f16's 11 bits round above |v| = 2
    split, "xfine":   x = i/4096, |i| <= 4095 (12 bits: lo != 0);  w = j/8, |j| <= 3 (lo = 0)   q = 15, K <= 256
    split, "wfine":   the same with x and w swapped
    Pre-BN scales are powers of two (w' = w*s stays on a grid one bit finer: q + 1), shifts multiples of 1/8; the split
    sets then keep |j| <= 1 so that the shift's share of the bias fits the budget as well."""
    gen = torch.Generator().manual_seed(1000 + seed)
    xs, ws = (g.n, g.H, g.W, g.Cin), (g.Cout, g.Cin, g.KH, g.KW)
    if dt == "bf16":
        x, w, q = _grid(gen, xs, 1 / 8, 15), _grid(gen, ws, 1 / 8, 7), 6
        rgrid = (1 / 8, 15)
    elif dt in ("f16", "f32"):
        x, w, q = _grid(gen, xs, 1 / 64, 127), _grid(gen, ws, 1 / 16, 15), 10
        rgrid = (1 / 64, 127)
    else:
        assert g.K <= EXACT_MAX_K_SPLIT
        cj = 1 if g.pre_bn else 3
        fine, coarse = (1 / 4096, 4095), (1 / 8, cj)
        x = _grid(gen, xs, *(fine if which == "xfine" else coarse))
        w = _grid(gen, ws, *(coarse if which == "xfine" else fine))
        q, rgrid = 15, (1 / 4096, 4095)
    d = Data(x=x, w=w, bias=_grid(gen, (g.Cout,), 2.0 ** -q, 2 ** (q + 2)), q=q, note=which)
    if g.res is not None:
        d.res = _grid(gen, (g.M, g.Cout), *rgrid)
    if g.act == ACT_PRELU:   # two significant bits: v * slope stays inside fp32's 24
        d.slope = torch.tensor([0.25, 0.5, 0.375, 0.125, 0.75])[torch.randint(0, 5, (g.Cout,), generator=gen)].double()
    if g.pre_bn:
        scales = [0.5, 1.0] if dt in SPLIT else [0.5, 1.0, 2.0]
        d.pre_s = torch.tensor(scales)[torch.randint(0, len(scales), (g.Cin,), generator=gen)].double()
        d.pre_t = _grid(gen, (g.Cin,), 1 / 8, 1 if dt in SPLIT else 4)
        d.q = q + 1
    return d


def exact_budget(g, dt, d):
    """(lhs, rhs) of K * max|x| * max|w'| + max|bias[m]| + max|res| < 2^(22-q), and whether every term sits on 2^-q."""
    A, valid = im2col(d.x, g)
    Wm = packed_weights(d.w, d.pre_s, dt)
    b = bias_rows(d.w, d.bias, d.pre_t, valid)
    lhs = g.K * d.x.abs().max().item() * Wm.abs().max().item() + b.abs().max().item() + (d.res.abs().max().item() if d.res is not None else 0.0)
    unit = 2.0 ** -d.q
    on_grid = all(bool((t / unit == torch.round(t / unit)).all()) for t in (d.x, Wm, b) + ((d.res,) if d.res is not None else ()))
    return lhs, 2.0 ** (22 - d.q), on_grid


def exact_self_check(g, dt, d):
    """Rejects (AssertionError) a data set that is not exact: operands the layout cannot hold, a budget over 2^(22-q),
    or a reference sum that differs between float32 in forward k order, float32 in reversed k order and float64.
    Returns the number of expected outputs that needed rounding to the storage type."""
    od = out_dtype(g, dt)
    assert torch.equal(stored(d.x, dt), d.x), "x is not representable in " + dt
    Wm = packed_weights(d.w, d.pre_s, dt)
    wf = d.w if d.pre_s is None else d.w * d.pre_s.view(1, -1, 1, 1)
    assert torch.equal(Wm, wf.permute(0, 2, 3, 1).reshape(g.Cout, -1)), "w is not representable in " + dt
    if d.res is not None:
        assert torch.equal(stored(d.res, dt), d.res), "res is not representable in " + dt
    lhs, rhs, on_grid = exact_budget(g, dt, d)
    assert on_grid and lhs < rhs, "budget: %g !< %g (q = %d)" % (lhs, rhs, d.q)
    A, _ = im2col(d.x, g)
    a32, w32 = A.float(), Wm.float()
    fwd = torch.zeros((g.M, g.Cout), dtype=torch.float32)
    rev = torch.zeros_like(fwd)
    wt = w32.t().contiguous()
    for r0 in range(0, g.M, 256):   # row blocks that stay in the cache; every element still sees its k one by one
        f, r, a = fwd[r0:r0 + 256], rev[r0:r0 + 256], a32[r0:r0 + 256]
        p = torch.empty_like(f)
        for k in range(g.K):        # a rounded product, then a rounded sum (addcmul_ would fuse the two)
            f.add_(torch.mul(a[:, k:k + 1], wt[k:k + 1], out=p))
            r.add_(torch.mul(a[:, g.K - 1 - k:g.K - k], wt[g.K - 1 - k:g.K - k], out=p))
    s64 = A @ Wm.t()
    assert torch.equal(fwd.double(), s64) and torch.equal(rev.double(), s64), "the sum depends on its order"
    v, _ = conv_pre_store(g, dt, d)
    assert torch.equal(rne(v, *_FMT["f32"]), v), "act(sum + bias + res) is not an fp32 value"
    return int((stored(v, od) != v).sum().item())


def rounding_can_bite(g, dt):
    """Whether a 22-bit exact value can need rounding at the store at all: only into bf16 (8 bits) and f16 (11 bits).
    fp32 and a split pair (22 bits) hold every value the exact budget allows."""
    return out_dtype(g, dt) in ("bf16", "f16")


def generic_data(g, dt, seed=0):
    """Seeded normal x and w (w scaled by K^-1/2), rounded to the storage type; bias and residual N(0, 1/4)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32).double()
    d = Data(x=stored(rn(g.n, g.H, g.W, g.Cin), dt), w=rne(rn(g.Cout, g.Cin, g.KH, g.KW) * g.K ** -0.5, *_FMT["f32"]),
             bias=rne(0.5 * rn(g.Cout), *_FMT["f32"]), note="generic")
    if g.res is not None:
        d.res = stored(0.5 * rn(g.M, g.Cout), dt)
    if g.act == ACT_PRELU:
        d.slope = rne(0.1 + 0.3 * torch.rand((g.Cout,), generator=gen, dtype=torch.float32).double(), *_FMT["f32"])
    if g.pre_bn:
        d.pre_s = rne(1.0 + 0.2 * rn(g.Cin), *_FMT["f32"])
        d.pre_t = rne(0.3 * rn(g.Cin), *_FMT["f32"])
    return d


def generic_bar(g, dt, v, absum):
    """The bar of the generic class per output element: 4e-7 * sum_k |x*w| for the fp32 chain (the kernel guide's figure
    for a k-ordered fp32 chain is 0.75-1.5e-7 at K <= 1024, 3.5e-7 at K = 4096), 2^-21 * sum_k |x*w| more for the split
    layouts' 22-bit operands and the dropped lo*lo', half a unit in the last place of the storage type at the expected
    value, and one more unit where that slack straddles a rounding boundary."""
    od = out_dtype(g, dt)
    slack = 4e-7 * absum + (2.0 ** -21 * absum if dt in SPLIT else 0.0)
    u = store_ulp(v, od)
    straddle = stored(v - slack, od) != stored(v + slack, od)
    return slack + 0.5 * u + torch.where(straddle, u, torch.zeros_like(u))


def with_dtype_alignment(g, dt):
    """None when the layout's channel granularity does not allow the case's input slice."""
    a = CHAN_ALIGN[dt]
    return None if (g.Cin % a or g.x_coff % a or g.ldx % a) else g


def expected_buffers(g, dt, v, M_rows, sentinel):
    """The raw output buffers a run must leave behind: (M_rows, ld) per segment, `sentinel` bits outside the segment's
    columns and in rows >= M."""
    od = out_dtype(g, dt)
    bufs = []
    for c0, c1, ld, coff in g.segs:
        b = torch.full((M_rows, ld), sentinel, dtype=raw_dtype(od))
        b[:g.M, coff:coff + c1 - c0] = encode(v[:, c0:c1].contiguous(), od)
        bufs.append(b)
    return bufs
