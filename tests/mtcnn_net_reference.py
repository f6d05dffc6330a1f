"""Float64 restatement of R-Net (mtcnn.py:84-99) and O-Net (mtcnn.py:138-157) LAYER BY LAYER, on stored values, for
the staged-parity hook MTCNN.debug_net / debug_net_tap (tests/test_gpu_mtcnn_nets.py; checked on the host by
tests/test_mtcnn_net_reference_host.py), and the frames and rectangles both tests run on.

A layer's input is the previous layer's buffer exactly as the device returned it (decoded); its output here is the
expected value v, the per-element absolute sum A = sum_k |x*w| + |bias| and the slack the arithmetic may use:

    slack = (K + 2) * 2^-24 * A * max(1, |slope_c|)  [+ 2^-21 * A * max(1, |slope_c|) in the split-f16 forms]
    bar   = slack + 1/2 ulp_store(v) + (one ulp_store more where v -+ slack straddles a store rounding boundary)

The first term is the forward bound of an fp32 sum of K products plus a bias in ANY order, with or without FMA
(gamma_(K+1) ~ (K+1) u on the sum, one more rounding for the PReLU product, which also scales the sum's error by
|slope|): a correct kernel cannot exceed it.  The split term (22-bit operands, dropped lo*lo') and the store terms are
conv_reference.generic_bar's.  A max pool moves values: a pooled element's slack is the largest slack in its window
(|max a - max b| <= max |a - b|), and a pool that reads a stored buffer is exact.  The project's tighter figure,
4e-7 * A (FIG), is reported, never asserted: torch's own fp32 convolution exceeds it on conv2 of both nets.

Operands: in the split forms the values the layout holds -- stored(w, "f16x2"), the decoded activations, and for the
front kernel, which splits the crop itself, stored(crop, "f16x2"); in the f32 form the fp32 values.  Bias and PReLU
slopes are fp32 in every form.  Everything is plain torch on the CPU in float64, NHWC."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from conv_reference import decode, store_ulp, stored

FORMS = ("mid", "split", "f32")      # default (split-f16 + fused conv2 / pool2 kernel), VNF_MTCNN_MID=0, VNF_MTCNN_DTYPE=f32
FORM_ENV = {"mid": {}, "split": {"VNF_MTCNN_MID": "0"}, "f32": {"VNF_MTCNN_DTYPE": "f32"}}
S_OF = {2: 24, 3: 48}
NF_OF = {2: 5, 3: 15}
DERIVED, FIG = 2.0 ** -24, 4e-7      # per-product coefficient of the gate (times K + 2) / the project's flat figure
SPLIT_TERM = 2.0 ** -21


def is_split(form):
    return form != "f32"


def store_dtype(form):
    return "f16x2" if is_split(form) else "f32"


# ------------------------------------------------------------------------------------------------ layers
@dataclass
class Layer:
    name: str                 # the tap that holds the layer's output
    src: str                  # the tap it reads
    kind: str                 # "conv" | "pool" | "dense" | "heads"
    w: torch.Tensor = None    # conv (Cout,Cin,KH,KW); dense / heads (Cout, features); fp32 values in float64
    b: torch.Tensor = None
    slope: torch.Tensor = None
    pool: int = 0             # max_pool2d(pool, 2, ceil_mode=True): behind the convolution (fused kernels), or the layer itself
    cpad: int = 0             # channels of the buffer (the rest are zero): R-Net pool1 28 -> 32, heads 6 -> 8
    pieces: tuple = ()        # heads: widths of the concatenated pieces

    @property
    def K(self):
        return int(self.w[0].numel())


def _d(sd, k):
    return sd[k].detach().double()


def _conv(sd, i, name, src, pool=0, cpad=0):
    return Layer(name, src, "conv", _d(sd, "conv%d.weight" % i), _d(sd, "conv%d.bias" % i), _d(sd, "prelu%d.weight" % i), pool, cpad)


def _dense(sd, i):
    return Layer("dense", "conv%d" % (i - 1), "dense", _d(sd, "dense%d.weight" % i), _d(sd, "dense%d.bias" % i), _d(sd, "prelu%d.weight" % i))


def _heads(sd, i, n, cpad):
    names = ["dense%d_%d" % (i, j + 1) for j in range(n)]
    return Layer("heads", "dense", "heads", torch.cat([_d(sd, h + ".weight") for h in names]), torch.cat([_d(sd, h + ".bias") for h in names]),
                 None, 0, cpad, tuple(int(sd[h + ".bias"].numel()) for h in names))


def layers(net, sd, form):
    """The layers of a net in plan order for a handle form; `sd` the net's state dict."""
    out = [_conv(sd, 1, "pool1", "crops", pool=3, cpad=32)]
    if form == "mid":
        out.append(_conv(sd, 2, "pool2", "pool1", pool=3))
    else:
        out += [_conv(sd, 2, "conv2", "pool1"), Layer("pool2", "conv2", "pool", pool=3)]
    out.append(_conv(sd, 3, "conv3", "pool2"))
    if net == 2:
        return out + [_dense(sd, 4), _heads(sd, 5, 2, 8)]
    return out + [Layer("pool3", "conv3", "pool", pool=2), _conv(sd, 4, "conv4", "pool3"), _dense(sd, 5), _heads(sd, 6, 3, 16)]


def tap_names(net, form):
    """Every buffer the builders create, and whether the form writes it."""
    names = ["crops", "pool1", "conv2", "pool2", "conv3"] + (["pool3", "conv4"] if net == 3 else []) + ["dense", "heads"]
    return [(n, not (form == "mid" and n == "conv2")) for n in names]


# ------------------------------------------------------------------------------------------------ one function per layer kind
def max_pool(x, k):
    """max_pool2d(k, 2, ceil_mode=True) on NHWC."""
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()


def prelu(v, slope):
    return v if slope is None else torch.where(v > 0, v, v * slope)


def conv_prelu(x, w, b, slope):
    """conv2d + bias + PReLU on NHWC x (the first w.shape[1] channels): (v, A), A = sum_k |x*w| + |bias|."""
    xc = x[..., :w.shape[1]].permute(0, 3, 1, 2)
    v = F.conv2d(xc, w, b).permute(0, 2, 3, 1)
    A = F.conv2d(xc.abs(), w.abs(), b.abs()).permute(0, 2, 3, 1)
    return prelu(v, slope).contiguous(), A.contiguous()


def flatten_whc(x):
    """x.permute(0,3,2,1) of the reference's NCHW tensor, flattened: feature (w*H + h)*C + c of NHWC x."""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], -1)


def dense_prelu(x, w, b, slope):
    f = flatten_whc(x)
    n = x.shape[0]
    return prelu(f @ w.t() + b, slope).view(n, 1, 1, -1), (f.abs() @ w.abs().t() + b.abs()).view(n, 1, 1, -1)


def heads(x, w, b):
    """The head pieces side by side (class scores, box regression, landmarks), no activation."""
    return dense_prelu(x, w, b, None)


def softmax1(h):
    """softmax over the two class scores, column 1: the table's probability."""
    return torch.softmax(h.reshape(h.shape[0], -1)[:, :2], dim=1)[:, 1]


def _pad_c(t, c):
    return t if c <= t.shape[-1] else F.pad(t, (0, c - t.shape[-1]))


def operands(layer, x, form):
    """(x, w) as the kernels' arithmetic sees them."""
    if not is_split(form):
        return x, layer.w
    return (stored(x, "f16x2") if layer.src == "crops" else x), stored(layer.w, "f16x2")


def expected(layer, x, form):
    """x: the decoded src tap (n,H,W,C).  Returns (v, A, unit): v the expected value of every element of the layer's
    tap before the store, A its absolute sum and unit = A * max(1, |slope_c|), pooled where the layer pools (the
    slack is a coefficient times unit); A and unit are None for a pool of a stored buffer, which is exact."""
    if layer.kind == "pool":
        return max_pool(x, layer.pool), None, None
    xo, w = operands(layer, x, form)
    if layer.kind == "conv":
        v, A = conv_prelu(xo, w, layer.b, layer.slope)
    elif layer.kind == "dense":
        v, A = dense_prelu(xo, w, layer.b, layer.slope)
    else:
        v, A = heads(xo, w, layer.b)
    unit = A if layer.slope is None else A * torch.clamp(layer.slope.abs(), min=1.0)
    if layer.pool:
        v, A, unit = max_pool(v, layer.pool), max_pool(A, layer.pool), max_pool(unit, layer.pool)
    return _pad_c(v, layer.cpad), _pad_c(A, layer.cpad), _pad_c(unit, layer.cpad)


def slack_of(layer, unit, form, coeff=None):
    """coeff None: the derived gate (K + 2) * 2^-24; FIG: the project's 4e-7."""
    c = (layer.K + 2) * DERIVED if coeff is None else coeff
    return (c + (SPLIT_TERM if is_split(form) else 0.0)) * unit


def bar(v, slack, form):
    """slack + the two store terms of conv_reference.generic_bar."""
    od = store_dtype(form)
    u = store_ulp(v, od)
    straddle = stored(v - slack, od) != stored(v + slack, od)
    return slack + 0.5 * u + torch.where(straddle, u, torch.zeros_like(u))


def check_layer(layer, x, got, form):
    """got: the decoded tap.  Returns (ok mask, figures): figures = (largest |got - ref| / A over elements with A > 0,
    largest |got - ref| / bar, largest |got - ref| / the 4e-7 bar); a pool of a stored buffer must be exact."""
    v, A, unit = expected(layer, x, form)
    assert got.shape == v.shape, (layer.name, tuple(got.shape), tuple(v.shape))
    err = (got - v).abs()
    if A is None:
        return err == 0, (0.0, float(err.max() > 0), float(err.max() > 0))
    gate, fig = bar(v, slack_of(layer, unit, form), form), bar(v, slack_of(layer, unit, form, FIG), form)
    pos = A > 0
    rel = float((err[pos] / A[pos]).max()) if bool(pos.any()) else 0.0
    return err <= gate, (rel, float((err / gate).max()), float((err / fig).max()))


def decode_tap(raw, split):
    """The hook's raw int32 words (n,H,W,C) -> float64 values."""
    return decode(torch.from_numpy(np.ascontiguousarray(raw)), "f16x2" if split else "f32")


# ------------------------------------------------------------------------------------------------ inputs
SIZES = ((240, 320), (233, 317))     # rows of 960 B at an aligned address: the strips; 951 B: the per-pixel gather


def frames(H, W):
    """(2,H,W,3) u8: the picture cut to H x W, and its mirror image."""
    from conftest import load_image
    img = load_image("mrDam_HaHo_recog.jpg")[:H, :W]
    return np.ascontiguousarray(np.stack([img, img[:, ::-1]]))


def rectangles(H, W):
    """(n,4) int32 y, ey, x, ex (1-based, inclusive, as pad() returns them), all distinct and valid under the reference's
    own condition.  With S = 24 | 48: squares that up-sample (12, 23 / 47), are the identity (24 / 48), sit just above
    (25 / 49) or at non-integer ratios (96 at 48 is 2, 150 is not); degenerate-thin ones; every border; the whole frame
    (60 chunks of 16 B at W = 320: the wide branch of the crop kernel); and widths whose byte span [3 x0, 3 (x0 + w))
    from x0 = 11 (3 x0 % 16 = 1: a non-zero offset into the first chunk) covers 1, 2, 32 and 33 chunks -- the
    rows-per-wave R = 64 / nch at both ends."""
    r = [(3 + 7 * i, 3 + 7 * i + s - 1, 2 + 13 * i, 2 + 13 * i + s - 1) for i, s in enumerate((12, 23, 24, 25, 47, 48, 49, 96, 150))]
    r += [(100, 100, 200, 200), (50, 50, 30, 69), (120, 121, 10, 12), (10, 19, 200, 299), (30, 129, 150, 159)]
    r += [(1, 30, 100, 140), (H - 40, H, 50, 95), (60, 110, 1, 33), (70, 120, W - 45, W), (H - 20, H, W - 25, W), (1, 20, 1, 20)]
    r += [(1, H, 1, W)]
    r += [(20, 79, 12, 11 + w) for w in (5, 6, 170, 171)]
    r = np.asarray(r, dtype=np.int32)
    assert len(set(map(tuple, r.tolist()))) == len(r)
    assert (r[:, 0] >= 1).all() and (r[:, 1] <= H).all() and (r[:, 2] >= 1).all() and (r[:, 3] <= W).all()
    assert (r[:, 1] > r[:, 0] - 1).all() and (r[:, 3] > r[:, 2] - 1).all()
    return r


def chunk_count(x, ex):
    """nch of crop_resize_rows_kernel for the columns x..ex (1-based, inclusive), and the offset into the first chunk."""
    bs, be = (x - 1) * 3, ex * 3
    return ((be + 15) >> 4) - (bs >> 4), bs & 15


def oracle_crops(fr, frame_idx, rects, S):
    """om._crops on frames (b,H,W,3) u8: (n,S,S,3) fp32 NHWC, normalised."""
    from oracle import mtcnn as om
    x = torch.from_numpy(fr.copy()).permute(0, 3, 1, 2).float()
    c = om._crops(x, frame_idx, rects[:, 0], rects[:, 1], rects[:, 2], rects[:, 3], S)
    return c.permute(0, 2, 3, 1).contiguous()
