"""An exact-arithmetic InceptionResnetV1: a state dict and images on which every convolution from conv2d_1a to repeat_2 is
exact in fp32, and a float64 restatement of that path with the kernels' documented rounding points.  The exact class of
tests/conv_reference.py, extended from one convolution to the network: operands sit on small dyadic grids, so every
partial sum, in any order and on any MFMA shape, is exact in fp32; the value in front of every store is unique and its
16-bit rounding deterministic -- the bits of every tap are known without a tolerance, independently of the plan, of the
oracle's fp32 order and of any recorded output.  Host only: checked by tests/test_exact_net_host.py, used on the GPU by
tests/test_gpu_trunk17_exact.py.

The network
  * every BatchNorm folds (bn_fold, csrc/plan.cpp, restated here) to scale exactly 1.0f and shift exactly the bias:
    weight 1, running_mean 0, running_var float32(0.999) with eps 1e-3f;
  * every BasicConv2d on the path has weights in {0, +-1}, a few per output row, positions and signs seeded;
  * the five Block35 and the Block17 outside the live set L have an all-zero up-projection with zero bias (their branch
    convolutions are zeroed too, so nothing they compute can leave the 16-bit range): the trunk behind conv2d_4b /
    mixed_6a is post-ReLU, so such a block is the identity on the fp32 trunk and on its 16-bit store;
  * a live Block17 has 8 weights per row in reduce / 1x7 / 7x1 (every k position of each is used by some row) and an
    up-projection weight = 10 g, bias = 10 h with g in {+-1, +-1/2}, h on the input grid: the plan folds the residual
    scale 0.10f on the host, and fl32(10 g * 0.1f) == g;
  * the biases of a live block's reduce / 1x7 / 7x1 are calibrated on the case's own images: minus a quantile of the
    channel's sums (an integer) plus a seeded i * step, 1 <= i <= 15.  Most outputs then end at zero behind the ReLU, the next
    convolution sums one or two non-zero terms instead of eight, and the gain of a block stays near 1 -- what lets a
    run of live blocks stay inside the budget.  A calibration is part of the generator, not of the check: whatever it
    produces has to pass self-check and the rounding shares, or the case is rejected.

The budget rule, per convolution: all terms on a common grid 2^-q, and max(sum_k |x*w| + |bias| + |residual|) < 2^(22-q)
-- fp32's 24 bits less the two spare bits tests/conv_reference.py keeps.

Storage types: "bf16", "f16" and "f16x2" (the encoders' planar split-f16; a pair holds every value the budget allows,
so there stored(v) == v is asserted and nothing rounds)."""
from dataclasses import dataclass, field, replace

import numpy as np
import torch
import torch.nn.functional as F

from conv_reference import SPLIT, _FMT, rne, stored

DTYPES = ("bf16", "f16", "f16x2")
TAPS = ("conv2d_1a", "conv2d_3b", "conv2d_4b", "repeat_1", "mixed_6a", "repeat_2")
BN_EPS = np.float32(1e-3)
RES_SCALE17 = np.float32(0.10)
F16_MAX = 65504.0
# name, cin, cout, (kh, kw), stride, (ph, pw) of every BasicConv2d in front of repeat_2
STEM = (("conv2d_1a", 3, 32, (3, 3), 2, (0, 0)), ("conv2d_2a", 32, 32, (3, 3), 1, (0, 0)), ("conv2d_2b", 32, 64, (3, 3), 1, (1, 1)),
        ("conv2d_3b", 64, 80, (1, 1), 1, (0, 0)), ("conv2d_4a", 80, 192, (3, 3), 1, (0, 0)), ("conv2d_4b", 192, 256, (3, 3), 2, (0, 0)))
MIXED_6A = (("mixed_6a.branch0", 256, 384, (3, 3), 2, (0, 0)), ("mixed_6a.branch1.0", 256, 192, (1, 1), 1, (0, 0)),
            ("mixed_6a.branch1.1", 192, 192, (3, 3), 1, (1, 1)), ("mixed_6a.branch1.2", 192, 256, (3, 3), 2, (0, 0)))
BLOCK17 = (("branch0", 896, 128, (1, 1), (0, 0)), ("branch1.0", 896, 128, (1, 1), (0, 0)),
           ("branch1.1", 128, 128, (1, 7), (0, 3)), ("branch1.2", 128, 128, (7, 1), (3, 0)))
BLOCK35 = ("branch0", "branch1.0", "branch1.1", "branch2.0", "branch2.1", "branch2.2")
MUTATIONS = ("tap_1x7_left", "tap_7x1_bottom", "swap_reduce_channels", "next_block_kstep", "bias_shifted", "round_trunk", "truncate_7x1")


@dataclass(frozen=True)
class Settings:
    """What the generator may vary per storage type (the values in use: SETTINGS)."""
    in_step: float          # images = i * in_step, |i| <= in_max; the biases of the stem sit on the same grid
    in_max: int
    stem_nz: int            # non-zero weights per output row in front of repeat_2
    live_nz: int = 8        # ... in a live block's reduce / 1x7 / 7x1 (>= 7: every k of a 128 x 896 matrix used)
    up_nz: int = 1          # ... in a live block's up-projection
    up_g: tuple = (1.0, 0.5)    # |g| of the up-projection weights
    quantile: tuple = (0.8, 0.85, 0.85)   # of the sums of reduce / 1x7 / 7x1 that the calibrated bias moves to zero


# bf16 rounds above 8 bits, f16 above 11: the f16 images are three bits finer, so that with the same weights the same
# share of a live block's values (1.5 % and more of every stored tensor) needs rounding.  Four weights per row in front of repeat_2 bring mixed_6a
# to ~2^11 (bf16) / 2^14 (f16) grid units.
SETTINGS = {"bf16": Settings(1 / 8, 15, 4), "f16": Settings(1 / 64, 127, 4), "f16x2": Settings(1 / 64, 127, 4)}
# A |g| of 1/2 makes the trunk's grid one bit finer per live block, which the budget pays for: runs of more than two live
# blocks keep |g| = 1, and with it all ten blocks pass the self-check in every storage type (largest budget use: bf16
# 0.03, f16 0.26, f16x2 0.28).
LONG_UP_G = (1.0,)
LONGEST = tuple(range(10))


# ------------------------------------------------------------------------------------------------ host folding, restated
def bn_fold(g, b, m, v, eps=BN_EPS):
    """bn_fold of csrc/plan.cpp: float32 tensors in, the fold in double, float32 (scale, shift) out."""
    g, b, m, v = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (g, b, m, v))
    sc = g / np.sqrt(v + np.float64(np.float32(eps)))
    return sc.astype(np.float32), (b - m * sc).astype(np.float32)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).double()


def basic_params(sd, p, dt):
    """BasicConv2d p as add_conv packs it: stored(fl32(w * scale)) and the fp32 bias, float64 tensors."""
    s, t = bn_fold(sd[p + ".bn.weight"], sd[p + ".bn.bias"], sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"])
    w = np.asarray(sd[p + ".conv.weight"], dtype=np.float32) * s.reshape(-1, 1, 1, 1)     # float32 product, as wv * sc
    return stored(_t64(w), dt), _t64(t)


def up_params(sd, p, scale, dt):
    """A block's up-projection as plan_irv1.cpp folds the residual scale: stored(fl32(w * scale)), fl32(bias * scale)."""
    w = np.asarray(sd[p + ".conv2d.weight"], dtype=np.float32) * np.float32(scale)
    b = np.asarray(sd[p + ".conv2d.bias"], dtype=np.float32) * np.float32(scale)
    return stored(_t64(w), dt), _t64(b)


# ------------------------------------------------------------------------------------------------ one convolution
def grid_q(*ts):
    """The smallest q >= 0 with every value of every tensor a multiple of 2^-q."""
    q = 0
    for t in ts:
        t = t[t != 0]
        while t.numel() and not bool((t * 2.0 ** q == torch.round(t * 2.0 ** q)).all()):
            q += 1
            assert q <= 60
    return q


def truncated(v, dt):
    """Round towards zero to the storage type (the mutation of a store that truncates); bf16 / f16, normal range."""
    bits = _FMT[dt][0]
    _, e = torch.frexp(v)
    u = torch.ldexp(torch.ones_like(v), e - bits)
    return torch.trunc(v / u) * u


@dataclass
class Rec:
    """What one convolution of the restatement reports."""
    name: str
    q: int                  # common grid of its terms
    use: float              # max(sum |x*w| + |bias| + |res|) / 2^(22 - q)
    sum_max: float          # the numerator, in grid units
    rounded: float          # share of outputs whose exact value the storage type cannot hold (0 where nothing is stored)
    nonzero: float          # share of non-zero outputs
    dead: int = 0           # output channels that are zero at every pixel of every image


def _order_check(x, W, stride, pad, s64):
    """The float32 sum in forward k order and in reversed k order, a rounded product and a rounded sum per k, equals the
    float64 sum.  k positions whose weight is zero in every row are passed over: they add +-0 to every element."""
    Cout, K = W.shape[0], W[0].numel()
    A = F.unfold(x.float(), W.shape[2:], padding=pad, stride=stride).permute(0, 2, 1).reshape(-1, K).contiguous()
    Wt = W.float().reshape(Cout, K).t().contiguous()
    want = s64.permute(0, 2, 3, 1).reshape(-1, Cout)
    ks = [int(k) for k in torch.nonzero(Wt.abs().sum(1)).flatten()]
    for r0 in range(0, A.shape[0], 2048):
        a = A[r0:r0 + 2048]
        fwd = torch.zeros((a.shape[0], Cout), dtype=torch.float32)
        rev = torch.zeros_like(fwd)
        p = torch.empty_like(fwd)
        for i in range(len(ks)):
            kf, kr = ks[i], ks[len(ks) - 1 - i]
            fwd.add_(torch.mul(a[:, kf:kf + 1], Wt[kf:kf + 1], out=p))
            rev.add_(torch.mul(a[:, kr:kr + 1], Wt[kr:kr + 1], out=p))
        w = want[r0:r0 + 2048]
        assert torch.equal(fwd.double(), w) and torch.equal(rev.double(), w), "the sum depends on its order"


def conv_layer(name, x, W, b, dt, stride=1, pad=(0, 0), res=None, store=True, log=None, check=False, sums_only=False,
               bias_roll=0, sub=None, trunc=False):
    """store(relu(conv(x, W) + b + res)) on float64 NCHW tensors of stored values; res (the fp32 trunk) is not rounded.
    log: a list that receives the convolution's Rec.  check: the self-check of this convolution (AssertionError).
    The keyword arguments behind sums_only exist for the mutations of the host test."""
    s = F.conv2d(x, W, None, stride, pad)
    if sums_only:
        return s
    if sub is not None:
        s = s - sub
    if bias_roll:
        b = torch.roll(b, bias_roll)
    v = s + b.view(1, -1, 1, 1)
    if res is not None:
        v = v + res
    v = torch.clamp(v, min=0.0) + 0.0      # + 0.0: a zero is +0, as every sum that starts from a +0 or a bias is
    out = (truncated(v, dt) if trunc else stored(v, dt)) if store else v
    if log is not None or check:
        terms = [b] + ([res] if res is not None else [])
        q = max(grid_q(x) + grid_q(W), grid_q(*terms))
        tot = F.conv2d(x.abs(), W.abs(), None, stride, pad) + b.abs().view(1, -1, 1, 1) + (res.abs() if res is not None else 0.0)
        top = tot.max().item() * 2.0 ** q
        rec = Rec(name, q, top / 2.0 ** 22, top, float((out != v).double().mean()) if store else 0.0, float((v != 0).double().mean()),
                  int((v.abs().amax(dim=(0, 2, 3)) == 0).sum()))
        if log is not None:
            log.append(rec)
        if check:
            assert torch.equal(stored(x, dt), x), name + ": x is not representable in " + dt
            assert torch.equal(stored(W, dt), W), name + ": w is not representable in " + dt
            assert rec.use < 1.0, "%s: budget %g !< 2^(22-%d)" % (name, top * 2.0 ** -q, q)
            _order_check(x, W, stride, pad, s)
            assert torch.equal(rne(v, *_FMT["f32"]), v), name + ": relu(sum + bias + res) is not an fp32 value"
            assert out.abs().max().item() < F16_MAX and v.abs().max().item() < F16_MAX, name + ": a value reaches 65504"
            if dt in SPLIT:
                assert torch.equal(out, v), name + ": a split pair does not hold the exact value"
    return out


# ------------------------------------------------------------------------------------------------ the restatement
def _is_identity(sd, p):
    return not np.any(np.asarray(sd[p + ".conv2d.weight"])) and not np.any(np.asarray(sd[p + ".conv2d.bias"]))


def live_set(sd):
    return tuple(k for k in range(10) if not _is_identity(sd, "repeat_2.%d" % k))


def upstream(sd, x, dt, log=None, check=False):
    """conv2d_1a ... mixed_6a on images x (n,3,160,160), float64 on the input grid.  conv2d_1a (aux_kernels.hip) reads
    the caller's fp32 pixels against fp32 weights; everything behind it reads stored values against stored weights."""
    taps = {}
    h = x
    for name, _, _, _, stride, pad in STEM:
        W, b = basic_params(sd, name, "f32" if name == "conv2d_1a" else dt)
        first = name == "conv2d_1a"
        if first and check:
            assert torch.equal(rne(x, *_FMT["f32"]), x)
        h = conv_layer(name, h, W, b, dt, stride, pad, log=log, check=check and not first)
        if first and check:   # the operands are fp32 here, not the storage type: the rest of the self-check by hand
            assert log is None or log[-1].use < 1.0
            _order_check(x, W, stride, pad, F.conv2d(x, W, None, stride, pad))
        if name == "conv2d_2b":
            h = F.max_pool2d(h, 3, 2)
        taps[name] = h
    for i in range(5):   # Block35 with a zero up-projection: relu(x + 0) of a stored, non-negative x
        assert _is_identity(sd, "repeat_1.%d" % i), "the exact network keeps every Block35 an identity"
    assert bool((h >= 0).all()) and torch.equal(stored(h, dt), h)
    taps["repeat_1"] = h
    prm = {name: basic_params(sd, name, dt) for name, *_ in MIXED_6A}
    kw = dict(log=log, check=check)
    b0 = conv_layer("mixed_6a.branch0", h, *prm["mixed_6a.branch0"], dt, 2, (0, 0), **kw)
    b1 = conv_layer("mixed_6a.branch1.0", h, *prm["mixed_6a.branch1.0"], dt, 1, (0, 0), **kw)
    b1 = conv_layer("mixed_6a.branch1.1", b1, *prm["mixed_6a.branch1.1"], dt, 1, (1, 1), **kw)
    b1 = conv_layer("mixed_6a.branch1.2", b1, *prm["mixed_6a.branch1.2"], dt, 2, (0, 0), **kw)
    taps["mixed_6a"] = torch.cat((b0, b1, F.max_pool2d(h, 3, 2)), 1)
    return {k: taps[k] for k in TAPS if k in taps}


def block17_params(sd, k, dt):
    p = "repeat_2.%d" % k
    prm = {name: basic_params(sd, p + "." + name, dt) for name, *_ in BLOCK17}
    prm["up"] = up_params(sd, p, RES_SCALE17, dt)
    return prm


def block17(prm, trunk, dt, tag, log=None, check=False, mut=None, nxt=None):
    """One live Block17 on the fp32 trunk (float64 tensor of fp32 values) -> the next fp32 trunk, unrounded.
    trunk17.hip / trunk17s.hip: the reduce convolution reads the 16-bit copy of the trunk; branch0 | branch1.0, the 1x7
    and the 7x1 outputs are stored in the 16-bit type (LDS); the up-projection accumulates onto the fp32 trunk, the
    (scaled) bias is added and the ReLU applied in fp32.  mut: one of MUTATIONS (nxt: the next block's parameters)."""
    kw = dict(log=log, check=check)
    xb = stored(trunk, dt)
    (W0, b0), (W1, b1) = prm["branch0"], prm["branch1.0"]   # one GEMM in the kernels: rows 0..127 | 128..255
    if mut == "next_block_kstep":   # one 32-deep k-step (channels 416..447) of the reduce weights from the block behind
        W0, W1 = W0.clone(), W1.clone()
        W0[:, 416:448], W1[:, 416:448] = nxt["branch0"][0][:, 416:448], nxt["branch1.0"][0][:, 416:448]
    c0 = conv_layer(tag + ".branch0", xb, W0, b0, dt, **kw)
    t0 = conv_layer(tag + ".branch1.0", xb, W1, b1, dt, **kw)
    if mut == "swap_reduce_channels":   # channels 2 and 9 of wave 3's tile of the branch0 half, 5 and 12 of its branch1.0 tile
        i0, i1 = torch.arange(128), torch.arange(128)
        i0[[50, 57]] = torch.tensor([57, 50])
        i1[[53, 60]] = torch.tensor([60, 53])
        c0, t0 = c0[:, i0], t0[:, i1]
    W17, b17 = prm["branch1.1"]
    W71, b71 = prm["branch1.2"]
    sub = None
    if mut == "tap_1x7_left":   # output column 0 loses its outermost tap inside the image: kw = 6, input column 3
        sub = torch.zeros((t0.shape[0], 128, 8, 8), dtype=torch.float64)
        sub[:, :, :, 0] = torch.einsum("nchw,oc->nohw", t0[:, :, :, 3:4], W17[:, :, 0, 6])[:, :, :, 0]
    t1 = conv_layer(tag + ".1x7", t0, W17, b17, dt, 1, (0, 3), sub=sub, bias_roll=1 if mut == "bias_shifted" else 0, **kw)
    sub = None
    if mut == "tap_7x1_bottom":   # output row 7 loses its outermost tap inside the image: kh = 0, input row 4
        sub = torch.zeros((t1.shape[0], 128, 8, 8), dtype=torch.float64)
        sub[:, :, 7, :] = torch.einsum("nchw,oc->nohw", t1[:, :, 4:5, :], W71[:, :, 0, 0])[:, :, 0, :]
    t2 = conv_layer(tag + ".7x1", t1, W71, b71, dt, 1, (3, 0), sub=sub, trunc=mut == "truncate_7x1", **kw)
    cat = torch.cat((c0, t2), 1)
    return conv_layer(tag + ".up", cat, *prm["up"], dt, res=trunk, store=False, **kw)


def repeat_2(sd, m6a, dt, carry="fp32", log=None, check=False, mut=None, mut_block=None):
    """mixed_6a (stored values) -> the repeat_2 tap.  carry "fp32": the persistent kernels -- the trunk stays unrounded
    across the blocks, one rounding at the final store; "stored": the per-convolution plan rounds it after every block.
    A block with a zero up-projection is relu(trunk + 0): the identity on a non-negative trunk in either mode.
    mut / mut_block: apply one of MUTATIONS at live block mut_block (default: the first live one)."""
    assert carry in ("fp32", "stored")
    live = live_set(sd)
    assert bool((m6a >= 0).all())
    trunk = m6a
    if mut is not None and mut_block is None:
        mut_block = live[0]
    for k in live:
        prm = block17_params(sd, k, dt)
        here = mut if k == mut_block else None
        nxt = block17_params(sd, (k + 1) % 10, dt) if here == "next_block_kstep" else None
        trunk = block17(prm, trunk, dt, "repeat_2.%d" % k, log=log, check=check,
                        mut=None if here == "round_trunk" else here, nxt=nxt)
        if carry == "stored" or here == "round_trunk":
            trunk = stored(trunk, dt)
    out = stored(trunk, dt)
    if log is not None:
        log.append(Rec("repeat_2.store", 0, 0.0, 0.0, float((out != trunk).double().mean()), float((out != 0).double().mean())))
    if check:
        assert out.abs().max().item() < F16_MAX
        if dt in SPLIT:
            assert torch.equal(out, trunk), "repeat_2: a split pair does not hold the exact trunk"
    return out


# ------------------------------------------------------------------------------------------------ the generator
def _sparse(gen, cout, cin, kh, kw, nz, cover=False):
    """(cout, cin, kh, kw) float32 in {0, +-1}: nz positions per row from consecutive seeded permutations of the K
    positions (so that every position is used once before any is used twice), seeded signs.  cover: assert that every
    k position is used by some row and that no row lost a weight to a repeated position."""
    K = cin * kh * kw
    need = cout * nz
    pos = torch.cat([torch.randperm(K, generator=gen) for _ in range((need + K - 1) // K)])[:need].reshape(cout, nz)
    sign = (torch.randint(0, 2, (cout, nz), generator=gen) * 2 - 1).float()
    w = torch.zeros((cout, K), dtype=torch.float32)
    w.scatter_(1, pos, sign)
    if cover:
        assert bool((w != 0).any(0).all()), "a k position is used by no output row"
        assert bool(((w != 0).sum(1) == nz).all()), "a row repeats a position"
    return w.reshape(cout, cin, kh, kw).numpy()


def _set_bn(sd, p, bias):
    c = len(bias)
    sd[p + ".bn.weight"] = np.ones(c, np.float32)
    sd[p + ".bn.running_mean"] = np.zeros(c, np.float32)
    sd[p + ".bn.running_var"] = np.full(c, 0.999, np.float32)
    sd[p + ".bn.bias"] = np.asarray(bias, dtype=np.float32)
    s, t = bn_fold(sd[p + ".bn.weight"], sd[p + ".bn.bias"], sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"])
    assert np.all(s == np.float32(1.0)) and np.array_equal(t, sd[p + ".bn.bias"]), p + ": the BatchNorm does not fold to (1, bias)"


def _grid_bias(gen, c, step, imax):
    return (torch.randint(-imax, imax + 1, (c,), generator=gen).double() * step).numpy().astype(np.float32)


def _zero_block(sd, p, branches):
    """An identity block: zero up-projection and bias; the branch convolutions zeroed and folded to (1, 0) as well."""
    for b in branches:
        sd[p + "." + b + ".conv.weight"] = np.zeros_like(np.asarray(sd[p + "." + b + ".conv.weight"], dtype=np.float32))
        _set_bn(sd, p + "." + b, np.zeros(sd[p + "." + b + ".conv.weight"].shape[0], np.float32))
    sd[p + ".conv2d.weight"] = np.zeros_like(np.asarray(sd[p + ".conv2d.weight"], dtype=np.float32))
    sd[p + ".conv2d.bias"] = np.zeros_like(np.asarray(sd[p + ".conv2d.bias"], dtype=np.float32))


def images(dt, n, seed=0):
    """(n, 3, 160, 160) float64 on the input grid of the storage type; image i does not depend on n."""
    st = SETTINGS[dt]
    gen = torch.Generator().manual_seed(4000 + seed)
    return torch.randint(-st.in_max, st.in_max + 1, (8, 3, 160, 160), generator=gen)[:n].double() * st.in_step


_base = {}


def base_state_dict(dt, seed=0):
    """The state dict with no live Block17: generate_state_dict("irv1", 0) with every tensor on the path to repeat_2
    overwritten (a fresh copy of the dict; the arrays are shared and never written)."""
    key = (dt, seed)
    if key not in _base:
        from vn_celeb_face_recognition_amd.weights import generate_state_dict
        st = SETTINGS[dt]
        sd = dict(generate_state_dict("irv1", 0))
        gen = torch.Generator().manual_seed(5000 + seed)
        for name, cin, cout, (kh, kw), _, _ in STEM + MIXED_6A:
            sd[name + ".conv.weight"] = _sparse(gen, cout, cin, kh, kw, st.stem_nz)
            _set_bn(sd, name, _grid_bias(gen, cout, st.in_step, st.in_max // 2))
        for i in range(5):
            _zero_block(sd, "repeat_1.%d" % i, BLOCK35)
        for k in range(10):
            _zero_block(sd, "repeat_2.%d" % k, [b for b, *_ in BLOCK17])
        _base[key] = sd
    return dict(_base[key])


def _calibrated(gen, sums, quantile, step):
    """Per-channel bias: minus the (integer part of the) quantile of the channel's sums over the case's images and
    pixels, plus a seeded i * step, 1 <= i <= 15: the tenth of a channel's outputs at or above the quantile stays positive,
    so no channel is dead and every channel keeps about the same share of non-zero outputs."""
    c = sums.shape[1]
    shift = torch.floor(torch.quantile(sums.permute(1, 0, 2, 3).reshape(c, -1), quantile, dim=1))
    return (-shift + torch.randint(1, 16, (c,), generator=gen).double() * step).numpy().astype(np.float32)


def make_live(sd, m6a, dt, live, seed=0, settings=None):
    """Fill the Block17 of `live` (ascending) into sd, calibrating their biases on the fp32-carried trunk from m6a."""
    st = settings or SETTINGS[dt]
    trunk = m6a
    for k in sorted(live):
        p = "repeat_2.%d" % k
        gen = torch.Generator().manual_seed(6000 + 16 * seed + k)
        for name, cin, cout, (kh, kw), _ in BLOCK17:
            sd[p + "." + name + ".conv.weight"] = _sparse(gen, cout, cin, kh, kw, st.live_nz, cover=True)
        up = torch.from_numpy(_sparse(gen, 896, 256, 1, 1, st.up_nz, cover=True)).reshape(896, 256)
        up = up * torch.tensor(st.up_g, dtype=torch.float32)[torch.randint(0, len(st.up_g), (896, 256), generator=gen)]
        h =torch.randint(-15, 16, (896,), generator=gen).double() * st.in_step
        w10, h10 = (up * 10.0).numpy().astype(np.float32), (h * 10.0).numpy().astype(np.float32)
        assert np.array_equal(w10 * RES_SCALE17, up.numpy()) and np.array_equal(h10 * RES_SCALE17, h.numpy().astype(np.float32)), \
            "fl32(10 g * 0.1f) != g"
        sd[p + ".conv2d.weight"] = w10.reshape(896, 256, 1, 1)
        sd[p + ".conv2d.bias"] = h10
        # biases: calibrated convolution by convolution on this block's own input
        xb = stored(trunk, dt)
        W = lambda n: stored(_t64(sd[p + "." + n + ".conv.weight"]), dt)
        s0, s1 = conv_layer("", xb, W("branch0"), None, dt, sums_only=True), conv_layer("", xb, W("branch1.0"), None, dt, sums_only=True)
        _set_bn(sd, p + ".branch0", _calibrated(gen, s0, st.quantile[0], st.in_step))
        _set_bn(sd, p + ".branch1.0", _calibrated(gen, s1, st.quantile[0], st.in_step))
        t0 = conv_layer("", xb, W("branch1.0"), _t64(sd[p + ".branch1.0.bn.bias"]), dt)
        _set_bn(sd, p + ".branch1.1", _calibrated(gen, conv_layer("", t0, W("branch1.1"), None, dt, pad=(0, 3), sums_only=True), st.quantile[1], st.in_step))
        t1 = conv_layer("", t0, W("branch1.1"), _t64(sd[p + ".branch1.1.bn.bias"]), dt, pad=(0, 3))
        _set_bn(sd, p + ".branch1.2", _calibrated(gen, conv_layer("", t1, W("branch1.2"), None, dt, pad=(3, 0), sums_only=True), st.quantile[2], st.in_step))
        trunk = block17(block17_params(sd, k, dt), trunk, dt, p)
    return sd


@dataclass
class Case:
    dt: str
    live: tuple
    sd: dict
    x: torch.Tensor                 # (n,3,160,160) float64
    taps: dict                      # upstream taps, float64 NCHW (shared between the cases of a dtype: never written)
    log: list = field(default_factory=list)


_upstream = {}


def upstream_cached(dt, n=2, check=False):
    """(x, taps, log) of the base state dict on the first n images; self-checked once when check is asked for."""
    key = (dt, n)
    if key not in _upstream or (check and not _upstream[key][3]):
        x = images(dt, n)
        log = []
        taps = upstream(base_state_dict(dt), x, dt, log=log, check=check)
        _upstream[key] = (x, taps, log, check)
    return _upstream[key][:3]


def make_case(dt, live, n=2, settings=None):
    x, taps, _ = upstream_cached(dt, n)
    if settings is None and len(live) > 2:
        settings = replace(SETTINGS[dt], up_g=LONG_UP_G)
    sd = make_live(base_state_dict(dt), taps["mixed_6a"], dt, live, settings=settings)
    assert live_set(sd) == tuple(sorted(live))
    return Case(dt, tuple(sorted(live)), sd, x, taps)


def expected(case, carry="fp32", check=False, mut=None, mut_block=None):
    """The repeat_2 tap of a case, float64 NCHW; with check, self-checks every convolution of the live blocks and
    leaves their Recs in case.log."""
    log = [] if check else None
    out = repeat_2(case.sd, case.taps["mixed_6a"], case.dt, carry, log=log, check=check, mut=mut, mut_block=mut_block)
    if check:
        case.log = log
    return out


def bits(v):
    """float64 values -> the uint32 bits of the fp32 array Encoder.tap returns for them."""
    return np.ascontiguousarray(v.float().numpy()).view(np.uint32)


# the cases of the GPU test
SINGLES = tuple((k,) for k in range(10))
RUNS = ((0, 1), (4, 5), (8, 9), LONGEST)
