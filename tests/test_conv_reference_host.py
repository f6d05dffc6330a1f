"""Host checks of tests/conv_reference.py: the float64 restatement of the convolution formula against
torch.nn.functional.conv2d, the layout encoders against torch's own conversions, and the self-check that admits only
exact data sets -- on every geometry of the sweep's shape table.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr
from conv_reference import ACT_PRELU, ACT_RELU, CASES, DTYPES, SPLIT

GEOMS = [g for case in CASES.values() for g in case] + [cr.persistent_geom(293, 896, False), cr.persistent_geom(293, 896, True)]
PAIRS = [(g, dt) for g in GEOMS for dt in DTYPES if cr.with_dtype_alignment(g, dt) is not None]
IDS = ["%s-%s" % (g.name, dt) for g, dt in PAIRS]
# the split layouts have exact sets up to K = 256 only: 12-bit operands leave 10 of the budget's 22 bits for the sum
EXACT_PAIRS = [(g, dt) for g, dt in PAIRS if not (dt in SPLIT and g.K > cr.EXACT_MAX_K_SPLIT)]


def _conv2d_formula(g, dt, d, x_nchw, w, bias_map=None):
    """act(conv2d(x, w) + bias + res) with torch's convolution in float64, as (M, Cout)."""
    y = F.conv2d(x_nchw, w, None, stride=(g.sh, g.sw)).permute(0, 2, 3, 1).reshape(g.M, g.Cout)
    y = y + (d.bias.view(1, -1) if bias_map is None else bias_map)
    if d.res is not None:
        y = y + d.res
    if g.act == ACT_RELU:
        y = torch.relu(y)
    elif g.act == ACT_PRELU:
        y = F.prelu(y, d.slope)
    return y


def _pad(x_nhwc, g):
    return F.pad(x_nhwc.permute(0, 3, 1, 2), (g.pw, g.pw, g.ph, g.ph))


@pytest.mark.parametrize("g,dt", PAIRS, ids=IDS)
def test_restatement_is_conv2d_on_the_stored_values(g, dt):
    """Generic data.  Without a pre-BN the restatement and conv2d(stored x, stored w) + bias + res through the activation
    are the same float64 formula: they differ by float64 rounding only (1e-12 of sum |x*w|).  With a pre-BN the
    restatement holds the FOLDED form (w' = fp32(w*s), bias = fp32(b + fp32(sum over valid taps of w*t))) and is compared
    with conv2d(pad(x*s + t), w) in the f32 layout, where folding costs three fp32 roundings: 2^-24 of sum |x*w'| for w',
    2^-23 of |b| + |sum w*t| for the bias."""
    d = cr.generic_data(g, dt)
    v, absum = cr.conv_pre_store(g, dt, d)
    if not g.pre_bn:
        w = cr.stored(d.w, dt)
        want = _conv2d_formula(g, dt, d, _pad(d.x, g), w)
        assert ((v - want).abs() <= 1e-12 * absum + 1e-300).all()
        return
    if dt != "f32":
        # the folded weights are rounded to the layout: conv2d on those, plus the restatement's own per-pixel bias
        wf = cr.packed_weights(d.w, d.pre_s, dt).reshape(g.Cout, g.KH, g.KW, g.Cin).permute(0, 3, 1, 2).contiguous()
        _, valid = cr.im2col(d.x, g)
        want = _conv2d_formula(g, dt, d, _pad(d.x, g), wf, cr.bias_rows(d.w, d.bias, d.pre_t, valid))
        assert ((v - want).abs() <= 1e-12 * absum + 1e-300).all()
        return
    xb = d.x * d.pre_s.view(1, 1, 1, -1) + d.pre_t.view(1, 1, 1, -1)
    want = _conv2d_formula(g, dt, d, _pad(xb, g), d.w)
    shift = F.conv2d(_pad(torch.ones_like(d.x) * d.pre_t.abs().view(1, 1, 1, -1), g), d.w.abs(), None, stride=(g.sh, g.sw))
    shift = shift.permute(0, 2, 3, 1).reshape(g.M, g.Cout)
    bar = 2.0 ** -24 * absum + 2.0 ** -23 * (d.bias.abs().view(1, -1) + shift)
    assert ((v - want).abs() <= bar).all(), ((v - want).abs() / bar).max().item()


@pytest.mark.parametrize("g,dt", EXACT_PAIRS, ids=["%s-%s" % (g.name, dt) for g, dt in EXACT_PAIRS])
def test_exact_sets_are_exact_and_equal_conv2d(g, dt):
    """Every exact data set of the sweep passes the self-check (operands representable, budget inside 2^(22-q), float32
    forward = float32 reversed = float64), its expected outputs include values the store must round -- ties among them
    -- wherever the storage type is narrower than the 22 bits of the budget, and the restatement EQUALS conv2d in
    float64 (with a pre-BN: conv2d(pad(x*s + t), w), nothing folded), every operation on such data being exact."""
    for which in cr.exact_sets(dt):
        d = cr.exact_data(g, dt, which)
        rounded = cr.exact_self_check(g, dt, d)
        v, _ = cr.conv_pre_store(g, dt, d)
        if g.pre_bn:
            xb = d.x * d.pre_s.view(1, 1, 1, -1) + d.pre_t.view(1, 1, 1, -1)
            want = _conv2d_formula(g, dt, d, _pad(xb, g), d.w)
        else:
            want = _conv2d_formula(g, dt, d, _pad(d.x, g), d.w)
        assert torch.equal(v, want)
        if cr.rounding_can_bite(g, dt):
            od = cr.out_dtype(g, dt)
            ties = int(((v - cr.stored(v, od)).abs() * 2 == cr.store_ulp(v, od)).sum())
            assert rounded > 0 and ties > 0, (rounded, ties)
        if dt in SPLIT:   # the fine operand has lo halves, the coarse one none: lo * lo' is zero, not merely small
            fine, coarse = (d.x, d.w) if which == "xfine" else (d.w, d.x)
            assert (cr.split_pair(fine)[1] != 0).any() and (cr.split_pair(coarse)[1] == 0).all()
            if d.pre_s is not None:
                assert (cr.split_pair(d.w * d.pre_s.view(1, -1, 1, 1))[1] != 0).any() == (which == "wfine")


def test_self_check_rejects_inexact_data():
    g = CASES["A"][0]
    with pytest.raises(AssertionError):
        cr.exact_self_check(g, "bf16", cr.generic_data(g, "bf16"))
    d = cr.exact_data(g, "f16", "grid")
    d.x = d.x * 4097 / 4096          # 13 more bits per operand: not an f16 value
    with pytest.raises(AssertionError):
        cr.exact_self_check(g, "f16", d)
    d = cr.exact_data(g, "bf16", "grid")
    d.bias = d.bias + 2.0 ** 17      # on the grid, over the budget
    with pytest.raises(AssertionError):
        cr.exact_self_check(g, "bf16", d)


def test_layout_encoders_against_torch_conversions():
    gen = torch.Generator().manual_seed(5)
    x32 = torch.randn((2, 3, 5, 16), generator=gen) * torch.tensor([1e-6, 1e-3, 1.0, 300.0]).repeat(4)
    x32[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 2.0 ** -24, 65504.0])
    x = x32.double()
    assert torch.equal(cr.encode(x, "f32"), x32.view(torch.int32))
    assert torch.equal(cr.encode(x, "bf16"), x32.to(torch.bfloat16).view(torch.int16))      # torch rounds to nearest even
    assert torch.equal(cr.encode(x, "f16"), x32.half().view(torch.int16))
    planar, values = cr.to_planar(x32)
    assert torch.equal(cr.encode(x, "f16p"), planar)
    assert torch.equal(cr.decode(planar, "f16p"), values.double()) and torch.equal(cr.from_planar(planar).double(), values.double())
    hi, lo = cr._split(x32)
    pairs = torch.stack([hi, lo], dim=-1).contiguous().view(torch.int32).squeeze(-1)
    assert torch.equal(cr.encode(x, "f16x2"), pairs)
    for dt in DTYPES:
        assert torch.equal(cr.decode(cr.encode(x, dt), dt), cr.stored(x, dt)), dt
    # ties go to even, in float64 as well (no double rounding through fp32)
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert cr.stored(t, "bf16").tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]


def test_bias_rows_follow_tap_validity_not_border_classes():
    """Where add_conv's nine classes are right (stride 1, one padding row) the per-pixel bias is the class table's; at a
    refused geometry (stride 2 on an even height) the last output row keeps its bottom tap, which the table drops."""
    g = CASES["E"][1]
    d = cr.exact_data(g, "f16", "grid")
    _, valid = cr.im2col(d.x, g)
    rows = cr.bias_rows(d.w, d.bias, d.pre_t, valid).reshape(g.n, g.Ho, g.Wo, g.Cout)
    T = (d.w * d.pre_t.view(1, -1, 1, 1)).sum(1)                      # (Cout, KH, KW)
    for ho, kh in ((0, slice(1, 3)), (2, slice(0, 3)), (g.Ho - 1, slice(0, 2))):
        for wo, kw in ((0, slice(1, 3)), (1, slice(0, 3)), (g.Wo - 1, slice(0, 2))):
            assert torch.equal(rows[1, ho, wo], d.bias + T[:, kh, kw].sum((1, 2)))
    r = cr.REFUSED[0]
    _, valid = cr.im2col(torch.zeros((r.n, r.H, r.W, r.Cin), dtype=torch.float64), r)
    assert valid.reshape(r.n, r.Ho, r.Wo, 9)[0, r.Ho - 1, 1].tolist() == [1.0] * 9    # all nine taps inside the image
