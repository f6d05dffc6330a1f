"""tests/mtcnn_net_reference.py checked on the host: the layering against the oracle's own networks, the bars against
stand-ins for a correct device, and the bars' power against the faults a kernel of this cascade can have -- all on
the frames and rectangles tests/test_gpu_mtcnn_nets.py runs on the MI355X.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mtcnn_net_reference as R
from conftest import mtcnn_state_dicts
from conv_reference import rne, stored
from oracle import mtcnn as om

H, W = R.SIZES[0]
_F16 = (11, -14)


def _f32(v):
    return v.float().double()


@pytest.fixture(scope="module")
def inputs():
    """Per net: state dict, the oracle's crops of every rectangle on both frames (n,S,S,4: RGB + 0), frame of each row."""
    sds = mtcnn_state_dicts()
    fr, rc = R.frames(H, W), R.rectangles(H, W)
    idx = np.repeat(np.arange(2), len(rc))
    rects = np.concatenate([rc, rc])
    out = {}
    for net in (2, 3):
        c = R.oracle_crops(fr, idx, rects, R.S_OF[net])
        out[net] = (sds[net - 1], F.pad(c, (0, 1)).double(), c)
    return out


# ------------------------------------------------------------------------------------------------ the layering
@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("form", ("f32", "split", "mid"))
def test_layers_chained_in_float64_reproduce_the_oracles_networks(inputs, net, form):
    """Proves the layering, the dense permutation, the head column order and the NHWC view; the split forms' operands
    are 22-bit roundings of the fp32 ones, well inside the gate."""
    sd, x, c32 = inputs[net]
    for layer in R.layers(net, sd, form):
        x, _, _ = R.expected(layer, x, form)
    h = x.reshape(x.shape[0], -1)
    with torch.no_grad():
        ref = om.rnet_forward(sd, c32.permute(0, 3, 1, 2)) if net == 2 else om.onet_forward(sd, c32.permute(0, 3, 1, 2))
    prob = ref[-1][:, 1].double()
    vals = torch.cat([r.double() for r in ref[:-1]], dim=1)
    assert float((R.softmax1(h) - prob).abs().max()) <= 1e-5
    assert float((h[:, 2:2 + vals.shape[1]] - vals).abs().max()) <= 1e-5
    assert torch.equal(h[:, 2 + vals.shape[1]:], torch.zeros_like(h[:, 2 + vals.shape[1]:]))


# ------------------------------------------------------------------------------------------------ stand-ins for a device
def _halves(v):
    hi = rne(v, *_F16)
    return hi, v - hi


def _sum(layer, x, w, b, form, cross=True, swap_hw=False):
    """sum_k x*w + bias as a correct device may compute it, fp32 values in float64.  f32 form: torch's own fp32 layer.
    Split forms: float64 products of the stored pairs with lo*lo' dropped (cross False: hi*hi' only), an fp32-rounded
    sum, then the fp32 bias."""
    if layer.kind == "conv":
        op = lambda a, ww, bb=None: F.conv2d(a[..., :ww.shape[1]].permute(0, 3, 1, 2), ww, bb).permute(0, 2, 3, 1)
    else:
        flat = (lambda a: a.reshape(a.shape[0], -1)) if swap_hw else R.flatten_whc
        op = lambda a, ww, bb=None: F.linear(flat(a), ww, bb).view(a.shape[0], 1, 1, -1)
    if not R.is_split(form):
        return op(x.float(), w.float(), b.float()).double()
    xh, xl = _halves(x)
    wh, wl = _halves(w)
    s = op(xh, wh) + ((op(xh, wl) + op(xl, wh)) if cross else 0.0)
    return _f32(_f32(s) + b)


def _pool_short(v, k, axis):
    """max_pool(k, 2, ceil) whose LAST window along `axis` (1: rows, 2: columns) loses its last valid element."""
    P, C = R.max_pool(v, k).shape[axis], v.shape[axis]
    lo, last = 2 * (P - 1), min(2 * (P - 1) + k, C) - 1
    assert last > lo and last > 2 * (P - 2) + k - 1     # the window keeps an element, and `last` belongs to no other window
    cut = v.clone()
    cut.select(axis, last).fill_(-float("inf"))
    return R.max_pool(cut, k)


def standin(layer, x, form, fault=None):
    """The stored values a device would leave in the layer's tap from the decoded src tap x; `fault` one of FAULTS."""
    od = R.store_dtype(form)
    if layer.kind == "pool":
        if fault in ("pool_short_row", "pool_short_col"):
            return _pool_short(x, layer.pool, 1 if fault.endswith("row") else 2)
        out = R.max_pool(x, layer.pool).clone()
        if fault in ("pool_floor_row", "pool_floor_col"):
            out.select(1 if fault.endswith("row") else 2, out.shape[1] - 1).zero_()
        return out
    xo, w = R.operands(layer, x, form)
    b, slope = layer.b, layer.slope
    if fault and fault[:-3] in ("slope_c", "bias_c"):
        sh = {"+01": -1, "-01": 1, "+16": -16, "-16": 16}[fault[-3:]]     # channel c takes the value of channel c +- d
        if fault.startswith("slope"):
            slope = torch.roll(slope, sh)
        else:
            b = torch.roll(b, sh)
    if fault == "w_lo_dropped":     # in one 16-channel tile: the second where the layer has two
        w = w.clone()
        t0 = 16 if w.shape[0] >= 32 else 0
        w[t0:t0 + 16] = rne(w[t0:t0 + 16], *_F16)
    if fault == "heads_order":
        order = torch.cat(list(reversed(torch.split(torch.arange(w.shape[0]), list(layer.pieces)))))
        w, b = w[order], b[order]
    v = _sum(layer, xo, w, b, form, cross=fault != "cross_dropped", swap_hw=fault == "dense_hw_swapped")
    if fault in ("tap_lost_row", "tap_lost_col"):
        w2 = w.clone()
        w2[:, :, 2, 2] = 0.0
        v2 = _sum(layer, xo, w2, b, form)
        ax = 1 if fault.endswith("row") else 2
        v.select(ax, v.shape[ax] - 1).copy_(v2.select(ax, v.shape[ax] - 1))
    if slope is not None:
        v = torch.where(v > 0, v, _f32(v * _f32(slope)))
    if layer.pool:
        if fault in ("pool_short_row", "pool_short_col"):
            v = _pool_short(v, layer.pool, 1 if fault.endswith("row") else 2)
        else:
            v = R.max_pool(v, layer.pool)
            if fault in ("pool_floor_row", "pool_floor_col"):
                v.select(1 if fault.endswith("row") else 2, v.shape[1] - 1).zero_()
    v = R._pad_c(v, layer.cpad)
    if fault == "pad_channels_nonzero":
        v[..., 28:32] = v[..., 0:4]
    return stored(v, od)


def applies(fault, layer, net, form):
    """Can the layer's kernel have this fault at all?"""
    conv3x3 = layer.kind == "conv" and layer.w.shape[-1] == 3
    if fault.startswith("tap_lost"):
        return conv3x3
    if fault.startswith("pool_floor"):      # only where floor mode is one short: (C - k) odd
        return bool(layer.pool) and layer.name == "pool1"
    if fault.startswith("pool_short"):
        return bool(layer.pool)
    if fault.startswith("slope_c"):
        return layer.slope is not None and (fault[-2:] == "01" or layer.w.shape[0] >= 32)
    if fault.startswith("bias_c"):
        return layer.kind != "pool" and (fault[-2:] == "01" or layer.w.shape[0] >= 32)
    if fault == "pad_channels_nonzero":
        return net == 2 and layer.name == "pool1"
    if fault in ("w_lo_dropped", "cross_dropped"):
        return R.is_split(form) and layer.kind != "pool"
    if fault == "dense_hw_swapped":
        return layer.kind == "dense"
    if fault == "heads_order":
        return layer.kind == "heads"
    raise KeyError(fault)


FAULTS = ("tap_lost_row", "tap_lost_col", "pool_floor_row", "pool_floor_col", "pool_short_row", "pool_short_col",
          "slope_c+01", "slope_c-01", "slope_c+16", "slope_c-16", "bias_c+01", "bias_c-01", "bias_c+16", "bias_c-16",
          "pad_channels_nonzero", "w_lo_dropped", "cross_dropped", "dense_hw_swapped", "heads_order")


@pytest.fixture(scope="module")
def chains(inputs):
    """Per (net, form): [(layer, the stand-in's stored src tap)] -- what a correct device would hand each layer."""
    out = {}
    for net in (2, 3):
        sd, x0, _ = inputs[net]
        for form in R.FORMS:
            x, ch = x0, []
            for layer in R.layers(net, sd, form):
                ch.append((layer, x))
                x = standin(layer, x, form)
            out[net, form] = (ch, x)
    return out


@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("form", R.FORMS)
def test_a_correct_device_stays_within_the_bar_on_every_layer(chains, net, form):
    ch, _ = chains[net, form]
    for layer, x in ch:
        ok, (rel, to_bar, to_fig) = R.check_layer(layer, x, standin(layer, x, form), form)
        print("net %d %-5s %-6s  err/A %.3e  /bar %.3f  /4e-7 figure %.3f" % (net, form, layer.name, rel, to_bar, to_fig))
        assert bool(ok.all()), (net, form, layer.name, to_bar)


def test_pools_floor_mode_is_one_short_only_at_pool1():
    """Where pool_floor does not apply, floor and ceil mode give the same map: nothing to get wrong."""
    for S, sizes in ((24, {"pool1": (22, 3), "pool2": (9, 3)}), (48, {"pool1": (46, 3), "pool2": (21, 3), "pool3": (8, 2)})):
        for name, (C, k) in sizes.items():
            assert ((C - k) % 2 == 1) == (name == "pool1")


# ------------------------------------------------------------------------------------------------ the bars' power
# The one (net, layer, fault) the derived bar leaves room for on any realistic input: the gate grows with K + 2, and at
# O-Net's dense layer (K = 1152) the lo halves of ONE 16-channel tile move an element by 0.39 .. 0.67 of its bar, whichever
# tile is taken (R-Net's dense, K = 576: 1.02 .. 1.41).  The fault is caught at the six other O-Net layers; losing the lo
# halves of the whole layer is caught here too.
BLIND = {(3, "dense", "w_lo_dropped")}


def _expected_faults(net, form):
    return {f for f in FAULTS if (net == 2 or f != "pad_channels_nonzero") and (R.is_split(form) or f not in ("w_lo_dropped", "cross_dropped"))}


@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("form", R.FORMS)
def test_every_fault_puts_its_layers_tap_beyond_the_bar(chains, net, form):
    """Each fault goes into a copy of the stand-in of ONE layer, at every layer whose kernel could have it; at least one
    element of that layer's tap must then miss its bar on the GPU test's own inputs.  A miss rejects the inputs."""
    ch, _ = chains[net, form]
    seen = set()
    for layer, x in ch:
        for f in FAULTS:
            if not applies(f, layer, net, form):
                continue
            ok, (_, to_bar, _) = R.check_layer(layer, x, standin(layer, x, form, f), form)
            print("net %d %-5s %-6s %-22s beyond %6d  worst/bar %.3g" % (net, form, layer.name, f, int((~ok).sum()), to_bar))
            if (net, layer.name, f) in BLIND:
                continue
            assert not bool(ok.all()), (net, form, layer.name, f, to_bar)
            seen.add(f)
    assert seen == _expected_faults(net, form)


@pytest.mark.parametrize("net", (2, 3))
def test_table_and_slot_faults_are_visible_on_these_inputs(inputs, chains, net):
    """The faults the bit checks are there for: a candidate reading its neighbour's crop (slot k - c0 +- 1), the second
    frame's rows starting at offset 0, softmax column 0 for column 1."""
    _, x0, _ = inputs[net]
    n = x0.shape[0] // 2
    for sh in (1, -1):       # no crop equals its neighbour's, on either side, across the frame boundary included
        assert bool((x0 != torch.roll(x0, sh, 0)).flatten(1).any(1).all())
    for form in R.FORMS:
        _, h = chains[net, form]
        h = h.reshape(2 * n, -1)
        # frame 1 read from offset 0 would repeat frame 0's rows: every row's value columns differ in their bits
        assert bool((h[:n, 2:R.NF_OF[net] + 1] != h[n:, 2:R.NF_OF[net] + 1]).any(1).all())
        p1, p0 = R.softmax1(h), torch.softmax(h[:, :2], dim=1)[:, 0]
        assert int(((p1 - p0).abs() > 1e-6).sum()) >= 2 * n - 2
