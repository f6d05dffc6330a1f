"""Block8 branch chain in one launch (block8_chain_kernel, bit 6 of VNF_FUSE) against the three plan convolutions it
replaces in each of the six blocks of repeat_3 / block8: the fused reducer 1x1 1792 -> (192 | 192), branch1.1 (1x3) and
branch1.2 (3x1).  The kernel uses the plan's MFMA, k order, epilogue and rounding points, so every tensor behind it must be
the same bytes -- apart from the order of profile rows, which the forms do not share, no comparison here has a tolerance.

A workgroup owns G = 3 whole 3x3 images (27 of its 32 pixel rows).  The batches:
  n = 1    a single partial group (9 valid rows, the second pixel tile all padding);
  n = 5    a full group and a partial one of 2 images (G - 1);
  n = 8    two full groups and a remainder of 2;
  n = 16   five full groups and a remainder of 1.
Inputs are seeded N(0,1) crops in the compute dtype.

The switches are read when a handle is created, so each form is a model of its own from the same seeded state dict, with the
heuristic tiles (VNF_AUTOTUNE=0: quick creates).  One max_batch = 16 handle per (dtype, switch) serves every case of this
file; the cases that are about what an earlier call left behind say in which order they call it."""
import os

import numpy as np
import pytest
import torch

from conftest import seeded_normal

pytestmark = pytest.mark.gpu

CROPS = {"bf16": torch.bfloat16, "f16": torch.float16, "f16x2": torch.float32}
MAX_N = 16
TAPS = ("mixed_7a", "repeat_3", "block8")
_models = {}
_inputs = {}


def _model(dt, fuse):
    """The max_batch = 16 model of (dtype, VNF_FUSE); fuse None: the default switch."""
    key = (dt, fuse)
    if key not in _models:
        from vn_celeb_face_recognition_amd.models import InceptionResnetV1
        keep = {k: os.environ.get(k) for k in ("VNF_FUSE", "VNF_AUTOTUNE")}
        os.environ["VNF_AUTOTUNE"] = "0"
        if fuse is None:
            os.environ.pop("VNF_FUSE", None)
        else:
            os.environ["VNF_FUSE"] = str(fuse)
        try:
            m = InceptionResnetV1(pretrained=None, device="cuda:0", compute_dtype=dt, max_batch=MAX_N).eval()
            m._ensure_handle()                           # the handle reads the switches here
        finally:
            for k, v in keep.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _models[key] = m
    return _models[key]


def _x(dt, n):
    """The first n of the 16 seeded crops of a dtype (image i is the same tensor at every batch size)."""
    if dt not in _inputs:
        _inputs[dt] = seeded_normal((MAX_N, 3, 160, 160), 808).to(CROPS[dt]).cuda()
    return _inputs[dt][:n].contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _embed(m, x):
    return _bits(m(x).cpu().numpy())


def _run(m, x, n):
    emb = _embed(m, x)
    return {t: _bits(m.tap(t, n)) for t in TAPS}, emb


@pytest.mark.parametrize("n", [1, 5, 8, 16])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_chain_kernel_is_bitwise_the_three_plan_convolutions(dt, n):
    x = _x(dt, n)
    taps, emb = _run(_model(dt, 64), x, n)
    want_taps, want = _run(_model(dt, 0), x, n)
    assert taps["mixed_7a"].shape == (n, 1792, 3, 3)
    for t in TAPS:
        assert np.isfinite(taps[t].view(np.float32)).all() and taps[t].any(), (dt, n, t)
        bad = np.argwhere(taps[t] != want_taps[t])
        assert len(bad) == 0, (dt, n, t, len(bad), bad[:4])
    assert np.isfinite(emb.view(np.float32)).all()
    assert np.array_equal(emb, want), (dt, n)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rows_an_earlier_larger_batch_left_behind_a_partial_group_do_not_reach_it(dt):
    """n = 16 fills every row of the handle's buffers; the n = 5 call behind it has a last group of 2 images whose third
    image's rows (and the images behind) still hold the earlier batch."""
    fused, plan = _model(dt, 64), _model(dt, 0)
    _embed(fused, _x(dt, 16))
    got_taps, got = _run(fused, _x(dt, 5), 5)
    want_taps, want = _run(plan, _x(dt, 5), 5)
    for t in TAPS:
        assert np.array_equal(got_taps[t], want_taps[t]), (dt, t)
    assert np.array_equal(got, want), dt


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_an_image_embeds_the_same_at_every_position_of_a_group(dt):
    m = _model(dt, 64)
    batch = _embed(m, _x(dt, 16))
    x = _x(dt, 16)
    for i in range(16):
        alone = _embed(m, x[i:i + 1].contiguous())
        assert np.array_equal(alone[0], batch[i]), (dt, i)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_default_switch_embeds_like_the_plan_without_bit_6(dt):
    x = _x(dt, 8)
    got = _embed(_model(dt, None), x)
    want = _embed(_model(dt, 31), x)
    assert np.isfinite(got.view(np.float32)).all() and got.any()
    assert np.array_equal(got, want), dt


def _tail_rows(m, x):
    rows = [line[:28].strip() or line.split()[0] for line in m.profile(x).splitlines() if line.strip()]
    return [r for r in rows if r.startswith(("repeat_3.", "block8"))]


def test_chain_kernel_is_in_the_plan_and_the_split_f16_plan_keeps_its_convolutions():
    for m, dt in ((_model("bf16", 64), "bf16"), (_model("bf16", None), "bf16"), (_model("f16", None), "f16")):
        rows = _tail_rows(m, _x(dt, 8))
        chain = [r for r in rows if " chain" in r]
        assert len(chain) == 6 and sum(r.startswith("repeat_3.") for r in chain) == 5 and sum(r.startswith("block8 ") for r in chain) == 1, rows
        assert not [r for r in rows if "branch1.1" in r or "branch1.2" in r or "reduce" in r.replace("(reduce", "")], rows
        assert len([r for r in rows if "conv2d" in r]) == 6, rows   # the up-projections stay plan convolutions
    rows = _tail_rows(_model("f16x2", None), _x("f16x2", 8))
    assert not [r for r in rows if " chain" in r], rows
    for part in ("reduce", "branch1.1", "branch1.2", "conv2d"):
        assert len([r for r in rows if r.endswith(part)]) == 6, (part, rows)
    rows = _tail_rows(_model("bf16", 0), _x("bf16", 8))
    assert not [r for r in rows if " chain" in r] and len([r for r in rows if r.endswith("branch1.2")]) == 6, rows


def test_flops_per_image_do_not_depend_on_the_switch():
    assert _model("bf16", 64).flops_per_image() == _model("bf16", 0).flops_per_image()
    assert _model("f16", None).flops_per_image() == _model("f16", 31).flops_per_image()
